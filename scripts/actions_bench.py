"""Probe: a policy's action tensor - velocity 3, IMU 7, tip force 18, joint effort 18 columns of every robot as one float32 [n, 46] device tensor -
into an engine through the action pass and through the route a caller had before it, on one GPU.
Engines: 6x3 hexapods with config 3's parameter set, two of them (one per route), 100 cycles of walking with joint efforts live before the timing;
both run on one stream s, which also carries the torch kernels of route (b).
  (a) action pass:   shc_engine_set_actions(tensor)                                                    - 1 kernel
  (b) setters route: six torch kernels on s that cut the six groups out of the same tensor as contiguous float64 arrays
                     (tensor[:, columns].double(): one strided cast-and-copy each), then the four device setters
                     (velocity 2, IMU 2, tip force 1, joint effort 1 scatter kernels)                   - 6 + 6 kernels
Each route runs --iters times back to back between two HIP events on s (the window ends in the event's synchronise); (a) and (b) alternate block by
block, medians over --rounds rounds after one warm-up round of both.  Afterwards both engines take one more call each with the same tensor and
their state records must be equal, then - the inputs are held inputs, no part of the record - three cycles later their joints.
Not a test and not part of bench.py.
Usage: python scripts/actions_bench.py [--sizes 65536 4096] [--out profiles/bench/actions.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")
LAUNCHES = {"action_pass": {"engine": 1, "torch": 0}, "setters_route": {"engine": 6, "torch": 6}}   # read off the code, not counted at run time


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine, action_columns

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    s = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    L, D = 6, 3
    lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n)
    force = np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 15, (n, L))], axis=2))
    effort = rng.normal(0, 0.5, (n, L * D))
    engines = [BatchEngine(p, n, stream=s.cuda_stream) for _ in range(2)]
    for e in engines:
        e.set_velocity(lin, ang)
        e.set_tip_force(force)
        e.set_joint_effort(effort)
        e.step(100)
        e.synchronize()
    a, b = engines
    cols, W = action_columns(FIELDS, L, D)
    rows = np.zeros((n, W))
    rows[:, cols["linear_xy"]], rows[:, cols["angular"]] = lin * 0.5, ang[:, None] * -1.0
    rows[:, cols["imu_orientation"]] = rng.normal(0, 0.05, (n, 4)) + np.array([1.0, 0.0, 0.0, 0.0])
    rows[:, cols["imu_angular_velocity"]] = rng.normal(0, 0.05, (n, 3))
    rows[:, cols["tip_force"]], rows[:, cols["joint_effort"]] = force.reshape(n, -1) * 0.9, effort * 0.7
    tensor = torch.from_numpy(rows).to(torch.float32).cuda()
    torch.cuda.synchronize()

    def action_pass(eng=a):
        eng.set_actions(tensor, FIELDS)

    def setters_route(eng=b):
        with torch.cuda.stream(s):
            g = {name: tensor[:, cols[name]].double() for name in FIELDS}
        assert all(t.is_contiguous() for t in g.values())
        ptr = {name: C.c_void_p(t.data_ptr()) for name, t in g.items()}
        lib, h = eng.L, eng.h
        rc = lib.shc_engine_set_velocity(h, ptr["linear_xy"], ptr["angular"], 1)
        rc |= lib.shc_engine_set_imu(h, ptr["imu_orientation"], ptr["imu_angular_velocity"], 1)
        rc |= lib.shc_engine_set_tip_force(h, ptr["tip_force"], 1)
        rc |= lib.shc_engine_set_joint_effort(h, ptr["joint_effort"], 1)
        assert rc == 0   # (the six arrays belong to s's allocator pool and the setters read them on s: a later reuse follows in stream order)

    routes = (("action_pass", action_pass), ("setters_route", setters_route))
    times = {name: [] for name, _ in routes}
    for r in range(rounds + 1):
        for name, fn in routes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(iters):
                fn()
            t1.record(s)
            t1.synchronize()
            if r > 0:
                times[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    action_pass(), setters_route()
    for e in engines:
        e.synchronize()
    state = [bytes(memoryview(e.get_state()).cast("B")) for e in engines]
    for e in engines:
        e.step(3)
    joints = [e.joints()[0].tobytes() + e.joints()[1].tobytes() for e in engines]
    row = {"n": n, "columns": W, "iters": iters, "rounds": rounds, "state_bytes_equal": bool(state[0] == state[1]),
           "joints_equal_3_cycles_later": bool(joints[0] == joints[1]), "launches_per_call": LAUNCHES}
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    row["ratio_pass_over_setters"] = row["action_pass"]["us_per_call_median"] / row["setters_route"]["us_per_call_median"]
    for e in engines:
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": "float32 [n, 46]: " + ", ".join(FIELDS), "expectation": "ratio < 1 at both sizes (one launch against twelve)",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["state_bytes_equal"] and r["joints_equal_3_cycles_later"] for r in result["sizes"]):
        sys.exit("the two routes left different engines")


if __name__ == "__main__":
    main()
