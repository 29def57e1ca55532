"""Probe: a K = 16 rollout of 6x3 hexapods driven by one float32 [K, n, 46] action tensor - velocity 3, IMU 7, tip force 18, joint effort 18
columns - with every cycle's joints handed back as one float32 [K, n, 36] tensor, through the rollout tensors and through the route a caller had
before them, on one GPU.
Engines: config 3's parameter set, three of them (one per route), 100 cycles of walking with joint efforts live before the timing; all run on one
stream s, which also carries the torch kernels of route (b).
  (a) rollout tensors: shc_engine_step_k_actions(tensor) + shc_engine_get_step_k_observations(q, qd)   - 1 stage kernel, the launch, 1 read kernel
  (b) today's route:   six torch kernels on s that cut the six groups out of the same tensor as contiguous float64 arrays
                       (tensor[..., columns].double().contiguous()), shc_engine_step_k on them, K x shc_engine_get_step_k_joint_state into
                       float64 device buffers (2 gather kernels each), the torch concatenation and cast into [K, n, 36] float32
                                                                                                         - 6 + the launch + 2 K + 2 kernels
  (c) bare step_k:     shc_engine_step_k on float64 arrays that are ready, nothing read back - what both routes are overhead over
Each route runs --iters times back to back between two HIP events on s (the window ends in the event's synchronise); the routes alternate block by
block, medians with min - max over --rounds rounds after one warm-up round of all three.  Afterwards the output tensors of (a) and (b) must be
equal, and the state records of the three engines (they have taken the same rows the same number of times).
The expectation, stated before the first run: (a) is not slower than (b) at either size by more than the rounds' own spread, and its overhead over
(c) is smaller than (b)'s.  Not a test and not part of bench.py.
Usage: python scripts/rollout_bench.py [--sizes 65536 4096] [--out profiles/bench/rollout.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")
K = 16


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
    engines = [BatchEngine(p, n, stream=s.cuda_stream) for _ in range(3)]
    for e in engines:
        e.set_velocity(lin, ang)
        e.set_tip_force(force)
        e.set_joint_effort(effort)
        e.step(100)
        e.synchronize()
    a, b, c = engines
    cols, W = action_columns(FIELDS, L, D)
    rows = np.zeros((K, n, W), dtype=np.float32)
    for k in range(K):   # every cycle its own rows
        rows[k, :, cols["linear_xy"]], rows[k, :, cols["angular"]] = lin * (0.5 + 0.02 * k), ang[:, None] * (-1.0 + 0.05 * k)
        rows[k, :, cols["imu_orientation"]] = rng.normal(0, 0.05, (n, 4)) + np.array([1.0, 0.0, 0.0, 0.0])
        rows[k, :, cols["imu_angular_velocity"]] = rng.normal(0, 0.05, (n, 3))
        rows[k, :, cols["tip_force"]], rows[k, :, cols["joint_effort"]] = force.reshape(n, -1) * (0.9 if k % 4 else 0.0), effort * (0.7 - 0.01 * k)
    tensor = torch.from_numpy(rows).cuda()

    def cut():
        return {name: tensor[..., cols[name]].double().contiguous() for name in FIELDS}
    out_a = torch.zeros((K, n, 2 * L * D), dtype=torch.float32, device="cuda")
    q64, qd64 = (torch.zeros((K, n, L * D), dtype=torch.float64, device="cuda") for _ in range(2))
    ready = cut()
    torch.cuda.synchronize()
    out_b = [None]

    def step_k(eng, g):
        ptr = {name: t.data_ptr() for name, t in g.items()}
        eng.step_k(K, velocity=(ptr["linear_xy"], ptr["angular"]), imu=(ptr["imu_orientation"], ptr["imu_angular_velocity"]),
                   tip_force=ptr["tip_force"], joint_effort=ptr["joint_effort"])

    def rollout_tensors(eng=a):
        eng.step_k_actions(tensor, FIELDS)
        eng.step_k_observations(("q", "qd"), out=out_a)

    def todays_route(eng=b):
        with torch.cuda.stream(s):
            g = cut()
        step_k(eng, g)
        lib, h, row = eng.L, eng.h, n * L * D * 8
        rc = 0
        for k in range(K):   # (each joins a split launch first: the six arrays are no longer read when this function returns them to s's pool)
            rc |= lib.shc_engine_get_step_k_joint_state(h, k, C.c_void_p(q64.data_ptr() + k * row), C.c_void_p(qd64.data_ptr() + k * row), 1)
        assert rc == 0
        with torch.cuda.stream(s):
            out_b[0] = torch.cat((q64, qd64), dim=2).float()

    def bare_step_k(eng=c):
        step_k(eng, ready)

    routes = (("rollout_tensors", rollout_tensors, a), ("todays_route", todays_route, b), ("bare_step_k", bare_step_k, c))
    times = {name: [] for name, _, _ in routes}
    for r in range(rounds + 1):
        for name, fn, eng in routes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(iters):
                fn()
            eng.join()   # (a large batch launches on the engine's two half streams: s follows them - events, no host wait - before the window closes)
            t1.record(s)
            t1.synchronize()
            if r > 0:
                times[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    for e in engines:
        e.synchronize()
    torch.cuda.synchronize()
    outputs_equal = bool(torch.equal(out_a, out_b[0]))
    state = [bytes(memoryview(e.get_state()).cast("B")) for e in engines]
    row = {"n": n, "K": K, "columns": W, "iters": iters, "rounds": rounds, "outputs_equal": outputs_equal,
           "state_bytes_equal": bool(state[0] == state[1] == state[2]),
           "launches_per_call": {"rollout_tensors": {"engine": 3, "torch": 0}, "todays_route": {"engine": 1 + 2 * K, "torch": 8}, "bare_step_k": {"engine": 1, "torch": 0}}}
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    med = {name: row[name]["us_per_call_median"] for name in times}
    spread = max(row[name]["us_max"] - row[name]["us_min"] for name in ("rollout_tensors", "todays_route"))
    row["overhead_over_bare_us"] = {name: med[name] - med["bare_step_k"] for name in ("rollout_tensors", "todays_route")}
    row["ratio_tensors_over_today"] = med["rollout_tensors"] / med["todays_route"]
    row["cycles_per_s"] = {name: K * n / (med[name] * 1e-6) for name in times}
    row["expectation_met"] = bool(med["rollout_tensors"] <= med["todays_route"] + spread and
                                  row["overhead_over_bare_us"]["rollout_tensors"] < row["overhead_over_bare_us"]["todays_route"])
    for e in engines:
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": f"float32 [{K}, n, 46]: " + ", ".join(FIELDS), "observations": f"float32 [{K}, n, 36]: q, qd",
              "expectation": "rollout_tensors is not slower than todays_route at either size by more than the rounds' own spread, and its overhead "
                             "over bare_step_k is smaller than todays_route's",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["outputs_equal"] and r["state_bytes_equal"] for r in result["sizes"]):
        sys.exit("the routes left different outputs or engines")


if __name__ == "__main__":
    main()
