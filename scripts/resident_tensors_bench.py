"""Probe: a learner's closed loop at the resident loop's batch sizes - one float32 [n, 46] action tensor in (velocity 3, IMU 7, tip force 18, joint
effort 18 columns), q / qd of the cycle back as one float32 [n, 36] tensor, one tick per iteration - by three routes on one GPU.
Engines: 6x3 hexapods with config 3's parameter set and joint efforts live, three twins on one stream s, which also carries the torch kernels.
  (a) resident tensors:  shc_engine_resident_post_actions(tensor, publish) + shc_engine_resident_get_observations_async
                         - post kernel, device-side wait, read kernel; no host wait
  (b) resident, before:  six torch kernels on s that cut the groups out of the tensor as contiguous float64 arrays, a synchronise of s (the
                         ordinary post reads them on the engine's input stream, which nothing orders behind s), shc_engine_resident_post(on_device,
                         publish), shc_engine_resident_get_joint_state_async (wait + two gathers), then the cast to float32 and the concatenation as
                         two torch copy kernels into the halves of the row (torch.cat finds no room beside a loop of 16 384 hexapods)
  (c) launches:          shc_engine_set_actions + shc_engine_step(1) + shc_engine_get_observations
Only one resident loop is alive at a time (16 384 hexapods fill most of the chip): a block of a resident route is resident_begin, a few ticks
of warm-up, --iters ticks between two HIP events on s (the window ends in the event's synchronise), resident_end.  The routes alternate block by
block, medians over --rounds rounds after one warm-up round.  Every engine sees the same tensor in the same number of ticks: afterwards the last
observation tensors and the state records of (a) and (b) must be equal (and those of (c), which runs the same cycles as launches).
The library is called through ctypes with specs built once, so that the wrapper's per-call marshalling is in no route.
Not a test and not part of bench.py.
Usage: python scripts/resident_tensors_bench.py [--sizes 4096 16384] [--out profiles/bench/resident_tensors.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")
# launches per tick, read off the code, not counted at run time
LAUNCHES = {"resident_tensors": {"engine": 3, "torch": 0, "host_syncs": 0}, "resident_before": {"engine": 4, "torch": 8, "host_syncs": 1},
            "launches": {"engine": 3, "torch": 0, "host_syncs": 0}}
WARM = 8


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine, CycleInputs, act_spec, action_columns, obs_spec

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
    lib = a.L
    cols, W = action_columns(FIELDS, L, D)
    rows = np.zeros((n, W))
    rows[:, cols["linear_xy"]], rows[:, cols["angular"]] = lin * 0.5, ang[:, None] * -1.0
    rows[:, cols["imu_orientation"]] = rng.normal(0, 0.05, (n, 4)) + np.array([1.0, 0.0, 0.0, 0.0])
    rows[:, cols["imu_angular_velocity"]] = rng.normal(0, 0.05, (n, 3))
    rows[:, cols["tip_force"]], rows[:, cols["joint_effort"]] = force.reshape(n, -1) * 0.9, effort * 0.7
    with torch.cuda.stream(s):
        tensor = torch.from_numpy(rows).to(torch.float32).cuda()
        obs = {name: torch.zeros((n, 2 * L * D), dtype=torch.float32, device="cuda") for name in LAUNCHES}
        q64, qd64 = (torch.zeros((n, L * D), dtype=torch.float64, device="cuda") for _ in range(2))
    s.synchronize()
    aspec, ospec = act_spec(FIELDS, L, D, "float32"), obs_spec(("q", "qd"), L, D, "float32")
    tptr = C.c_void_p(tensor.data_ptr())
    optr = {name: C.c_void_p(t.data_ptr()) for name, t in obs.items()}

    def tick_a(cycle):
        rc = lib.shc_engine_resident_post_actions(a.h, C.byref(aspec), tptr, 1, None)
        rc |= lib.shc_engine_resident_get_observations_async(a.h, cycle, C.byref(ospec), optr["resident_tensors"], 0)
        assert rc == 0, lib.shc_last_error()

    ci = CycleInputs()
    ci.on_device, ci.publish = 1, 1

    def tick_b(cycle):
        g = {name: tensor[:, cols[name]].double() for name in FIELDS}     # (contiguous float64 copies: six torch kernels on s)
        s.synchronize()                                                    # the ordinary post reads them on the engine's input stream
        ci.linear_xy, ci.angular = g["linear_xy"].data_ptr(), g["angular"].data_ptr()
        ci.imu_orientation_wxyz, ci.imu_angular_velocity = g["imu_orientation"].data_ptr(), g["imu_angular_velocity"].data_ptr()
        ci.tip_force, ci.joint_effort = g["tip_force"].data_ptr(), g["joint_effort"].data_ptr()
        rc = lib.shc_engine_resident_post(b.h, C.byref(ci), None)
        rc |= lib.shc_engine_resident_get_joint_state_async(b.h, cycle, C.c_void_p(q64.data_ptr()), C.c_void_p(qd64.data_ptr()), 0)
        assert rc == 0, lib.shc_last_error()
        # the cast and the concatenation as two cast-and-place kernels.  (torch.cat itself cannot be used here: its 512-thread workgroups need
        # eight free wave slots on one compute unit, which 1 640 loop wavefronts at 16 384 hexapods leave nowhere - the kernel, and the stream
        # behind it, would wait until the loop has left by its idle timeout.)
        obs["resident_before"][:, :L * D].copy_(q64)
        obs["resident_before"][:, L * D:].copy_(qd64)
        return g   # (alive until the next tick's synchronise: the post kernel has read them by then)

    def tick_c(cycle):
        rc = lib.shc_engine_set_actions(c.h, C.byref(aspec), tptr, 1)
        rc |= lib.shc_engine_step(c.h, 1)
        rc |= lib.shc_engine_get_observations(c.h, 0, n, C.byref(ospec), optr["launches"], 1)
        assert rc == 0, lib.shc_last_error()

    routes = (("resident_tensors", a, tick_a), ("resident_before", b, tick_b), ("launches", None, tick_c))
    times = {name: [] for name, _, _ in routes}
    with torch.cuda.stream(s):
        for r in range(rounds + 1):
            for name, eng, tick in routes:
                if eng is not None:
                    eng.resident_begin(ring_depth=8, max_cycles=WARM + iters + 8)
                keep = None
                for k in range(WARM):
                    keep = tick(k)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(s)
                for k in range(WARM, WARM + iters):
                    keep = tick(k)
                t1.record(s)
                t1.synchronize()
                del keep
                if r > 0:
                    times[name].append(t0.elapsed_time(t1) * 1e3 / iters)
                if eng is not None:
                    assert eng.resident_end() == WARM + iters
    s.synchronize()
    for e in engines:
        e.synchronize()
    last = {name: t.cpu().numpy().tobytes() for name, t in obs.items()}
    state = [bytes(memoryview(e.get_state()).cast("B")) for e in engines]
    row = {"n": n, "action_columns": W, "observation_columns": 2 * L * D, "iters": iters, "rounds": rounds, "launches_per_tick": LAUNCHES,
           "outputs_equal_tensors_vs_before": bool(last["resident_tensors"] == last["resident_before"] and state[0] == state[1]),
           "outputs_equal_tensors_vs_launches": bool(last["resident_tensors"] == last["launches"] and state[0] == state[2])}
    for name, ts in times.items():
        row[name] = {"us_per_tick_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    ta, tb = row["resident_tensors"], row["resident_before"]
    spread = max(ta["us_max"] - ta["us_min"], tb["us_max"] - tb["us_min"])
    row["ratio_tensors_over_before"] = ta["us_per_tick_median"] / tb["us_per_tick_median"]
    row["tensors_not_slower_than_before_beyond_spread"] = bool(ta["us_per_tick_median"] <= tb["us_per_tick_median"] + spread)
    for e in engines:
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": "float32 [n, 46]: " + ", ".join(FIELDS) + "; back: float32 [n, 36] q, qd",
              "expectation": "resident_tensors is not slower than resident_before at either size beyond the rounds' own min-max spread, with fewer launches per tick",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["outputs_equal_tensors_vs_before"] for r in result["sizes"]):
        sys.exit("the routes left different outputs")


if __name__ == "__main__":
    main()
