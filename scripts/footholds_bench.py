"""Probe: a foothold planner's request tensor - position 3, rotation 4, transform 7, clearance, frame and defined of every leg of every robot as one
float32 [n, 6 * 17] device tensor - into an engine and back out of it through the foothold pass, and through the only route a caller had before
it from the same device tensor, on one GPU.
Engines: 6x3 hexapods in rough terrain mode, two of them (one per route), 100 cycles of walking before the timing; both run on one stream s.
  (a) foothold pass:   shc_engine_set_footholds(tensor, on_device = 1, device count)                      - 1 kernel, no copy, no host wait
  (b) host route:      tensor.cpu(), the ExternalTarget rows filled with numpy through a structured dtype (vectorised, no Python loop),
                       shc_engine_set_external_target: its row-by-row conversion, hipMalloc, H2D copy, 1 kernel, D2H copy of the count,
                       stream synchronise, hipFree
  (c) read-back pass:  shc_engine_get_footholds(tensor, on_device = 1)                                    - 1 kernel
  (d) host read-back:  shc_engine_get_external_target (hipMalloc, 1 kernel, D2H copy, synchronise, hipFree, conversion), the float32 rows
                       filled with numpy from the structured array, torch.from_numpy(..).cuda()
For orientation the action pass (scripts/actions_bench.py: its engine, its float32 [n, 46] tensor) is timed in the same run as (e).
Each route runs its iterations back to back between two HIP events on s (the window ends in the event's synchronise, and contains the host's
share of a route: the second event is recorded when the host gets there); the routes alternate block by block, medians over --rounds rounds
after one warm-up round of all.  The host routes take --iters / 20 iterations (at least 3): one of them takes milliseconds.  Afterwards both
engines take one more call each with the same tensor and their state records, auxiliary blobs and dropped-row counts must be equal, and (c) and
(d) must have produced the same tensor.
Not a test and not part of bench.py.
Usage: python scripts/footholds_bench.py [--sizes 65536 4096] [--out profiles/bench/footholds.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACTION_FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import FH_FIELD_NAMES, BatchEngine, action_columns, foothold_columns, generate_tables
    from syropod_highlevel_controller_amd.params import ExternalTarget

    L = 6
    p = default_hexapod_params("tripod")
    p.rough_terrain_mode = 1
    s = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    lin, ang = rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.4, 0.4, n)
    lin[::16], ang[::16] = 0.0, 0.0                 # one robot in sixteen stands: its targets go to its poser, its defaults are dropped
    tables = generate_tables(p)
    engines = [BatchEngine(p, n, stream=s.cuda_stream, tables=tables) for _ in range(2)]
    for e in engines:
        e.set_velocity(lin, ang)
        e.step(100)
        e.synchronize()
    a, b = engines
    tips = a.leg_state()["walker_tip"].reshape(n, L, 3)
    b.leg_state()
    fields = tuple(FH_FIELD_NAMES)
    cols, W = foothold_columns(fields, L)
    block = {"position": tips + np.array([0.02, -0.01, 0.0]), "rotation": np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, L, 1)),
             "transform": np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (n, L, 1)), "swing_clearance": np.full((n, L, 1), 0.02),
             "frame_is_odom_ideal": (rng.uniform(size=(n, L, 1)) < 0.5).astype(np.float64), "defined": np.ones((n, L, 1))}
    rows = np.zeros((n, W))
    for name in fields:
        rows[:, cols[name]] = block[name].reshape(n, -1)
    tensor = torch.from_numpy(rows).to(torch.float32).cuda()
    out_pass = torch.zeros((n, W), dtype=torch.float32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    et = np.dtype({"names": [k for k, _ in ExternalTarget._fields_], "formats": [(np.float64, 7), (np.float64, 7), np.float64, np.int32, np.int32],
                   "offsets": [getattr(ExternalTarget, k).offset for k, _ in ExternalTarget._fields_], "itemsize": C.sizeof(ExternalTarget)})
    col = lambda name, width: (lambda arr: arr[:, cols[name]].reshape(n, L, width))
    host_ignored = C.c_int64(0)
    kept = {}

    def foothold_pass(eng=a):
        eng.set_footholds(tensor, fields, ignored=counter)

    def host_route(eng=b):
        with torch.cuda.stream(s):
            h = tensor.cpu().numpy()
        r = np.empty((n, L), dtype=et)
        r["pose"][..., :3], r["pose"][..., 3:] = col("position", 3)(h), col("rotation", 4)(h)
        r["transform"], r["swing_clearance"] = col("transform", 7)(h), col("swing_clearance", 1)(h)[..., 0]
        r["frame_is_odom_ideal"], r["defined"] = col("frame_is_odom_ideal", 1)(h)[..., 0] != 0, col("defined", 1)(h)[..., 0] > 0
        assert eng.L.shc_engine_set_external_target(eng.h, 0, 0, n, -1, r.ctypes.data_as(C.c_void_p), C.byref(host_ignored)) == 0

    def read_back_pass(eng=a):
        eng.footholds(out_pass, fields)

    def host_read_back(eng=b):
        r = np.empty((n, L), dtype=et)
        assert eng.L.shc_engine_get_external_target(eng.h, 0, 0, n, -1, r.ctypes.data_as(C.c_void_p)) == 0
        h = np.empty((n, W), dtype=np.float32)
        col("position", 3)(h)[:], col("rotation", 4)(h)[:] = r["pose"][..., :3], r["pose"][..., 3:]
        col("transform", 7)(h)[:], col("swing_clearance", 1)(h)[..., 0] = r["transform"], r["swing_clearance"]
        col("frame_is_odom_ideal", 1)(h)[..., 0], col("defined", 1)(h)[..., 0] = r["frame_is_odom_ideal"], r["defined"]
        with torch.cuda.stream(s):
            kept["out_host"] = torch.from_numpy(h).cuda()

    # (e) the action pass on the engine and tensor of scripts/actions_bench.py
    pa = default_hexapod_params("wave")
    pa.admittance_control, pa.imu_posing = 1, 1
    pa.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    c = BatchEngine(pa, n, stream=s.cuda_stream)
    force = np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 15, (n, L))], axis=2))
    effort = rng.normal(0, 0.5, (n, L * 3))
    c.set_velocity(lin, ang), c.set_tip_force(force), c.set_joint_effort(effort)
    c.step(100)
    c.synchronize()
    acols, AW = action_columns(ACTION_FIELDS, L, 3)
    arows = np.zeros((n, AW))
    arows[:, acols["linear_xy"]], arows[:, acols["angular"]] = lin * 0.5, ang[:, None] * -1.0
    arows[:, acols["imu_orientation"]] = rng.normal(0, 0.05, (n, 4)) + np.array([1.0, 0.0, 0.0, 0.0])
    arows[:, acols["imu_angular_velocity"]] = rng.normal(0, 0.05, (n, 3))
    arows[:, acols["tip_force"]], arows[:, acols["joint_effort"]] = force.reshape(n, -1) * 0.9, effort * 0.7
    actions = torch.from_numpy(arows).to(torch.float32).cuda()
    torch.cuda.synchronize()

    def action_pass(eng=c):
        eng.set_actions(actions, ACTION_FIELDS)

    slow = max(3, iters // 20)
    routes = (("foothold_pass", foothold_pass, iters), ("host_route", host_route, slow), ("read_back_pass", read_back_pass, iters),
              ("host_read_back", host_read_back, slow), ("action_pass", action_pass, iters))
    times = {name: [] for name, _, _ in routes}
    for r in range(rounds + 1):
        for name, fn, k in routes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(k):
                fn()
            t1.record(s)
            t1.synchronize()
            if r > 0:
                times[name].append(t0.elapsed_time(t1) * 1e3 / k)
    counter.zero_()
    torch.cuda.synchronize()
    foothold_pass(), host_route()
    read_back_pass(), host_read_back()
    for e in engines:
        e.synchronize()
    torch.cuda.synchronize()
    state = [bytes(memoryview(e.get_state()).cast("B")) + bytes(e.get_aux_state()) for e in engines]
    row = {"n": n, "columns": W, "iters": {name: k for name, _, k in routes}, "rounds": rounds, "state_and_aux_bytes_equal": bool(state[0] == state[1]),
           "ignored_equal": bool(int(counter.item()) == host_ignored.value), "read_back_tensors_equal": bool(torch.equal(out_pass, kept["out_host"]))}
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    row["ratio_pass_over_host_route"] = row["foothold_pass"]["us_per_call_median"] / row["host_route"]["us_per_call_median"]
    row["ratio_read_back_pass_over_host_read_back"] = row["read_back_pass"]["us_per_call_median"] / row["host_read_back"]["us_per_call_median"]
    for e in engines + [c]:
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": "float32 [n, 102]: position, rotation, transform, swing_clearance, frame_is_odom_ideal, defined of six legs",
              "method": "per route: its iterations back to back between two HIP events on the engines' stream, the window ending in the event's "
                        "synchronise (it contains the host's share of a route); routes alternate block by block; median of the rounds after one warm-up "
                        "round; action_pass: the [n, 46] tensor and engine of scripts/actions_bench.py, for orientation",
              "expectation": "both ratios < 1 at both sizes: the host routes cross the bus twice, allocate, free and synchronise; the passes do none of it",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["state_and_aux_bytes_equal"] and r["ignored_equal"] and r["read_back_tensors_equal"] for r in result["sizes"]):
        sys.exit("the two routes left different engines or tensors")
    if not all(r["ratio_pass_over_host_route"] < 1 and r["ratio_read_back_pass_over_host_read_back"] < 1 for r in result["sizes"]):
        sys.exit("a pass is not faster than its host route")


if __name__ == "__main__":
    main()
