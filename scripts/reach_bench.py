"""Probe: which of C = 8 candidate tip targets per robot every leg of 6x3 hexapods can reach, by the IK line search of S = 16 steps, as one
float32 [n, 8, 30] tensor (fraction 6, limit proximity 6, tip 18 per candidate) - through the reach probe and through the route a caller had
before it, on one GPU.
Engines: config 3's parameter set, two of them (one per route), 100 cycles of walking before the timing; both on one stream s.  Targets: the
present tip + r u, u a unit vector and r uniform in 1 .. 25 cm, so that legs arrive, stop on the way and fail at once.
  (a) reach probe:    probe_reach(targets [n, 8, 6, 3] float32)                                                      - 1 launch
  (b) today's route:  per candidate a checkpoint restore, then S x (shc_leg_set_desired_tip_pose + shc_leg_apply_ik(simulation = 1), every
                      leg, device arrays), then shc_leg_apply_fk                                                     - (2 S + 2) C = 272 launches
      (b) is given its S x C desired tip poses ready-made on the device (a caller would compute them too), keeps every step's result, and
      ends with its engine restored; it overwrites the joints, the desired tip and the tip-force estimate on the way, and it takes every
      step of a leg that has stopped.
Each route runs --iters times back to back between two HIP events on s (the window ends in the event's synchronise, behind a join of split
halves); the routes alternate block by block, medians with min - max over --rounds rounds after one warm-up round of both.  Afterwards the
outputs are compared: the fractions exactly (from (b)'s per-step results), limit proximity and - for the legs that took every step, where
(b)'s one FK at the end measures the same tip - the tips within 1e-6 (float32 against float64), and the engine of (a) against its bytes
before the first call.
The expectation, stated before the first run: at both sizes (a) is not slower than (b) by more than the rounds' own min - max spread.  Not a
test and not part of bench.py.
Usage: python scripts/reach_bench.py [--sizes 65536 4096] [--out profiles/bench/reach.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("fraction", "limit_proximity", "tip")
CANDIDATES, STEPS = 8, 16


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine, reach_columns

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    s = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    L = 6
    lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n)
    a, b = (BatchEngine(p, n, stream=s.cuda_stream) for _ in range(2))
    for e in (a, b):
        e.set_velocity(lin, ang)
        e.step(100)
        e.synchronize()
    origin = a.leg_apply_fk()[:, :3].reshape(n, 1, L, 3)
    b.leg_apply_fk()
    u = rng.normal(size=(n, CANDIDATES, L, 3))
    u /= np.linalg.norm(u, axis=3, keepdims=True)
    targets32 = (origin + u * rng.uniform(0.01, 0.25, (n, CANDIDATES, L, 1))).astype(np.float32)
    targets = torch.from_numpy(targets32).cuda()
    cols, D = reach_columns(FIELDS, L, 3)
    out_a = torch.zeros((n, CANDIDATES, D), dtype=torch.float32, device="cuda")
    # route (b)'s inputs and outputs: desired poses [C][S][n L][7] (rotation undefined: zeros), results [C][S][n L], tips [C][n L][7]
    o64, t64 = torch.from_numpy(origin.reshape(n * L, 3)).cuda(), targets.double().permute(1, 0, 2, 3).reshape(CANDIDATES, n * L, 3)
    poses = torch.zeros((CANDIDATES, STEPS, n * L, 7), dtype=torch.float64, device="cuda")
    for k in range(STEPS):
        w = float(k + 1) / STEPS
        poses[:, k, :, :3] = o64 * (1.0 - w) + t64 * w
    results = torch.zeros((CANDIDATES, STEPS, n * L), dtype=torch.float64, device="cuda")
    tips = torch.zeros((CANDIDATES, n * L, 7), dtype=torch.float64, device="cuda")
    ck = b.checkpoint()
    torch.cuda.synchronize()
    before = bytes(memoryview(a.get_state()).cast("B")), bytes(a.get_aux_state())
    lib = b.L
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def reach_probe():
        a.probe_reach(targets, STEPS, FIELDS, out=out_a)

    def todays_route():
        for c in range(CANDIDATES):
            b.restore(ck)
            for k in range(STEPS):
                if lib.shc_leg_set_desired_tip_pose(b.h, 0, n, -1, ptr(poses[c, k]), 0, 1) or lib.shc_leg_apply_ik(b.h, 0, n, -1, 1, ptr(results[c, k]), 1):
                    sys.exit("a per-leg call failed")
            if lib.shc_leg_apply_fk(b.h, 0, n, -1, None, ptr(tips[c]), 1):
                sys.exit("a per-leg call failed")

    routes = (("reach_probe", reach_probe, a), ("todays_route", todays_route, b))
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
    b.restore(ck)
    for e in (a, b):
        e.synchronize()
    torch.cuda.synchronize()
    got = out_a.cpu().numpy()
    res = results.cpu().numpy().reshape(CANDIDATES, STEPS, n, L)
    done = np.cumprod(res != 0.0, axis=1).sum(axis=1)                                   # leading non-zero steps: (C, n, L)
    last = np.take_along_axis(res, np.minimum(done, STEPS - 1)[:, None], axis=1)[:, 0]  # the step it stopped at, or the last one
    fraction = got[:, :, cols["fraction"]].transpose(1, 0, 2)
    proximity = got[:, :, cols["limit_proximity"]].transpose(1, 0, 2)
    tip = got[:, :, cols["tip"]].reshape(n, CANDIDATES, L, 3).transpose(1, 0, 2, 3)
    full = done == STEPS
    tip_b = tips.cpu().numpy()[:, :, :3].reshape(CANDIDATES, n, L, 3)
    row = {"n": n, "candidates": CANDIDATES, "steps": STEPS, "iters": iters, "rounds": rounds,
           "fractions_equal": bool(np.array_equal(fraction, (done / float(STEPS)).astype(np.float32))),
           "limit_proximity_max_abs_diff": float(np.abs(proximity - last).max()),
           "tip_max_abs_diff_full_legs": float(np.abs(tip - tip_b)[full].max()) if full.any() else 0.0,
           "legs_full_partial_zero": [int(full.sum()), int(((done > 0) & ~full).sum()), int((done == 0).sum())],
           "engine_untouched": bool((bytes(memoryview(a.get_state()).cast("B")), bytes(a.get_aux_state())) == before),
           "launches_per_call": {"reach_probe": 1, "todays_route": (2 * STEPS + 2) * CANDIDATES}}
    row["outputs_agree"] = bool(row["fractions_equal"] and row["limit_proximity_max_abs_diff"] <= 1e-6 and row["tip_max_abs_diff_full_legs"] <= 1e-6)
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    med = {name: row[name]["us_per_call_median"] for name in times}
    spread = max(row[name]["us_max"] - row[name]["us_min"] for name in times)
    row["ratio_probe_over_today"] = med["reach_probe"] / med["todays_route"]
    row["leg_candidates_per_s"] = {name: n * L * CANDIDATES / (med[name] * 1e-6) for name in times}
    row["expectation_met"] = bool(med["reach_probe"] <= med["todays_route"] + spread)
    ck.close()
    for e in (a, b):
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"targets": f"float32 [n, {CANDIDATES}, 6, 3]", "result": f"float32 [n, {CANDIDATES}, 30]: " + ", ".join(FIELDS), "steps": STEPS,
              "expectation": "reach_probe is not slower than todays_route at either size by more than the rounds' own min - max spread",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["outputs_agree"] and r["engine_untouched"] for r in result["sizes"]):
        sys.exit("the routes left different outputs, or the probe wrote into its engine")


if __name__ == "__main__":
    main()
