"""Probe: K cycles of a GPU-resident caller's loop around a mixed fleet - velocity + tip force + joint effort in for every cycle, q / qd of every
cycle out - cycle by cycle through the fleet's device I/O, and K cycles per launch through shc_fleet_step_k, next to two floors.
Fleet: 6x3 hexapods and 8x5 octopods interleaved (i % 2) on one device, config 3's parameter set, 100 cycles of walking before the timing.  The K-deep
arrays are made on the device (torch, seeded).  K = 16 at 65 536 robots; at a size where a part's 2 GiB bounds (its step_k output ring, its K-deep
staging) admit less, the largest K they admit - computed here from the parts' own sizes and recorded.
  (a) cycle by cycle: order_after(s), K x (set_inputs(row k), step(1), outputs(q[k], qd[k])), order_before(s);
  (b) step_k:         order_after(s), step_k(K, rows), step_k_joints(q, qd), order_before(s);
  (c) floor:          every part's own shc_engine_step_k on rows packed beforehand (dense, the part's order), no fleet I/O, nothing read back;
  (d) step(K):        shc_fleet_step(K), inputs held, nothing read back.
A block is --iters such groups back to back and ONE synchronise (of s for (a) and (b), of the fleet for (c) and (d)): wall clock around the block /
(iters x K) = microseconds per cycle.  The routes alternate block by block; median / min / max over --rounds rounds after one warm-up round.
outputs_equal: (a) and (b) from the same checkpointed state give the same bytes for every cycle's q and qd.  Not a test and not part of bench.py.
Usage: python scripts/fleet_step_k_bench.py [--sizes 65536 1048576] [--out profiles/bench/fleet_step_k.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = ("linear_xy", "angular", "tip_force", "joint_effort")


def largest_k(fleet, views, k_max):
    """The largest K <= k_max every part admits: K x NJ x n_slots x 16 bytes of output ring and K x rows x (3 + 3 L + L D) x 8 bytes of staging
    (velocity + tip force + joint effort), each below 2 GiB.  n_slots from the part's joint buffer: ceil(NJ / 2) planes of n_slots double2."""
    k, bounds = k_max, []
    for view in views:
        ptr, count = C.c_void_p(), C.c_int64()
        assert fleet.L.shc_engine_joint_buffer(view.h, C.byref(ptr), C.byref(count)) == 0
        n_slots = count.value // (2 * ((view.dof + 1) // 2))
        ring, stage = view.dof * n_slots * 16, view.n * (3 + 3 * view.legs + view.legs * view.dof) * 8
        bounds.append({"rows": view.n, "legs": view.legs, "dof": view.dof, "ring_bytes_per_cycle": ring, "staging_bytes_per_cycle": stage})
        k = min(k, ((1 << 31) - 1) // ring, ((1 << 31) - 1) // stage)
    return k, bounds


def measure(n, k_max, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine
    from syropod_highlevel_controller_amd.fleet import MixedFleet

    morphs = [default_hexapod_params("wave"), synthetic_octopod_params("ripple", 5, 8)]
    for p in morphs:
        p.admittance_control, p.imu_posing = 1, 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    fleet = MixedFleet(morphs, np.arange(n) % 2)
    ML, MD = fleet.max_legs, fleet.max_dof
    parts = [(BatchEngine.view(handle, fleet.params[m], len(ids)), torch.from_numpy(ids).cuda()) for handle, m, _, ids in fleet.parts()]
    K, bounds = largest_k(fleet, [v for v, _ in parts], k_max)
    gen = torch.Generator(device="cuda").manual_seed(n)
    uniform = lambda shape, lo, hi: torch.rand(shape, generator=gen, dtype=torch.float64, device="cuda") * (hi - lo) + lo
    normal = lambda shape, sd: torch.randn(shape, generator=gen, dtype=torch.float64, device="cuda") * sd
    rows = {"linear_xy": uniform((K, n, 2), -0.6, 0.6), "angular": uniform((K, n), -0.8, 0.8),
            "tip_force": torch.stack([normal((K, n, ML), 1), normal((K, n, ML), 1), uniform((K, n, ML), 0, 15)], dim=3).contiguous(),
            "joint_effort": normal((K, n, ML, MD), 2)}
    q, qd = (torch.empty((K, n, ML, MD), dtype=torch.float64, device="cuda") for _ in range(2))
    # (c)'s rows: what the K-deep pack would stage, made beforehand
    dense = [{"velocity": (rows["linear_xy"][:, ids].contiguous(), rows["angular"][:, ids].contiguous()),
              "tip_force": rows["tip_force"][:, ids, :v.legs].contiguous(), "joint_effort": rows["joint_effort"][:, ids, :v.legs, :v.dof].contiguous()}
             for v, ids in parts]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    fleet.set_inputs(**{name: rows[name][0] for name in GROUPS})
    fleet.step(100)
    fleet.synchronize()

    def cycle_by_cycle(reps=iters):
        for _ in range(reps):
            fleet.order_after(s)
            for k in range(K):
                fleet.set_inputs(**{name: rows[name][k] for name in GROUPS})
                fleet.step(1)
                fleet.outputs(q=q[k], qd=qd[k])
            fleet.order_before(s)
        s.synchronize()

    def step_k(reps=iters):
        for _ in range(reps):
            fleet.order_after(s)
            fleet.step_k(K, **rows)
            fleet.step_k_joints(q=q, qd=qd)
            fleet.order_before(s)
        s.synchronize()

    def engine_step_k():
        for _ in range(iters):
            for (view, _), d in zip(parts, dense):
                view.step_k(K, velocity=(d["velocity"][0].data_ptr(), d["velocity"][1].data_ptr()), tip_force=d["tip_force"].data_ptr(),
                            joint_effort=d["joint_effort"].data_ptr())
        fleet.synchronize()

    def step_held():
        for _ in range(iters):
            fleet.step(K)
        fleet.synchronize()

    routes = (("cycle_by_cycle", cycle_by_cycle), ("step_k", step_k), ("engine_step_k_floor", engine_step_k), ("step_held", step_held))
    times = {name: [] for name, _ in routes}
    for r in range(rounds + 1):
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) / (iters * K)
            if r > 0:
                times[name].append(dt)
    io_bytes = fleet.io_nbytes
    # (a) and (b) from the same state: every cycle's q and qd, byte for byte (NaN padding included: compared as 64-bit patterns)
    ck = fleet.checkpoint()
    fleet.synchronize()
    cycle_by_cycle(1)
    want = (q.clone(), qd.clone())
    q.zero_(), qd.zero_()
    torch.cuda.synchronize()
    fleet.restore(ck)
    fleet.synchronize()
    step_k(1)
    same = all(bool(torch.equal(x.view(torch.int64), y.view(torch.int64))) for x, y in zip(want, (q, qd)))
    ck.close()
    row = {"n": n, "hexapods": n - n // 2, "octopods": n // 2, "K": K, "K_asked": k_max, "part_bounds": bounds, "iters": iters, "rounds": rounds,
           "io_bytes": io_bytes, "outputs_equal": bool(same)}
    for name, ts in times.items():
        row[name] = {"us_per_cycle_median": statistics.median(ts) * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6}
    med = lambda name: row[name]["us_per_cycle_median"]
    row["step_k_gain_over_cycle_by_cycle_us"] = med("cycle_by_cycle") - med("step_k")
    row["cycle_by_cycle_spread_us"] = row["cycle_by_cycle"]["us_max"] - row["cycle_by_cycle"]["us_min"]
    row["gain_exceeds_spread"] = bool(row["step_k_gain_over_cycle_by_cycle_us"] > row["cycle_by_cycle_spread_us"])
    row["step_k_over_floor_us"] = med("step_k") - med("engine_step_k_floor")
    fleet.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"loop": "K cycles: velocity + tip force + joint effort in for every cycle, q / qd of every cycle out; microseconds per cycle",
              "sizes": [measure(n, args.k, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
