"""Probe: the device checkpoint (shc_engine_checkpoint_update) and the indexed restore (shc_engine_restore_instances) against a plain plane copy of
the same byte count and against the host route (get_state / get_aux_state -> set_state / set_aux_state).
Hexapods with config 3's parameter set (wave gait, admittance, IMU posing) after 200 cycles, 4 096 and 65 536 instances.  Per size:
  (a) capture, full restore (NULL map), a random 10 % reset and a one-to-all clone (device maps), each timed with events on the engine's stream: median of
      --calls calls after --warmup warm-up calls;
  (b) shc_debug_plane_copy over the checkpoint's byte count in this process: the wall-clock difference between a long and a short run of repetitions
      (the two allocations and the memset of each run cancel), per repetition;
  (c) the host route over --host-instances instances (read the four records, write them back), scaled linearly to n (an extrapolation: the route
      moves a fixed record per instance through one temporary buffer and one synchronisation per call).
Not a test and not part of bench.py.  Usage: python scripts/checkpoint_bench.py [--out profiles/bench/checkpoint_restore.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-instances", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params, engine
    from syropod_highlevel_controller_amd.engine import BatchEngine

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    L, NJ = 6, 3
    lib = engine.lib()
    cls = lib.shc_debug_checkpoint_field_class
    leg_fields = next(f for f in range(1, 1000) if cls(NJ, 0, f) < 0)
    rob_fields = next(f for f in range(1, 1000) if cls(NJ, 1, f) < 0)
    leg_copied = sum(cls(NJ, 0, f) in (0, 2) for f in range(leg_fields)) - 4   # (the POSER_TIP planes move only while they are state)
    rob_copied = sum(cls(NJ, 1, f) in (0, 2) for f in range(rob_fields))
    result = {"calls": args.calls, "warmup": args.warmup, "sizes": {}}
    stream = torch.cuda.Stream()
    for n in args.sizes:
        rng = np.random.default_rng(n)
        eng = BatchEngine(p, n, stream=stream.cuda_stream)
        eng.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
        eng.set_tip_force(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 2, (n, L))], axis=2))
        eng.step(200)
        eng.synchronize()
        ck = eng.checkpoint()
        with torch.cuda.stream(stream):
            ident = torch.arange(n, dtype=torch.int64, device="cuda")
            reset = torch.where(torch.from_numpy(rng.random(n) < 0.1).cuda(), ident, torch.full_like(ident, -1)).contiguous()
            clone = torch.full_like(ident, n // 3)
        stream.synchronize()

        def timed(fn):
            times = []
            for k in range(args.warmup + args.calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                if k >= args.warmup:
                    times.append(a.elapsed_time(b) * 1e-3)
            return {"us_median": statistics.median(times) * 1e6, "us_min": min(times) * 1e6, "us_max": max(times) * 1e6}

        held = ck.nbytes
        per_robot = L * (leg_copied * 8 + 4) + rob_copied * 8 + 16   # bytes a restored robot reads, and writes
        n_reset = int((reset >= 0).sum().item())
        calls = {"capture": (ck.update, 2 * held, n), "restore_all": (lambda: eng.restore(ck), 2 * n * per_robot, n),
                 "reset_10_percent": (lambda: eng.restore(ck, reset), 2 * n_reset * per_robot + 8 * n, n_reset),
                 "clone_one_to_all": (lambda: eng.restore(ck, clone), 2 * n * per_robot + 8 * n, n)}
        doubles = (held // 16) * 2
        short, long_ = 5, 45
        lib.shc_debug_plane_copy(0, doubles, 2)
        t0 = time.perf_counter()
        lib.shc_debug_plane_copy(0, doubles, short)
        t1 = time.perf_counter()
        lib.shc_debug_plane_copy(0, doubles, long_)
        t2 = time.perf_counter()
        t_copy = ((t2 - t1) - (t1 - t0)) / (long_ - short)
        copy_rate = 2 * 8 * doubles / t_copy
        row = {"checkpoint_bytes": held, "plane_copy_us": t_copy * 1e6, "plane_copy_GBps": copy_rate / 1e9}
        m = min(args.host_instances, n)
        t0 = time.perf_counter()
        state, aux = eng.get_state(0, m), eng.get_aux_state(0, m)
        eng.set_state(state, 0)
        eng.set_aux_state(aux, 0)
        t_host = (time.perf_counter() - t0) / m
        row["host_route_us_per_instance"] = t_host * 1e6
        row["host_route_instances_timed"] = m
        row["host_route_extrapolated_ms"] = t_host * n * 1e3
        for name, (fn, moved, robots) in calls.items():
            r = timed(fn)
            t = r["us_median"] * 1e-6
            r.update({"bytes_moved": moved, "GBps": moved / t / 1e9, "fraction_of_plane_copy_rate": moved / t / copy_rate,
                      "instances": robots, "speedup_over_host_route_extrapolated": t_host * robots / t})
            row[name] = r
        result["sizes"][str(n)] = row
        ck.close()
        eng.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
