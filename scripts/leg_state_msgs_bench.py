"""Probe: one shc_engine_get_leg_state_msgs call into a device buffer against the per-instance route (shc_engine_read_leg_state_msg in a loop).
Hexapods with config 3's parameter set (wave gait, admittance, IMU posing) after 200 cycles, 4 096 and 65 536 instances.
  (a) the batched call, timed with events on the engine's stream: median of --calls calls after --warmup warm-up calls;
  (b) the bytes it must move (state planes read + n x legs x 512 B written) over (a), as a fraction of the plane-copy rate that
      shc_debug_plane_copy reaches in this process;
  (c) the per-instance route over --per-instance instances, scaled linearly to n (an extrapolation: each call is independent and
      synchronous - its own derive pass over the batch, the batched pass with count = 1, copy and stream synchronisation - so n calls cost n times one).
Usage: python scripts/leg_state_msgs_bench.py [--out profiles/bench/leg_state_msgs.json]"""
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
    ap.add_argument("--per-instance", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params, engine
    from syropod_highlevel_controller_amd.engine import BatchEngine

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    L, NJ = 6, 3
    # planes the kernel reads per leg slot (16 B each): Q / QD / TIP, TARG, POSER_TIP, MODEL_TIP, TF, ADM_DELTA, EFFORT_IN, MEAS_Q; + the leg word
    planes_read = (2 * NJ + 3 + 1) // 2 + 7 * 2
    lib = engine.lib()
    copy_doubles, copy_reps = 1 << 25, 20   # 256 MiB read + 256 MiB written per repetition: past the Infinity Cache
    lib.shc_debug_plane_copy(0, copy_doubles, 2)
    t0 = time.perf_counter()
    lib.shc_debug_plane_copy(0, copy_doubles, copy_reps)
    copy_rate = 2 * 8 * copy_doubles * copy_reps / (time.perf_counter() - t0)   # (includes two allocations and a memset: a lower bound)
    result = {"plane_copy_GBps": copy_rate / 1e9, "sizes": {}}
    stream = torch.cuda.Stream()
    for n in args.sizes:
        rng = np.random.default_rng(n)
        eng = BatchEngine(p, n, stream=stream.cuda_stream)
        eng.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
        eng.set_tip_force(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 2, (n, L))], axis=2))
        eng.step(200)
        eng.synchronize()
        buf = torch.empty(n * L * 64, dtype=torch.float64, device="cuda")
        times = []
        for k in range(args.warmup + args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.leg_state_msgs(out=buf.data_ptr())
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b) * 1e-3)
        t_call = statistics.median(times)
        moved = n * L * (planes_read * 16 + 4 + 512)
        m = min(args.per_instance, n)
        t0 = time.perf_counter()
        for i in range(m):
            eng.leg_state_msg(i * (n // m))
        t_one = (time.perf_counter() - t0) / m
        result["sizes"][str(n)] = {
            "batched_call_us_median": t_call * 1e6, "batched_call_us_min": min(times) * 1e6, "batched_call_us_max": max(times) * 1e6,
            "bytes_moved": moved, "GBps": moved / t_call / 1e9, "fraction_of_plane_copy": moved / t_call / copy_rate,
            "per_instance_call_us": t_one * 1e6, "per_instance_instances_timed": m,
            "per_instance_route_extrapolated_ms": t_one * n * 1e3, "speedup_over_per_instance_route": t_one * n / t_call}
        eng.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
