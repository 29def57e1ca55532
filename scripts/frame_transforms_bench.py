"""Probe: one shc_engine_get_frame_transforms call (legs + body records, SHC_FRAME_BASE_LINK) into device buffers against the host route it
replaces (joints() read-back + a DH chain per leg per robot in numpy, tests/frames_numpy.py).  4 096 and 65 536 hexapods, 65 536 8 x 5
octopods, after 100 cycles of walking.
  (a) the batched call, timed with events on the engine's stream: median of --calls calls after --warmup warm-up calls;
  (b) shc_debug_plane_copy of the same number of bytes as the call writes, in this process (the difference of two repetition counts, so
      that its allocations drop out), and the ratio copy time / call time;
  (c) the figure scripts/leg_state_msgs_bench.py reports, for comparison with the LegState pass: bytes moved (planes read + records
      written) per second over the rate of a 256 MiB plane copy (past the Infinity Cache);
  (d) the host route over --host-robots robots, scaled linearly to n (an extrapolation: the numpy chain is per robot).
Usage: python scripts/frame_transforms_bench.py [--out profiles/bench/frame_transforms.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def copy_seconds(lib, n_doubles, reps):
    t0 = time.perf_counter()
    lib.shc_debug_plane_copy(0, n_doubles, reps)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-robots", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import frames_numpy as fn
    from syropod_highlevel_controller_amd import default_hexapod_params, engine, synthetic_octopod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine

    lib = engine.lib()
    copy_doubles = 1 << 25   # 256 MiB read + 256 MiB written per repetition
    copy_seconds(lib, copy_doubles, 2)
    big = (copy_seconds(lib, copy_doubles, 22) - copy_seconds(lib, copy_doubles, 2)) / 20
    copy_rate = 2 * 8 * copy_doubles / big
    result = {"plane_copy_GBps": copy_rate / 1e9, "cases": {}}
    stream = torch.cuda.Stream()
    cases = [("hexapod_6x3", default_hexapod_params("ripple"), 4096), ("hexapod_6x3", default_hexapod_params("ripple"), 65536),
             ("octopod_8x5", synthetic_octopod_params("ripple", 5, 8), 65536)]
    for name, p, n in cases:
        L, NJ = p.leg_count, max(p.leg_dof[l] for l in range(p.leg_count))
        rng = np.random.default_rng(n)
        eng = BatchEngine(p, n, stream=stream.cuda_stream)
        eng.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
        eng.step(100)
        eng.synchronize()
        lbuf = torch.empty(n * L * 42, dtype=torch.float64, device="cuda")
        bbuf = torch.empty(n * 20, dtype=torch.float64, device="cuda")
        times = []
        for k in range(args.warmup + args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.frame_transforms(out_legs=lbuf.data_ptr(), out_body=bbuf.data_ptr())
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b) * 1e-3)
        t_call = statistics.median(times)
        written = n * (L * 336 + 160)
        read = n * (L * 16 * ((NJ + 2) // 2) + 14 * 8)   # the joint-angle planes (16 B each) + current pose, odometry, velocity
        same = 2 * ((written // 8 + 1) // 2)
        copy_seconds(lib, same, 4)
        reps = 200 if n <= 4096 else 40
        t_copy = (copy_seconds(lib, same, 4 + reps) - copy_seconds(lib, same, 4)) / reps
        m = min(args.host_robots, n)
        t0 = time.perf_counter()
        q = eng.joints()[0]
        t_readback = time.perf_counter() - t0
        t0 = time.perf_counter()
        fn.robot_frames(p, q[:m])
        t_chain = (time.perf_counter() - t0) / m
        result["cases"][f"{name}_{n}"] = {
            "instances": n, "legs": L, "dof": NJ, "frames_per_call": n * (L * (NJ + 1) + 2),
            "batched_call_us_median": t_call * 1e6, "batched_call_us_min": min(times) * 1e6, "batched_call_us_max": max(times) * 1e6,
            "bytes_written": written, "bytes_read": read, "same_bytes_plane_copy_us": t_copy * 1e6, "plane_copy_time_over_call_time": t_copy / t_call,
            "GBps_moved": (written + read) / t_call / 1e9, "fraction_of_plane_copy_rate": (written + read) / t_call / copy_rate,
            "host_joint_readback_ms": t_readback * 1e3, "host_numpy_chain_us_per_robot": t_chain * 1e6, "host_robots_timed": m,
            "host_route_extrapolated_ms": (t_readback + t_chain * n) * 1e3, "speedup_over_host_route": (t_readback + t_chain * n) / t_call}
        eng.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
