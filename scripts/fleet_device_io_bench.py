"""Probe: one iteration of a GPU-resident caller's loop around a mixed fleet - velocity + tip force + joint effort in, one step, q / qd out -
through the host forms and through the device forms, next to the bare step.
Fleet: 6x3 hexapods and 8x5 octopods interleaved (i % 2) on one device, config 3's parameter set, 100 cycles of walking before the timing.
  (a) device route: shc_fleet_order_after_stream(s), shc_fleet_set_inputs_device, shc_fleet_step(1), shc_fleet_get_outputs_device(q, qd),
      shc_fleet_order_stream_after(s), --iters times back to back, then ONE synchronise of s: wall clock around the block / --iters;
  (b) host route: shc_fleet_set_velocity, _set_tip_force, _set_joint_effort from host arrays, shc_fleet_step(1), shc_fleet_get_joint_state into host
      arrays (every one of them synchronises): wall clock around --host-iters iterations / --host-iters;
  (c) the step alone: shc_fleet_step(1) --iters times, then shc_fleet_synchronize: wall clock / --iters.
(a), (b) and (c) alternate block by block; medians over --rounds rounds after one warm-up round.  The record shows each route's overhead over the
bare step.  Not a test and not part of bench.py.
Usage: python scripts/fleet_device_io_bench.py [--sizes 65536 1048576] [--out profiles/bench/fleet_device_io.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(n, iters, host_iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
    from syropod_highlevel_controller_amd.fleet import MixedFleet

    morphs = [default_hexapod_params("wave"), synthetic_octopod_params("ripple", 5, 8)]
    for p in morphs:
        p.admittance_control, p.imu_posing = 1, 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    rng = np.random.default_rng(n)
    fleet = MixedFleet(morphs, np.arange(n) % 2)
    ML, MD = fleet.max_legs, fleet.max_dof
    host = {"linear_xy": rng.uniform(-0.6, 0.6, (n, 2)), "angular": rng.uniform(-0.8, 0.8, n),
            "tip_force": np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, ML)), rng.normal(0, 1, (n, ML)), rng.uniform(0, 15, (n, ML))], axis=2)),
            "joint_effort": rng.normal(0, 2, (n, ML, MD))}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    q, qd = (torch.empty((n, ML, MD), dtype=torch.float64, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    fleet.set_velocity(host["linear_xy"], host["angular"])
    fleet.set_tip_force(host["tip_force"])
    fleet.set_joint_effort(host["joint_effort"])
    fleet.step(100)
    fleet.synchronize()

    def device_route():
        for _ in range(iters):
            fleet.order_after(s)
            fleet.set_inputs(**dev)
            fleet.step(1)
            fleet.outputs(q=q, qd=qd)
            fleet.order_before(s)
        s.synchronize()
        return iters

    def host_route():
        for _ in range(host_iters):
            fleet.set_velocity(host["linear_xy"], host["angular"])
            fleet.set_tip_force(host["tip_force"])
            fleet.set_joint_effort(host["joint_effort"])
            fleet.step(1)
            fleet.joints()
        return host_iters

    def step_alone():
        for _ in range(iters):
            fleet.step(1)
        fleet.synchronize()
        return iters

    routes = (("device_route", device_route), ("host_route", host_route), ("step_alone", step_alone))
    times = {name: [] for name, _ in routes}
    for r in range(rounds + 1):
        for name, fn in routes:
            t0 = time.perf_counter()
            k = fn()
            dt = (time.perf_counter() - t0) / k
            if r > 0:
                times[name].append(dt)
    # the two routes end in the same joints (the device route's last q against the host getter's, on the same fleet and state)
    fleet.outputs(q=q, qd=qd)
    fleet.synchronize()
    wq, wqd = fleet.joints()
    same = q.cpu().numpy().tobytes() == wq.tobytes() and qd.cpu().numpy().tobytes() == wqd.tobytes()
    row = {"n": n, "hexapods": n - n // 2, "octopods": n // 2, "iters": iters, "host_iters": host_iters, "rounds": rounds, "io_bytes": fleet.io_nbytes,
           "outputs_equal": bool(same)}
    for name, ts in times.items():
        row[name] = {"us_per_iteration_median": statistics.median(ts) * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6}
    step = row["step_alone"]["us_per_iteration_median"]
    row["device_overhead_over_step_us"] = row["device_route"]["us_per_iteration_median"] - step
    row["host_overhead_over_step_us"] = row["host_route"]["us_per_iteration_median"] - step
    fleet.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1 << 20])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"loop": "velocity + tip force + joint effort in, one step, q / qd out", "sizes": [measure(n, args.iters, args.host_iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
