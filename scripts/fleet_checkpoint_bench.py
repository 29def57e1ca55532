"""Probe: "reset the robots that fell over" for a mixed fleet, the new call against the route a caller had before it.
Fleet: 6x3 hexapods and 8x5 octopods interleaved (i % 2) on one device, config 3's parameter set, 200 cycles of walking, then a checkpoint.
A chosen fraction of the robots (1 %, 10 %, 100 %) is made unhealthy by an injected IK-deviation flag (set_state on the parts, before the timing) -
the flag is state, so a reset clears it; every timed call is therefore preceded by an untimed call that plants the flags again.  Per fraction:
  (a) shc_fleet_scan_and_restore with both outputs NULL, then shc_fleet_synchronize (the call itself does not wait): wall clock around the pair;
  (b) the host route: shc_fleet_scan_health, then per part set_state / set_aux_state of the selected robots' rows from HOST copies read with
      get_state / get_aux_state at capture time, one call per run of consecutive selected robots (what tests/test_gpu_checkpoint.py's
      host_restore does), then shc_fleet_synchronize: wall clock around all of it.
(a) and (b) alternate call by call; medians over --calls calls after --warmup warm-up calls of each.  Not a test and not part of bench.py.
Usage: python scripts/fleet_checkpoint_bench.py [--n 8192] [--out profiles/bench/fleet_checkpoint.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.01, 0.1, 1.0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
    from syropod_highlevel_controller_amd.engine import HEALTH_IK_DEVIATION, BatchEngine, HealthCriteria, _check
    from syropod_highlevel_controller_amd.fleet import MixedFleet
    from syropod_highlevel_controller_amd.params import InstanceState

    morphs = [default_hexapod_params("wave"), synthetic_octopod_params("ripple", 5, 8)]
    for p in morphs:
        p.admittance_control, p.imu_posing = 1, 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    n = args.n
    rng = np.random.default_rng(n)
    fleet = MixedFleet(morphs, np.arange(n) % 2)
    L = fleet.L
    fleet.set_velocity(rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n))
    fleet.step(200)
    fleet.synchronize()
    ck = fleet.checkpoint()
    parts = [(BatchEngine.view(h, fleet.params[m], len(ids)), ids) for h, m, _, ids in fleet.parts()]
    held = [(v.get_state(), v.get_aux_state()) for v, _ in parts]   # the host copies route (b) restores from
    crit = HealthCriteria(HEALTH_IK_DEVIATION, 0, 0.0, 0.0)
    result = {"n": n, "hexapods": int(len(parts[0][1])), "octopods": int(len(parts[1][1])), "calls": args.calls, "warmup": args.warmup,
              "checkpoint_bytes": ck.nbytes, "fractions": {}}

    def plant(chosen):
        """Raise the IK-deviation flag of the chosen robots (leg 0) through set_state on their parts; untimed."""
        for v, ids in parts:
            states = v.get_state()
            s = np.frombuffer(states, dtype=np.dtype(InstanceState))
            s["leg"]["ik_failed"][:, 0] = chosen[ids]
            v.set_state(states)
        fleet.synchronize()

    def device_route():
        _check(L.shc_fleet_scan_and_restore(fleet.h, ck.h, C.byref(crit), None, None), "shc_fleet_scan_and_restore")
        fleet.synchronize()

    def host_route():
        health = fleet.scan_health(select=HEALTH_IK_DEVIATION)
        sick = (health["flags"] & HEALTH_IK_DEVIATION) != 0
        for (v, ids), (states, aux) in zip(parts, held):
            per = len(aux) // len(ids)
            sel = np.flatnonzero(sick[ids])
            if len(sel) == 0:
                continue
            for run in np.split(sel, np.flatnonzero(np.diff(sel) != 1) + 1):   # one call per run of consecutive rows
                lo, hi = int(run[0]), int(run[-1]) + 1
                v.set_state((InstanceState * (hi - lo)).from_buffer(states, lo * C.sizeof(InstanceState)), first=lo)
                v.set_aux_state(aux[lo * per:hi * per], first=lo)
        fleet.synchronize()

    for frac in args.fractions:
        chosen = np.zeros(n, dtype=np.int32)
        chosen[rng.permutation(n)[:max(1, int(round(frac * n)))]] = 1
        # how many the scan really selects (a walking robot may carry the bit of its own accord): counted once, with the outputs asked for
        plant(chosen)
        selected = int(((fleet.scan_health(select=HEALTH_IK_DEVIATION)["flags"] & HEALTH_IK_DEVIATION) != 0).sum())
        times = {"scan_and_restore": [], "host_route": []}
        for k in range(args.warmup + args.calls):
            for name, fn in (("scan_and_restore", device_route), ("host_route", host_route)):
                plant(chosen)
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if k >= args.warmup:
                    times[name].append(dt)
        row = {"planted": int(chosen.sum()), "selected": selected}
        for name, ts in times.items():
            row[name] = {"us_median": statistics.median(ts) * 1e6, "us_min": min(ts) * 1e6, "us_max": max(ts) * 1e6}
        row["host_over_device"] = row["host_route"]["us_median"] / row["scan_and_restore"]["us_median"]
        row["device_not_slower"] = bool(row["scan_and_restore"]["us_median"] <= row["host_route"]["us_median"])
        result["fractions"][str(frac)] = row
    ck.close()
    fleet.close()
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
