"""Probe: what every LegStepper of 6x3 hexapods is doing with its target - the control nodes of its three Bezier curves, stride vector, swing
clearance and the tip path of the next H = 12 cycles - as one float32 [n, 522] tensor (6 legs x (3 x 15 + 3 + 3 + 36)), through the step plan
pass and through the only route to these numbers that exists without it, on one GPU.
Engines: config 3's parameter set, one engine on one stream s, 150 cycles of walking before the timing, every fourth robot never commanded.
  (a) step plan pass:  step_plan(nodes, stride, clearance, path; H = 12) into a device tensor                 - 1 launch, no host wait
  (b) today's route:   shc_engine_get_state to the host (4.7 KB per robot, with a stream synchronisation), then the node formulas
                       restated in the caller's code - here tests/plan_numpy.py, vectorised numpy - as a float32 host array
      (b) ends on the host; a planner on the GPU would add the copy back, which is not charged.
(a) runs --iters times back to back, (b) once, between two HIP events on s; the routes alternate, medians with min - max over --rounds rounds
after one warm-up round of both.  Afterwards the outputs are compared - pad in the same places, values within 1e-6 (float32 against float64) -
and the engine against its bytes before the first call.
The route comparison is the record: no ratio is fixed in advance, nobody has measured either side.  Not a test and not part of bench.py.
Usage: python scripts/step_plan_bench.py [--sizes 65536 4096] [--out profiles/bench/step_plan.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("swing_1_nodes", "swing_2_nodes", "stance_nodes", "stride_vector", "swing_clearance", "path")
HORIZON = 12


def measure(n, iters, rounds):
    import torch
    import plan_numpy
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import BatchEngine, plan_columns

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    s = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n)
    lin[::4], ang[::4] = 0.0, 0.0
    eng = BatchEngine(p, n, stream=s.cuda_stream)
    eng.set_velocity(lin, ang)
    eng.step(150)
    eng.synchronize()
    tables = eng.tables()
    _, D = plan_columns(FIELDS, 6, HORIZON)
    out_a = torch.zeros((n, D), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = bytes(memoryview(eng.get_state()).cast("B")), bytes(eng.get_aux_state())
    host = {}

    def step_plan_pass():
        eng.step_plan(FIELDS, HORIZON, out=out_a)

    def todays_route():
        host["rows"] = plan_numpy.rows(eng.get_state(), p, tables, FIELDS, 6, HORIZON).astype(np.float32)

    routes = (("step_plan_pass", step_plan_pass, iters), ("todays_route", todays_route, 1))
    times = {name: [] for name, _, _ in routes}
    for r in range(rounds + 1):
        for name, fn, reps in routes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(reps):
                fn()
            eng.join()   # (a large batch launches on the engine's two half streams: s follows them - events, no host wait - before the window closes)
            t1.record(s)
            t1.synchronize()
            if r > 0:
                times[name].append(t0.elapsed_time(t1) * 1e3 / reps)
        print(f"n = {n}: round {r} of {rounds} done", file=sys.stderr, flush=True)
    eng.synchronize()
    torch.cuda.synchronize()
    got, want = out_a.cpu().numpy(), host["rows"]
    same_pad = bool((np.isnan(got) == np.isnan(want)).all())
    finite = np.isfinite(want) & np.isfinite(got)
    row = {"n": n, "columns": D, "horizon": HORIZON, "iters": iters, "rounds": rounds, "pad_in_the_same_places": same_pad,
           "max_abs_diff": float(np.abs(got[finite].astype(np.float64) - want[finite].astype(np.float64)).max()),
           "pad_fraction": float(np.isnan(want).mean()),
           "engine_untouched": bool((bytes(memoryview(eng.get_state()).cast("B")), bytes(eng.get_aux_state())) == before),
           "state_bytes_per_robot": len(before[0]) // n}
    row["outputs_agree"] = bool(same_pad and row["max_abs_diff"] <= 1e-6)
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    row["ratio_pass_over_today"] = row["step_plan_pass"]["us_per_call_median"] / row["todays_route"]["us_per_call_median"]
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"result": "float32 [n, 522]: " + ", ".join(FIELDS) + f", H = {HORIZON}",
              "routes": {"step_plan_pass": "shc_engine_get_step_plan into a device tensor, 1 launch",
                         "todays_route": "shc_engine_get_state to the host + tests/plan_numpy.py, result on the host"},
              "expectation": "none fixed in advance: the route comparison is the record",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    if args.out and os.path.exists(args.out):   # the compiler's register report kept in the record is not this script's to measure: carried over
        with open(args.out) as f:
            kept = json.load(f).get("registers")
        if kept is not None:
            result["registers"] = kept
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["outputs_agree"] and r["engine_untouched"] for r in result["sizes"]):
        sys.exit("the routes left different outputs, or the pass wrote into its engine")


if __name__ == "__main__":
    main()
