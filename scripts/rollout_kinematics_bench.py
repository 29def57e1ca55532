"""Probe: a K = 16 rollout of 6x3 hexapods driven by one float32 [K, n, 46] action tensor, with what a learner needs of every cycle handed
back - joints and foot tips as one float32 [K, n, 54] tensor (q 18, qd 18, model_tip 18), the joint-limit health records [K, n] and the first
cycle each robot stood on a limit - through the rollout kinematics and through the route a caller had before them, on one GPU.
Engines: config 3's parameter set, four of them (one per route), 100 cycles of walking with joint efforts live before the timing; all on one stream s.
  (a) rollout kinematics: step_k_actions(tensor) + step_k_kinematics(q, qd, model_tip) + step_k_health          - 4 kernels and the launch
  (b) today's route:      K x (set_actions(tensor[k]), step(1), observations(q, qd, model_tip) into row k of the output, scan_health into
                          device buffers)                                                                        - 4 K launches and more
  (c) bare rollout:       step_k_actions(tensor) + step_k_observations(q, qd)        - what (a) is overhead over
  (d) K bare steps:       K x (set_actions(tensor[k]), step(1))                      - what (b) is overhead over
Each route runs --iters times back to back between two HIP events on s (the window ends in the event's synchronise, behind a join of split
halves); the routes alternate block by block, medians with min - max over --rounds rounds after one warm-up round of all four.  Afterwards
the tensors of (a) and (b) must be equal, the live fields of their records, first_hit against (b)'s records, and the joints of the four engines.
The expectation, stated before the first run: (a) is not slower than (b) at either size by more than the rounds' own spread, and its cost over
(c) is less than (b)'s cost over (d).  Not a test and not part of bench.py.
Usage: python scripts/rollout_kinematics_bench.py [--sizes 65536 4096] [--out profiles/bench/rollout_kinematics.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort")
KIN = ("q", "qd", "model_tip")
K = 16
NEAR = 0.05


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import (HEALTH_NEAR_LIMIT, HEALTH_POSITION_LIMIT, HEALTH_SPEED_LIMIT, ROBOT_HEALTH_DTYPE, BatchEngine,
                                                         action_columns)

    select = HEALTH_POSITION_LIMIT | HEALTH_SPEED_LIMIT | HEALTH_NEAR_LIMIT
    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    s = torch.cuda.Stream()
    rng = np.random.default_rng(n)
    L, D = 6, 3
    lin, ang = rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n)
    force = np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 15, (n, L))], axis=2))
    effort = rng.normal(0, 0.5, (n, L * D))
    engines = [BatchEngine(p, n, stream=s.cuda_stream) for _ in range(4)]
    for e in engines:
        e.set_velocity(lin, ang)
        e.set_tip_force(force)
        e.set_joint_effort(effort)
        e.step(100)
        e.synchronize()
    a, b, c, d = engines
    cols, W = action_columns(FIELDS, L, D)
    rows = np.zeros((K, n, W), dtype=np.float32)
    for k in range(K):   # every cycle its own rows
        rows[k, :, cols["linear_xy"]], rows[k, :, cols["angular"]] = lin * (0.5 + 0.02 * k), ang[:, None] * (-1.0 + 0.05 * k)
        rows[k, :, cols["imu_orientation"]] = rng.normal(0, 0.05, (n, 4)) + np.array([1.0, 0.0, 0.0, 0.0])
        rows[k, :, cols["imu_angular_velocity"]] = rng.normal(0, 0.05, (n, 3))
        rows[k, :, cols["tip_force"]], rows[k, :, cols["joint_effort"]] = force.reshape(n, -1) * (0.9 if k % 4 else 0.0), effort * (0.7 - 0.01 * k)
    tensor = torch.from_numpy(rows).cuda()
    width = L * (2 * D + 3)
    out_a, out_b = (torch.zeros((K, n, width), dtype=torch.float32, device="cuda") for _ in range(2))
    out_c = torch.zeros((K, n, 2 * L * D), dtype=torch.float32, device="cuda")
    rec_a, rec_b = (torch.zeros((K, n, 4), dtype=torch.float64, device="cuda") for _ in range(2))
    hit_a = torch.zeros(n, dtype=torch.int32, device="cuda")
    map_b = torch.zeros((K, n), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def rollout_kinematics(eng=a):
        eng.step_k_actions(tensor, FIELDS)
        eng.step_k_kinematics(KIN, out=out_a)
        eng.step_k_health(select, NEAR, health=rec_a, first_hit=hit_a)

    def todays_route(eng=b):
        for k in range(K):
            eng.set_actions(tensor[k], FIELDS)
            eng.step(1)
            eng.observations(KIN, out=out_b[k])
            eng.scan_health(select, NEAR, out_health=rec_b[k], out_restore_map=map_b[k])

    def bare_rollout(eng=c):
        eng.step_k_actions(tensor, FIELDS)
        eng.step_k_observations(("q", "qd"), out=out_c)

    def bare_steps(eng=d):
        for k in range(K):
            eng.set_actions(tensor[k], FIELDS)
            eng.step(1)

    routes = (("rollout_kinematics", rollout_kinematics, a), ("todays_route", todays_route, b), ("bare_rollout", bare_rollout, c), ("bare_steps", bare_steps, d))
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
    for e in engines:
        e.synchronize()
    torch.cuda.synchronize()
    ha, hb = (t.cpu().numpy().view(ROBOT_HEALTH_DTYPE).reshape(K, n) for t in (rec_a, rec_b))
    records_equal = bool(all(ha[f].tobytes() == hb[f].tobytes() for f in ("min_limit_proximity", "max_speed_ratio")) and
                         np.array_equal(ha["leg_masks"] & 0x00ffff00, hb["leg_masks"] & 0x00ffff00) and np.array_equal(ha["flags"] & select, hb["flags"] & select))
    selected = (hb["flags"] & select) != 0
    first_hit_equal = bool(np.array_equal(hit_a.cpu().numpy(), np.where(selected.any(axis=0), selected.argmax(axis=0), -1)))
    joints = [e.joints()[0].tobytes() for e in engines]
    row = {"n": n, "K": K, "iters": iters, "rounds": rounds, "tensors_equal": bool(torch.equal(out_a, out_b)), "records_equal": records_equal,
           "first_hit_equal": first_hit_equal, "robots_selected": int(selected.any(axis=0).sum()), "joints_equal": bool(len(set(joints)) == 1),
           "engine_calls_per_rollout": {"rollout_kinematics": 3, "todays_route": 4 * K, "bare_rollout": 2, "bare_steps": 2 * K}}
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    med = {name: row[name]["us_per_call_median"] for name in times}
    spread = max(row[name]["us_max"] - row[name]["us_min"] for name in ("rollout_kinematics", "todays_route"))
    row["cost_over_bare_us"] = {"rollout_kinematics": med["rollout_kinematics"] - med["bare_rollout"], "todays_route": med["todays_route"] - med["bare_steps"]}
    row["ratio_kinematics_over_today"] = med["rollout_kinematics"] / med["todays_route"]
    row["cycles_per_s"] = {name: K * n / (med[name] * 1e-6) for name in times}
    row["expectation_met"] = bool(med["rollout_kinematics"] <= med["todays_route"] + spread and
                                  row["cost_over_bare_us"]["rollout_kinematics"] < row["cost_over_bare_us"]["todays_route"])
    for e in engines:
        e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": f"float32 [{K}, n, 46]: " + ", ".join(FIELDS), "kinematics": f"float32 [{K}, n, 54]: " + ", ".join(KIN),
              "health": f"records [{K}, n] and first_hit [n], select POSITION_LIMIT | SPEED_LIMIT | NEAR_LIMIT, near_limit_proximity {NEAR}",
              "expectation": "rollout_kinematics is not slower than todays_route at either size by more than the rounds' own spread, and its cost over "
                             "bare_rollout is less than todays_route's cost over bare_steps",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not all(r["tensors_equal"] and r["records_equal"] and r["first_hit_equal"] and r["joints_equal"] for r in result["sizes"]):
        sys.exit("the routes left different outputs or engines")


if __name__ == "__main__":
    main()
