"""Probe: a learner-sized observation tensor of a fleet - q, qd, model tip, stance / swing progress, body pose, desired velocity of every robot
as one float32 [n, D] device tensor - through the observation pass and through the record route, on one GPU.
Fleet: 6x3 hexapods with config 3's parameter set (one part), 100 cycles of walking before the timing.
  (a) observation pass: shc_fleet_order_after_stream(s), shc_fleet_get_observations_device, shc_fleet_order_stream_after(s);
  (b) record route:     shc_fleet_order_after_stream(s), shc_fleet_get_outputs_device(q, qd, leg_state_msgs, body_frames),
                        shc_fleet_order_stream_after(s), then on s the torch slicing, cast and concatenation that build the same tensor.  No fleet
                        output carries the body pose: the record route takes the seven doubles of body_frames.odom_to_base_link in its place (the
                        same bytes moved); every other column is compared with (a)'s and must be equal.
Each route runs --iters times back to back between two HIP events on s (the window ends in the event's synchronise); (a) and (b) alternate block by
block, medians over --rounds rounds after one warm-up round of both.  Not a test and not part of bench.py.
Usage: python scripts/observations_bench.py [--sizes 65536 4096] [--out profiles/bench/observations.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("q", "qd", "model_tip", "stance_progress", "swing_progress", "body_pose", "desired_velocity")


def measure(n, iters, rounds):
    import torch
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.engine import BODY_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, observation_columns
    from syropod_highlevel_controller_amd.fleet import MixedFleet

    p = default_hexapod_params("wave")
    p.admittance_control, p.imu_posing = 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    rng = np.random.default_rng(n)
    fleet = MixedFleet([p], np.zeros(n, dtype=np.int32))
    L, D = fleet.max_legs, fleet.max_dof
    fleet.set_velocity(rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n))
    fleet.set_tip_force(np.ascontiguousarray(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 15, (n, L))], axis=2)))
    fleet.step(100)
    fleet.synchronize()
    cols, W = observation_columns(FIELDS, L, D)
    msg_words, body_words = LEG_STATE_MSG_DTYPE.itemsize // 8, BODY_FRAMES_DTYPE.itemsize // 8
    at = lambda dt, name: dt.fields[name][1] // 8
    obs = torch.zeros((n, W), dtype=torch.float32, device="cuda")
    q, qd = (torch.zeros((n, L, D), dtype=torch.float64, device="cuda") for _ in range(2))
    msgs = torch.zeros((n, L, msg_words), dtype=torch.float64, device="cuda")
    body = torch.zeros((n, body_words), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    tip, stance, swing = at(LEG_STATE_MSG_DTYPE, "model_tip_position"), at(LEG_STATE_MSG_DTYPE, "stance_progress"), at(LEG_STATE_MSG_DTYPE, "swing_progress")
    o2b, vel = at(BODY_FRAMES_DTYPE, "odom_to_base_link"), at(BODY_FRAMES_DTYPE, "desired_velocity")

    def observation_pass():
        fleet.order_after(s)
        fleet.observations(obs, FIELDS)
        fleet.order_before(s)
        return obs

    def record_route():
        fleet.order_after(s)
        fleet.outputs(q=q, qd=qd, leg_state_msgs=msgs, body_frames=body)
        fleet.order_before(s)
        with torch.cuda.stream(s):
            return torch.cat([q.reshape(n, -1), qd.reshape(n, -1), msgs[:, :, tip:tip + 3].reshape(n, -1), msgs[:, :, stance], msgs[:, :, swing],
                              body[:, o2b:o2b + 7], body[:, vel:vel + 3]], dim=1).to(torch.float32)

    routes = (("observation_pass", observation_pass), ("record_route", record_route))
    times = {name: [] for name, _ in routes}
    for r in range(rounds + 1):
        for name, fn in routes:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(s)
            for _ in range(iters):
                fn()
            t1.record(s)
            t1.synchronize()
            if r > 0:
                times[name].append(t0.elapsed_time(t1) * 1e3 / iters)
    a, b = observation_pass().clone(), record_route()
    s.synchronize()
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    compared = np.ones(W, dtype=bool)
    compared[cols["body_pose"]] = False
    row = {"n": n, "columns": W, "iters": iters, "rounds": rounds, "columns_equal": bool(a[:, compared].tobytes() == b[:, compared].tobytes()),
           "bytes_written_per_robot": {"observation_pass": W * 4, "record_route": 2 * L * D * 8 + L * msg_words * 8 + body_words * 8}}
    for name, ts in times.items():
        row[name] = {"us_per_call_median": statistics.median(ts), "us_min": min(ts), "us_max": max(ts)}
    row["ratio_pass_over_records"] = row["observation_pass"]["us_per_call_median"] / row["record_route"]["us_per_call_median"]
    fleet.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tensor": "float32 [n, D]: " + ", ".join(FIELDS), "expectation": "ratio <= 0.5 at 65 536 hexapods, <= 1 at 4 096",
              "sizes": [measure(n, args.iters, args.rounds) for n in args.sizes]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
