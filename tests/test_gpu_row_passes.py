"""GPU (-m gpu): the four row passes together.  set_actions and set_footholds take their rows from two column views of ONE wider float32 device
tensor, observations and footholds write theirs into two column views of another; a twin engine takes the same values through the device
setters and the host calls and is read with the record getters.  Equal bytes: the read-back, the dropped rows, get_state, and the joints a few
cycles later - and the columns of the wider tensors that belong to no view are untouched.  The passes share one tile mover (shc_rows.hpp): this
pins that it serves copy-in and copy-out with the same handling of the seam between two rows, on a batch whose last wavefront is partial
(23 hexapods: 10 per wavefront) and on one with idle lanes (14 robots of 5 x 3: 12 per wavefront, four lanes unused)."""
import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import FH_FIELD_NAMES, action_columns, foothold_columns, observation_columns
from test_gpu_actions import action_values, device_setters
from test_gpu_footholds import PLANNER, SENTINEL, TARGET, device_counter, host_calls, host_rows, joint_bits, records, requests, rough, walking
from test_gpu_observations import assert_bits, expected, msg_fields
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

CASES = {"23 hexapods": (lambda: default_hexapod_params("tripod"), 23), "14 robots of 5 x 3": (lambda: synthetic_octopod_params("ripple", 3, 5), 14)}
ACT = ("linear_xy", "angular", "tip_force", "joint_effort")
FH = tuple(FH_FIELD_NAMES)
OBS = ("q", "qd", "joint_effort", "tip_force", "walker_tip", "target_tip", "step_state", "body_pose", "walk_state")


def getters(eng):
    """The fields of OBS from the record getters, as expected() of the observation tests takes them"""
    n, L, D = eng.n, eng.legs, eng.dof
    q, qd = eng.joints()
    ref = {"q": q.reshape(n, L, D), "qd": qd.reshape(n, L, D)}
    ref.update(msg_fields(eng.leg_state_msgs(), D))
    ref["step_state"] = (eng.leg_state()["leg_status"] & 3).astype(np.float64)[:, :, None]
    pose, _, ws = eng.body_state()
    ref["body_pose"], ref["walk_state"] = pose, ws.astype(np.float64)[:, None]
    return ref


@pytest.mark.parametrize("case", list(CASES))
def test_write_and_read_back_through_column_views(case):
    import torch
    make, n = CASES[case]
    p = rough(make())
    L, D = p.leg_count, 3
    (a, b), tips = walking(p, n, 5, stopped=3)
    try:
        A, F, W = action_columns(ACT, L, D)[1], foothold_columns(FH, L)[1], observation_columns(OBS, L, D)[1]
        src = torch.full((n, 5 + A + 3 + F + 4), SENTINEL, dtype=torch.float32, device="cuda")
        act, fh = src[:, 5:5 + A], src[:, 5 + A + 3:5 + A + 3 + F]
        act.copy_(torch.from_numpy(action_values(31, n, ACT, L, D, L, D)).float())
        fh.copy_(torch.from_numpy(requests(tips, FH, L, seed=7)).float())
        before = src.clone()
        counter = device_counter()   # (synchronises: the tensors are complete before the engines, on streams of their own, read them)
        a.set_actions(act, ACT)
        assert a.set_footholds(fh, FH, TARGET, ignored=counter) is None
        keep = device_setters(b, act, ACT, L, D)
        dropped = host_calls(b, fh.double().cpu().numpy(), FH, L)
        a.synchronize(), b.synchronize()
        del keep
        assert int(counter.item()) == dropped
        assert torch.equal(src, before), "a source tensor was written"
        assert state_bytes(a) == state_bytes(b), "the state records differ after the writes"
        assert bytes(a.get_aux_state()) == bytes(b.get_aux_state()), "the auxiliary blobs differ after the writes"

        dst = torch.full((n, 4 + W + 2 + F + 5), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        obs_out, fh_out = dst[:, 4:4 + W], dst[:, 4 + W + 2:4 + W + 2 + F]
        a.observations(OBS, out=obs_out)
        a.footholds(out=fh_out, fields=FH, which=TARGET)
        a.synchronize()
        got = dst.cpu().numpy()
        outside = np.ones(got.shape[1], dtype=bool)
        outside[4:4 + W], outside[4 + W + 2:4 + W + 2 + F] = False, False
        assert (got[:, outside] == np.float32(SENTINEL)).all(), "a column outside the two views was written"
        assert_bits(got[:, 4:4 + W], expected(getters(b), OBS, L, D, 0.0), f"{case}: observations against the twin's getters")
        want, _ = host_rows(got[:, 4 + W + 2:4 + W + 2 + F].astype(np.float64), FH, L, L)
        assert want.tobytes() == records(b, TARGET).tobytes(), "footholds against the twin's get_external_target"
        a.footholds(out=fh_out, fields=FH, which=PLANNER)
        a.synchronize()
        want, _ = host_rows(fh_out.double().cpu().numpy(), FH, L, L)
        assert want.tobytes() == records(b, PLANNER).tobytes(), "planner targets against the twin's get_external_target"

        a.step(3), b.step(3)
        assert joint_bits(a) == joint_bits(b), "the joints differ 3 cycles later"
        a.leg_state(), b.leg_state()   # (both refresh the derived tips)
        assert state_bytes(a) == state_bytes(b), "the state records differ 3 cycles later"
    finally:
        a.close(), b.close()
