"""GPU: shc_engine_get_state / shc_engine_set_state after the move onto one record walk (csrc/shc_snapshot.hpp: state_kernel<NJ, TO_ENGINE>),
and a robot's LegState.msg through the batched pass.

Six small batches, each one robot more than a wavefront holds (10, 8 and 16 robots per wavefront for 6, 8 and 4 legs: n = 11, 9, 17); the first half of
a batch walks, the second half has no velocity command and stands.  Per case:
(a) the bytes of get_state() after 1, 40 and 60 cycles;
(b) a get_state(first, count) sub-range across the wavefront boundary is the slice of (a) (no golden);
(c) the last records, injected in reversed robot order into a fresh engine of the same parameters: the bytes of get_state() right after, and again
    after 3 more cycles with the same held inputs;
(d) case 1 only: the same with some legs' swing_progress = stance_progress = -1, the progress mode no walk produces.
(a), (c) and (d) are compared byte for byte with tests/golden/state_records_golden.npz - what the commit before the one walk returned for the same calls on
an MI355X (`python tests/test_gpu_state_records.py OUT.npz` records it, with that commit's package on PYTHONPATH; the recorder refuses records that do
not exercise the members each case is there for: `check_coverage`)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "state_records_golden.npz")
pytestmark = pytest.mark.gpu

READS = (1, 40, 60)   # cycles run at each read
LOST = 2147483647.0   # a range sensor that lost contact (standard_includes.h:57)
CASES = ("hexapod_ripple_efforts", "hexapod_tripod_auto_pose", "hexapod_ripple_imu_rough", "octopod_8x5_gravity", "quadruped_4x4_amble", "mixed_dof_gravity")
SEED = {name: 300 + i for i, name in enumerate(CASES)}


def case_params(name):
    """(parameters, robots, a sub-range that crosses the wavefront boundary)"""
    from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
    if name == "hexapod_ripple_efforts":
        p = default_hexapod_params("ripple")
        p.admittance_control, p.use_joint_effort, p.force_gain = 1, 1, 0.05
    elif name == "hexapod_tripod_auto_pose":   # the amplitude / negation set of tests/test_gpu_parity.py::test_leg_state_message_auto_pose
        p = default_hexapod_params("tripod")
        p.auto_posing, p.admittance_control, p.dynamic_stiffness = 1, 1, 1
        p.inclination_posing = 1   # the engine keeps auto_pose_rotation only for the cycle that reads it back: updateInclinationPose
        for l in range(6):
            p.negation_transition_ratio[l] = 0.25
        for i in range(p.n_auto_posers):
            p.x_amplitudes[i], p.yaw_amplitudes[i] = 0.004 * (-1) ** i, 0.01
            if i % 2:
                p.gravity_amplitudes[i] = 0.008
    elif name == "hexapod_ripple_imu_rough":
        p = default_hexapod_params("ripple")
        p.imu_posing, p.rough_terrain_mode = 1, 1
    elif name == "octopod_8x5_gravity":
        p = synthetic_octopod_params("ripple", 5, 8)
        p.gravity_aligned_tips = 1
        return p, 9, (6, 3)
    elif name == "quadruped_4x4_amble":
        return synthetic_octopod_params("amble", 4, 4), 17, (14, 3)
    else:
        p = synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4))
        p.gravity_aligned_tips, p.time_to_start = 1, 2.0
    return p, 11, (8, 3)


def case_inputs(name, p, n):
    """The held inputs, and for the rough-terrain case the IMU / step-plane rows set before each read."""
    rng = np.random.default_rng(SEED[name])
    L = p.leg_count
    inp = {"lin": rng.uniform(-0.6, 0.6, (n, 2)), "ang": rng.uniform(-0.8, 0.8, n)}
    inp["lin"][n // 2:], inp["ang"][n // 2:] = 0.0, 0.0
    if name == "hexapod_ripple_efforts":
        inp["effort"] = rng.normal(0, 0.5, (n, L * 3))
    if name == "hexapod_tripod_auto_pose":
        inp["force"] = np.abs(rng.normal(0, 2.0, (n, L, 3)))
    if name == "hexapod_ripple_imu_rough":
        inp["imu"], inp["step_plane"] = [], []
        for _ in READS:
            axis, half = rng.normal(0, 1, (n, 3)), 0.5 * rng.uniform(0.02, 0.15, (n, 1))
            axis /= np.linalg.norm(axis, axis=1, keepdims=True)
            inp["imu"].append((np.concatenate([np.cos(half), np.sin(half) * axis], axis=1), rng.normal(0, 0.05, (n, 3))))
            sp = np.stack([rng.normal(0, 0.1, (n, L)), rng.normal(0, 0.1, (n, L)), rng.uniform(0.0, 0.03, (n, L))], axis=2)
            sp[rng.random((n, L)) < 0.3, 2] = LOST
            inp["step_plane"].append(sp)
    return inp


def hold(e, inp, order=slice(None), read=-1):
    """Apply the held inputs (rows in `order`)."""
    e.set_velocity(inp["lin"][order], inp["ang"][order])
    if "effort" in inp:
        e.set_joint_effort(inp["effort"][order])
    if "force" in inp:
        e.set_tip_force(inp["force"][order])
    if "imu" in inp:
        e.set_imu(inp["imu"][read][0][order], inp["imu"][read][1][order])
        e.set_tip_states_msg(None, inp["step_plane"][read][order])


def state_bytes(e, *rng):
    return np.frombuffer(bytes(e.get_state(*rng)), dtype=np.uint8)


def records(raw):
    from syropod_highlevel_controller_amd.params import InstanceState
    return np.frombuffer(raw.tobytes(), dtype=np.dtype(InstanceState))


def injected(make, p, n, recs, inp):
    """`recs` (a structured array, already in the order to inject) into a fresh engine: get_state right after, and after 3 more cycles."""
    from syropod_highlevel_controller_amd.params import InstanceState
    e = make(p, n)
    try:
        hold(e, inp, order=slice(None, None, -1))
        e.set_state((InstanceState * n).from_buffer_copy(recs.tobytes()))
        first = state_bytes(e)
        e.step(3)
        return first, state_bytes(e)
    finally:
        e.close()


def record_case(name, make, sub_ranges=True):
    p, n, (first, count) = case_params(name)
    inp = case_inputs(name, p, n)
    out, done = {}, 0
    e = make(p, n)
    try:
        for k, cycles in enumerate(READS):
            hold(e, inp, read=k)
            e.step(cycles - done)
            done = cycles
            out[f"{name}.read{cycles}"] = state_bytes(e)
            if sub_ranges:
                size = out[f"{name}.read{cycles}"].size // n
                assert state_bytes(e, first, count).tobytes() == out[f"{name}.read{cycles}"][first * size:(first + count) * size].tobytes(), (name, cycles)
    finally:
        e.close()
    last = records(out[f"{name}.read{READS[-1]}"])[::-1].copy()
    out[f"{name}.injected"], out[f"{name}.injected+3"] = injected(make, p, n, last, inp)
    if name == CASES[0]:
        for i in range(n):
            for l in range(p.leg_count):
                if (i + l) % 3 == 0:
                    last["leg"]["swing_progress"][i, l] = last["leg"]["stance_progress"][i, l] = -1.0
        out[f"{name}.edited"], out[f"{name}.edited+3"] = injected(make, p, n, last, inp)
    return out


def check_coverage(name, out):
    """What each case is there for occurs in its records: a golden that exercises nothing is not recordable."""
    p, n, _ = case_params(name)
    L = p.leg_count
    r40, r60 = records(out[f"{name}.read40"]), records(out[f"{name}.read60"])
    for r in (r40, r60):
        swing, stance = r["leg"]["swing_progress"][:, :L], r["leg"]["stance_progress"][:, :L]
        assert (swing >= 0).any() and (stance > 0).any() and (stance == 0).any(), (name, "progress modes")
    both = np.concatenate([r40, r60])
    assert len(set(both["walk_state"].tolist())) >= 2, (name, "walk states", set(both["walk_state"].tolist()))
    leg = both["leg"][:, :L]
    nz = lambda a: bool(np.any(a != 0))

    def occur(**members):
        missing = [k for k, a in members.items() if not nz(a)]
        assert not missing, (name, "all zero in the records", missing)
    if name == "hexapod_ripple_efforts":
        occur(tip_force_calculated=leg["tip_force_calculated"], admittance_state=leg["admittance_state"], virtual_stiffness=leg["virtual_stiffness"])
        edited = records(out[f"{name}.edited"])["leg"][:, :L]
        assert ((edited["swing_progress"] == -1) & (edited["stance_progress"] == -1)).any(), (name, "the fourth progress mode")
    if name == "hexapod_tripod_auto_pose":
        occur(auto_poser_flags=both["auto_poser_flags"], negate_auto_pose=leg["negate_auto_pose"], auto_pose_rotation_xyz=both["auto_pose_rotation"][:, 1:],
              admittance_delta=leg["admittance_delta"])
    if name == "hexapod_ripple_imu_rough":
        occur(rotation_absement_error=both["rotation_absement_error"])
        assert set(leg["step_plane_defined"].ravel().tolist()) == {0, 1} and (both["touchdown_detection"] == 1).all(), name
    if name in ("octopod_8x5_gravity", "mixed_dof_gravity"):
        long_legs = np.array([p.leg_dof[l] > 3 for l in range(L)])
        for flag in ("tip_rotation_defined", "target_rotation_defined"):
            assert nz(leg[flag][:, long_legs]) and not nz(leg[flag][:, ~long_legs]), (name, flag)
        assert long_legs.all() == (name == "octopod_8x5_gravity")
    if name == "mixed_dof_gravity":
        occur(tip_align_pose=r60["tip_align_pose"])


def engine(p, n):
    from syropod_highlevel_controller_amd.engine import BatchEngine
    return BatchEngine(p, n)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", CASES)
def test_records_against_the_recorded_parent(golden, name):
    got = record_case(name, engine)
    want = {k: v for k, v in golden.items() if k.startswith(name + ".")}
    assert sorted(want) == sorted(got)
    check_coverage(name, want)
    for k in sorted(want):
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and want[k].tobytes() == got[k].tobytes(), k


def test_one_robots_leg_state_msg_is_the_batched_pass():
    """leg_state_msg(i) returns the bytes of leg_state_msgs(i, 1) and of leg_state_msgs()[i]; an instance out of range is refused."""
    from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG
    from syropod_highlevel_controller_amd.params import LegStateMsg
    name = "hexapod_tripod_auto_pose"
    p, n, _ = case_params(name)
    inp = case_inputs(name, p, n)
    e = engine(p, n)
    try:
        hold(e, inp)
        e.step(40)
        full = e.leg_state_msgs()
        assert np.abs(full["auto_pose"][..., :3]).max() > 0 and np.abs(full["admittance_delta"]).max() > 0
        for i in (0, 9, 10):
            one = b"".join(bytes(m) for m in e.leg_state_msg(i))
            assert one == e.leg_state_msgs(i, 1).tobytes() and one == full[i].tobytes(), i
        msgs = (LegStateMsg * p.leg_count)()
        for i in (-1, n):
            assert e.L.shc_engine_read_leg_state_msg(e.h, i, msgs) == SHC_ERR_INVALID_ARG and b"instance out of range" in e.L.shc_last_error()
    finally:
        e.close()


if __name__ == "__main__":   # record the golden: with the package of the commit whose behaviour is the reference on PYTHONPATH
    recorded = {}
    for case in CASES:
        recorded.update(record_case(case, engine))
        check_coverage(case, recorded)
        print(case, "recorded", flush=True)
    np.savez_compressed(sys.argv[1], **recorded)
