"""GPU (-m gpu): shc_engine_get_leg_state_msgs / BatchEngine.leg_state_msgs - StateController::publishLegState (state_controller.cpp:
809-893) for every instance of a batch in one device pass - against the oracle's per-robot orc_get_leg_state_msg and against the getters
that already exist.  Tolerances against the oracle are those of tests/test_gpu_parity.py::test_leg_state_message_payload / _auto_pose:
stance_progress, swing_progress and joint_efforts bit-equal, auto_pose within 1e-12, every other field within 1e-8 absolute."""
import numpy as np
import pytest

from conftest import parity_report
from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, BatchEngine
from syropod_highlevel_controller_amd.params import LegStateMsg
from test_gpu_parity import apply, make_inputs
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

EXACT = ("stance_progress", "swing_progress", "joint_efforts")
COPIED = ("walker_tip_position", "target_tip_position", "poser_tip_position", "model_tip_position", "model_tip_velocity", "joint_positions",
          "joint_velocities", "joint_efforts", "stance_progress", "swing_progress", "admittance_delta", "virtual_stiffness")
DERIVED = ("actual_tip_pose", "time_to_swing_end", "pose_delta", "auto_pose", "tip_force")
FIELDS = [name for name, _ in LegStateMsg._fields_]
assert sorted(COPIED + DERIVED) == sorted(FIELDS)


@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


def as_records(ctypes_msgs, dtype):
    """A list of LegStateMsg -> a structured array (one record per leg)."""
    return np.frombuffer(b"".join(bytes(m) for m in ctypes_msgs), dtype=dtype).copy()


def oracle_msgs(ob, n, dtype, instances=None):
    instances = range(n) if instances is None else instances
    return np.stack([as_records(ob.leg_state_msg(i), dtype) for i in instances])


def dofs_of(p):
    return [p.leg_dof[l] for l in range(p.leg_count)]


def check_against_oracle(got, want, p, where, stats=None):
    """got / want: structured arrays (instances, legs).  Joint arrays are compared over each leg's own DOF; the rest of a joint array is zero."""
    assert got.shape == want.shape, where
    for l, d in enumerate(dofs_of(p)):
        for name in FIELDS:
            a, b = got[name][:, l], want[name][:, l]
            if name.startswith("joint_"):
                assert (a[:, d:] == 0.0).all(), f"{name}: joint slots past DOF {d} of leg {l} are not zero ({where})"
                a, b = a[:, :d], b[:, :d]
            err = float(np.abs(a - b).max())
            if stats is not None:
                stats[name] = max(stats.get(name, 0.0), err)
            if name in EXACT:
                assert np.array_equal(a, b), f"{name} leg {l} {where}: max |d| = {err:.3e}"
            else:
                assert err <= (1e-12 if name == "auto_pose" else 1e-8), f"{name} leg {l} {where}: max |d| = {err:.3e}"


def padded_rows(rows, p):
    """[n][legs][longest DOF] rows -> (engine rows with the padded joints zeroed, oracle rows packed leg by leg)."""
    rows = rows.copy()
    for l, d in enumerate(dofs_of(p)):
        rows[:, l, d:] = 0.0
    n = rows.shape[0]
    return rows.reshape(n, -1), np.concatenate([rows[:, l, :d] for l, d in enumerate(dofs_of(p))], axis=1)


def walk_and_compare(Engine, p, n, seed, steps, force=None, msg_after=2, teacher_forced=False):
    """Engine and oracle side by side from the same inputs; after each entry of `steps` every instance's records are compared.  Fresh
    set_joint_states_msg rows (raw motor positions, efforts) arrive once more than msg_after cycles have run: before that actual_tip_pose is
    the FK of the initial default positions.  teacher_forced: the last cycle before every read starts from the oracle's complete state (legs of
    more than three joints are redundant: the two init chains end on start-up configurations that differ by more than the payload's
    tolerance, tests/test_gpu_parity.py::test_init_chain_on_device_matches_the_oracle - this file checks the payload, not the trajectory)."""
    L, D = p.leg_count, max(dofs_of(p))
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n)
    eff_e, eff_o = padded_rows(rng.normal(0, 0.5, (n, L, D)), p)
    eng, ob = Engine(p, n), OracleBatch(p, n)
    for o, eff in ((eng, eff_e), (ob, eff_o)):
        o.set_velocity(lin, ang)
        o.set_joint_effort(eff)
        if force is not None:
            o.set_tip_force(force)
    done, stats = 0, {}
    for k in steps:
        if teacher_forced:
            if k > 1:
                eng.step(k - 1)
                ob.step(k - 1, 8)
            eng.set_state(ob.get_state())
            eng.step(1)
            ob.step(1, 8)
        else:
            eng.step(k)
            ob.step(k, 8)
        eng.synchronize()
        done += k
        if done > msg_after:  # jointStatesCallback: raw motor positions (offset still in) and efforts -> actual_tip_pose, joint_efforts
            raw_e, raw_o = padded_rows(eng.joints()[0].reshape(n, L, D) + rng.normal(0, 0.02, (n, L, D)) + 0.1, p)
            eff_e, eff_o = padded_rows(rng.normal(0, 0.5, (n, L, D)), p)
            eng.set_joint_states_msg(raw_e, None, eff_e)
            ob.set_joint_states_msg(raw_o, None, eff_o)
        got = eng.leg_state_msgs()
        assert got.shape == (n, L) and got.dtype.itemsize == 512
        check_against_oracle(got, oracle_msgs(ob, n, got.dtype), p, f"after {done} cycles", stats)
    eng.close()
    return stats


def test_every_instance_and_leg_against_the_oracle(Engine):
    """Test 1: hexapod, ripple, admittance + dynamic stiffness, tip forces; n = 47 is not a multiple of the 10 robots of a wavefront.  All 47
    instances after 1, 2, 39, 119 and 152 cycles; the first two reads come before any set_joint_states_msg."""
    p = default_hexapod_params("ripple")
    p.admittance_control, p.dynamic_stiffness = 1, 1
    n = 47
    force = make_inputs(p, n, 83, force=2.0)["force"]
    stats = walk_and_compare(Engine, p, n, 183, (1, 1, 37, 80, 33), force=force)
    parity_report("[leg_state_msgs] hexapod ripple + admittance, 47 instances x 6 legs, 5 reads up to 152 cycles: max |field - oracle| " +
                  ", ".join(f"{k} {v:.1e}" for k, v in sorted(stats.items()) if v > 0))


@pytest.mark.parametrize("case", ["octopod_8x5_ripple", "quadruped_4x4_amble", "mixed_dof_ripple"])
def test_other_morphologies_against_the_oracle(Engine, case):
    """Test 2: 8 legs x 5 joints, 4 legs x 4 joints, and a hexapod with legs of 3 / 5 / 4 joints (joint arrays compared over each leg's own
    DOF, the padded slots zero); n leaves the last wavefront partly filled (8, 16 and 10 robots per wavefront).  The oracle's leg_state_msg
    serves all three.  Teacher-forced (see walk_and_compare)."""
    if case.startswith("octopod"):
        p, n = synthetic_octopod_params("ripple", 5, 8), 19
    elif case.startswith("quadruped"):
        p, n = synthetic_octopod_params("amble", 4, 4), 37
    else:
        p, n = synthetic_mixed_dof_params("ripple"), 23
        assert sorted(set(dofs_of(p))) == [3, 4, 5]
    walk_and_compare(Engine, p, n, 190, (1, 1, 30, 45), teacher_forced=True)


@pytest.mark.parametrize("own_clock", [False, True])
def test_auto_pose_of_every_instance(Engine, own_clock):
    """Test 3: the parameter set of test_gpu_parity.py::test_leg_state_message_auto_pose; auto_pose of every instance after each step count."""
    p = default_hexapod_params("tripod")
    p.auto_posing = 1
    for l in range(6):
        p.negation_transition_ratio[l] = 0.25
    for i in range(p.n_auto_posers):
        p.x_amplitudes[i], p.yaw_amplitudes[i] = 0.004 * (-1) ** i, 0.01
        if i % 2:
            p.gravity_amplitudes[i] = 0.008
    if own_clock:
        p.pose_frequency = 0.8
        base = p.pose_phase_length
        k = int((1.0 / p.pose_frequency) / p.time_delta / base)
        length = (k if k % 2 == 0 else k + 1) * base
        p.time_to_start = ((299 // length) * length + 1) * p.time_delta
    n = 16
    inp = make_inputs(p, n, 85, imu=True, zero_every=5)
    eng, ob = Engine(p, n), OracleBatch(p, n)
    apply(eng, inp)
    apply(ob, inp)
    seen = 0.0
    for k in (1, 1, 30, 17, 23, 41, 60, 9):
        eng.step(k)
        eng.synchronize()
        ob.step(k, 8)
        got = eng.leg_state_msgs()
        want = oracle_msgs(ob, n, got.dtype)
        np.testing.assert_allclose(got["auto_pose"], want["auto_pose"], rtol=0, atol=1e-12)
        seen = max(seen, float(np.abs(want["auto_pose"][..., :3]).max()))
    assert seen > 1e-3


def walking_hexapods(Engine, n, seed, cycles, with_oracle=False):
    p = default_hexapod_params("ripple")
    p.admittance_control, p.dynamic_stiffness = 1, 1
    inp = make_inputs(p, n, seed, force=2.0)
    eng = Engine(p, n)
    apply(eng, inp)
    eng.step(cycles)
    rng = np.random.default_rng(seed + 1)
    eng.set_joint_states_msg(eng.joints()[0] + rng.normal(0, 0.02, (n, 18)) + 0.1, None, rng.normal(0, 0.5, (n, 18)))
    eng.step(3)
    eng.synchronize()
    return p, eng


def check_against_per_instance_call(eng, got, instances):
    for i in instances:
        one = as_records(eng.leg_state_msg(int(i)), got.dtype)
        for name in FIELDS:  # the per-instance call is the batched pass for [i, i + 1): the device's bits in every field
            assert np.array_equal(got[name][i], one[name]), (name, i)


def test_agreement_with_the_existing_getters(Engine):
    """Test 4: the copied fields are the bytes of shc_engine_get_leg_state / get_joint_state / get_virtual_stiffness; against the per-instance
    call every field is byte-equal."""
    n = 53
    p, eng = walking_hexapods(Engine, n, 91, 77)
    got = eng.leg_state_msgs()
    ls = eng.leg_state()
    assert np.array_equal(got["walker_tip_position"], ls["walker_tip"])
    assert np.array_equal(got["poser_tip_position"], ls["poser_tip"])
    assert np.array_equal(got["model_tip_position"], ls["model_tip"])
    assert np.array_equal(got["admittance_delta"], ls["admittance"])
    q, qd = eng.joints()
    assert np.array_equal(got["joint_positions"][..., :3], q.reshape(n, 6, 3))
    assert np.array_equal(got["joint_velocities"][..., :3], qd.reshape(n, 6, 3))
    assert (got["joint_positions"][..., 3:] == 0).all() and (got["joint_velocities"][..., 3:] == 0).all() and (got["joint_efforts"][..., 3:] == 0).all()
    assert np.array_equal(got["virtual_stiffness"], eng.virtual_stiffness())
    assert np.abs(got["virtual_stiffness"]).max() > 0 and np.abs(got["tip_force"]).max() > 0
    check_against_per_instance_call(eng, got, (0, 9, 10, 31, n - 1))
    eng.close()


def test_ranges_device_output_and_refusals(Engine):
    """Test 5: sub-ranges are slices of the full call; the device form writes the bytes of the host form and nothing past count x legs
    records; NULL / out-of-range arguments and resident mode are refused."""
    import torch
    n = 47
    p, eng = walking_hexapods(Engine, n, 95, 60)
    full = eng.leg_state_msgs()
    for first, count in ((0, 1), (n - 1, 1), (7, 13), (19, 2), (0, n)):
        part = eng.leg_state_msgs(first, count)
        assert part.shape == (count, 6)
        assert part.tobytes() == full[first:first + count].tobytes(), (first, count)
    assert eng.leg_state_msgs(5, 0).shape == (0, 6)
    sentinel = -12345.678
    for first, count in ((0, n), (7, 13)):
        buf = torch.full(((count * 6 + 3) * 64,), sentinel, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert eng.leg_state_msgs(first, count, out=buf.data_ptr()) is None
        eng.synchronize()
        host = buf.cpu().numpy()
        assert host[:count * 6 * 64].tobytes() == full[first:first + count].tobytes()
        assert (host[count * 6 * 64:] == sentinel).all()
    lib, h = eng.L, eng.h
    arr = (LegStateMsg * (n * 6))()
    assert lib.shc_engine_get_leg_state_msgs(h, 0, n, None, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_get_leg_state_msgs(h, -1, 2, arr, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_get_leg_state_msgs(h, 1, n, arr, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_get_leg_state_msgs(h, 0, -1, arr, 0) == SHC_ERR_INVALID_ARG
    assert eng.leg_state_msgs().tobytes() == full.tobytes()   # ... and none of these calls has changed anything
    eng.resident_begin(ring_depth=4, max_cycles=50)
    try:
        assert lib.shc_engine_get_leg_state_msgs(h, 0, n, arr, 0) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    assert eng.leg_state_msgs().shape == (n, 6)   # served again once resident mode has ended
    eng.close()


@pytest.mark.parametrize("case", ["auto_posing", "manual_leg"])
def test_reading_does_not_disturb_the_run(Engine, case):
    """Test 6: two engines with the same inputs, one reads its LegState records every few cycles: state records and joints stay equal byte
    for byte over 120 cycles.  auto_posing: the poser tip is state, not derived.  manual_leg: after toggle_leg_state has put a leg of some
    robots into MANUAL; those robots' records agree with the per-instance call."""
    p = default_hexapod_params("tripod")
    n = 23
    if case == "auto_posing":
        p.auto_posing = 1
        for i in range(p.n_auto_posers):
            p.x_amplitudes[i], p.yaw_amplitudes[i] = 0.004 * (-1) ** i, 0.01
    inp = make_inputs(p, n, 97, imu=(case == "auto_posing"))
    a, b = Engine(p, n), Engine(p, n)
    for e in (a, b):
        apply(e, inp)
    if case == "manual_leg":
        sel = np.full(n, -1, dtype=np.int32)
        sel[::3] = np.arange(len(sel[::3])) % 6   # every third robot toggles a leg, the others keep walking
        lin, ang = inp["lin"].copy(), inp["ang"].copy()
        for e in (a, b):
            e.step(20)
        pending = sel >= 0
        for _ in range(3000):   # legStateToggle as tests/test_gpu_manual_legs.py drives it: -1 = still walking (the node zeroes that robot's
            if not pending.any():   # velocity inputs), 1 / 2 = the request has been served
                break
            cur = np.where(pending, sel, -1).astype(np.int32)
            ra, rb = a.toggle_leg_state(cur), b.toggle_leg_state(cur)
            assert np.array_equal(ra, rb)
            if (ra == -1).any():
                lin[ra == -1], ang[ra == -1] = 0.0, 0.0
                for e in (a, b):
                    e.set_velocity(lin, ang)
            pending &= ~((ra == 1) | (ra == 2))
        assert not pending.any()
        manual = a.leg_manipulation_state()
        assert (manual[::3].max(axis=1) == 1).all() and (manual.sum(axis=1)[sel < 0] == 0).all(), "the designated legs did not reach MANUAL"
    for c in range(120):
        for e in (a, b):
            e.step(1)
        if c % 7 == 0:
            got = a.leg_state_msgs()
            if c % 28 == 0:
                check_against_per_instance_call(a, got, (0, 3, 6, n - 1))
    for e in (a, b):
        e.synchronize()
    assert state_bytes(a) == state_bytes(b)
    for e in (a, b):   # the aux blob carries the LegPoser tips, a derived plane every getter refreshes (shc_engine_get_leg_state): refreshed on both
        e.leg_state()  # sides, the blobs are equal if the batched call has done nothing beyond that
    assert a.get_aux_state() == b.get_aux_state()
    for x, y in zip(a.joints(), b.joints()):
        assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


def test_split_stream_batch_into_a_device_buffer(Engine):
    """Test 7: 41 000 hexapods (steps run as two halves on two streams); one call into a device buffer.  Copied fields of ALL instances are
    the bytes of get_leg_state / get_joint_state; 64 instances (first, last, random) against a 64-robot oracle fed their inputs."""
    import torch
    from syropod_highlevel_controller_amd.engine import LEG_STATE_MSG_DTYPE
    p = default_hexapod_params("ripple")
    n, cycles = 41000, 25
    rng = np.random.default_rng(101)
    lin, ang = rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n)
    effort = rng.normal(0, 0.5, size=(n, 18))
    eng = Engine(p, n)
    eng.set_velocity(lin, ang)
    eng.set_joint_effort(effort)
    for _ in range(cycles):
        eng.step(1)
    buf = torch.zeros(n * 6 * 64, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.leg_state_msgs(out=buf.data_ptr())
    eng.synchronize()
    got = buf.cpu().numpy().view(LEG_STATE_MSG_DTYPE).reshape(n, 6)
    ls = eng.leg_state()
    assert np.array_equal(got["walker_tip_position"], ls["walker_tip"])
    assert np.array_equal(got["poser_tip_position"], ls["poser_tip"])
    assert np.array_equal(got["model_tip_position"], ls["model_tip"])
    q, qd = eng.joints()
    assert np.array_equal(got["joint_positions"][..., :3], q.reshape(n, 6, 3))
    assert np.array_equal(got["joint_velocities"][..., :3], qd.reshape(n, 6, 3))
    assert np.array_equal(got["joint_efforts"][..., :3], effort.reshape(n, 6, 3))
    pick = np.unique(np.concatenate([[0, n - 1], rng.choice(n, 62, replace=False)]))[:64]
    ob = OracleBatch(p, len(pick))
    ob.set_velocity(lin[pick], ang[pick])
    ob.set_joint_effort(effort[pick])
    ob.step(cycles, 8)
    check_against_oracle(got[pick], oracle_msgs(ob, len(pick), got.dtype), p, "split-stream batch")
    eng.close()


def test_fleet_records_in_caller_order(Engine):
    """Test 8: hexapods (6 x 3) and octopods (8 x 5) interleaved in one fleet on one device: records arrive in the caller's instance order,
    each robot's records are its part engine's, and records [6, 8) of the hexapods are all zero."""
    from syropod_highlevel_controller_amd.fleet import MixedFleet
    morphs = [default_hexapod_params("tripod"), synthetic_octopod_params("ripple", 5, 8)]
    n = 29
    mid = (np.arange(n) % 3 == 1).astype(np.int32)
    rng = np.random.default_rng(111)
    fleet = MixedFleet(morphs, mid)
    assert (fleet.max_legs, fleet.max_dof) == (8, 5)
    fleet.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
    fleet.set_joint_effort(rng.normal(0, 0.5, size=(n, 8, 5)))
    fleet.step(45)
    fleet.synchronize()
    got = fleet.leg_state_msgs()
    assert got.shape == (n, 8)
    seen = np.zeros(n, dtype=bool)
    for handle, m, _, ids in fleet.parts():
        part = BatchEngine.view(handle, morphs[m], len(ids)).leg_state_msgs()
        L = morphs[m].leg_count
        assert part.shape == (len(ids), L) and (mid[ids] == m).all()
        assert got[ids, :L].tobytes() == part.tobytes()
        assert got[ids, L:].tobytes() == bytes(len(ids) * (8 - L) * 512)
        assert np.abs(part["walker_tip_position"]).max() > 0
        seen[ids] = True
    assert seen.all()
    fleet.close()
