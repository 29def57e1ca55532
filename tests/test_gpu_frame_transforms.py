"""GPU (-m gpu): shc_engine_get_frame_transforms / BatchEngine.frame_transforms - StateController::publishFrameTransforms
(state_controller.cpp:963-1047) for every instance of a batch in one device pass - against the numpy reading of the reference in
tests/frames_numpy.py, against the oracle's Leg::applyFK and against the getters that already exist.

Bars: joint / tip frames 1e-8 absolute per component against the numpy reading and the oracle (the bar tests/test_gpu_leg_state_msgs.py
holds actual_tip_pose to), quaternions component by component with their sign; a frame whose rotation matrix lies within 1e-6 of a branch
boundary of Eigen's matrix-to-quaternion may be compared up to overall sign, and such frames stay under 1 % of the frames compared (asserted).
Body records and the odom_ideal form 1e-12 (two pose compositions and one Euler extraction of FP64 inputs); tip position against
model_tip_position 1e-12; desired_velocity bit-equal."""
import ctypes as C

import numpy as np
import pytest

import frames_numpy as fn
from conftest import parity_report
from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (BODY_FRAMES_DTYPE, LEG_FRAMES_DTYPE, SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, BatchEngine)
from syropod_highlevel_controller_amd.params import WALK_STOPPED
from test_gpu_parity import apply, make_inputs
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

TOL_FRAME, TOL_BODY, NEAR_CAP = 1e-8, 1e-12, 0.01


@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


def dofs_of(p):
    return [p.leg_dof[l] for l in range(p.leg_count)]


def pose_error(got, want, near):
    """max |component difference| of poses (..., 7); where `near`, the quaternion may carry the other overall sign."""
    d = np.abs(got - want).max(axis=-1)
    flipped = want * np.array([1, 1, 1, -1, -1, -1, -1.0])
    d = np.where(near, np.minimum(d, np.abs(got - flipped).max(axis=-1)), d)
    return float(d.max()) if d.size else 0.0


def check_legs_against_numpy(lf, p, q, where, stats):
    """lf: structured (n, legs) records; q: joints()[0].  Every joint frame of each leg's own DOF and every tip against the numpy reading;
    joint slots past a leg's DOF exactly zero.  Returns (frames compared, frames near a branch boundary)."""
    joint, tip, near = fn.robot_frames(p, q)
    compared = n_near = 0
    for l, d in enumerate(dofs_of(p)):
        assert (lf["joint"][:, l, d:] == 0.0).all(), f"joint slots past DOF {d} of leg {l} are not zero ({where})"
        ej = pose_error(lf["joint"][:, l, :d], joint[:, l, :d], near[:, l, :d])
        et = pose_error(lf["tip"][:, l], tip[:, l], near[:, l, fn.FRAME_JOINTS])
        stats["joint"], stats["tip"] = max(stats.get("joint", 0.0), ej), max(stats.get("tip", 0.0), et)
        assert ej <= TOL_FRAME, f"joint frames of leg {l} {where}: max |d| = {ej:.3e}"
        assert et <= TOL_FRAME, f"tip frame of leg {l} {where}: max |d| = {et:.3e}"
        compared += lf.shape[0] * (d + 1)
        n_near += int(near[:, l, :d].sum() + near[:, l, fn.FRAME_JOINTS].sum())
    return compared, n_near


def check_body_against_numpy(bf, eng, where, stats):
    pose, vel, _ = eng.body_state()
    want = fn.body_frames(eng.odometry(), pose, vel)
    for name in ("odom_to_base_link", "base_link_to_walk_plane", "pose_euler"):
        err = float(np.abs(bf[name] - want[name]).max())
        stats[name] = max(stats.get(name, 0.0), err)
        assert err <= TOL_BODY, f"{name} {where}: max |d| = {err:.3e}"
    assert np.array_equal(bf["desired_velocity"], vel), where


def walk_and_check(Engine, p, n, seed, label):
    """Random velocity commands; reads before the first cycle, after it, mid-swing, after a change of command and after a stop."""
    rng = np.random.default_rng(seed)
    L, D = p.leg_count, max(dofs_of(p))
    eng = Engine(p, n)
    eng.set_joint_effort(np.zeros((n, L * D)))
    stats, compared, n_near, done = {}, 0, 0, 0
    schedule = [(0, "random"), (1, None), (1, None), (31, None), (44, "random"), (23, None), (300, "stop")]
    for cycles, command in schedule:
        if command == "random":
            eng.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
        elif command == "stop":
            eng.set_velocity(np.zeros((n, 2)), np.zeros(n))
        if cycles:
            eng.step(cycles)
        done += cycles
        lf, bf = eng.frame_transforms()
        assert lf.shape == (n, L) and lf.dtype.itemsize == 336 and bf.shape == (n,) and bf.dtype.itemsize == 160
        c, k = check_legs_against_numpy(lf, p, eng.joints()[0], f"after {done} cycles", stats)
        compared, n_near = compared + c, n_near + k
        check_body_against_numpy(bf, eng, f"after {done} cycles", stats)
        np.testing.assert_allclose(lf["tip"][..., :3], eng.leg_state_msgs()["model_tip_position"], rtol=0, atol=1e-12)
    assert (eng.body_state()[2] == WALK_STOPPED).all(), "the last read is meant to come after every robot has stopped"
    eng.close()
    share = n_near / compared
    parity_report(f"[frame_transforms] {label}, {n} instances, {len(schedule)} reads up to {done} cycles: max |frame - numpy reading| " +
                  ", ".join(f"{k} {v:.1e}" for k, v in sorted(stats.items())) + f"; {n_near} of {compared} frames near a branch boundary")
    assert share < NEAR_CAP, f"{n_near} of {compared} frames lie near a branch boundary"


@pytest.mark.parametrize("case", ["hexapod_6x3_ripple", "octopod_8x5_ripple", "quadruped_4x4_amble", "mixed_dof_ripple"])
def test_joint_and_tip_frames_against_the_numpy_reading(Engine, case):
    """Tests 1 and 5: every instance, leg and joint on four morphologies; n leaves the last wavefront partly filled (10, 8, 16 and 10 robots
    per wavefront).  On the hexapod with 3 / 5 / 4-joint legs the slots past a leg's own DOF are exactly zero and its tip is the tip of the
    numpy chain of its own joint count."""
    if case.startswith("hexapod"):
        p, n = default_hexapod_params("ripple"), 47
    elif case.startswith("octopod"):
        p, n = synthetic_octopod_params("ripple", 5, 8), 19
    elif case.startswith("quadruped"):
        p, n = synthetic_octopod_params("amble", 4, 4), 37
    else:
        p, n = synthetic_mixed_dof_params("ripple"), 23
        assert sorted(set(dofs_of(p))) == [3, 4, 5]
    walk_and_check(Engine, p, n, 211, case)


@pytest.mark.parametrize("case", ["hexapod_free_running", "octopod_8x5_teacher_forced"])
def test_tip_frame_against_the_oracle(Engine, case):
    """Test 2: tip = Leg::applyFK of the oracle's robots (orc_leg_apply_fk(r, leg, NULL, ...)) within 1e-8.  The octopod's legs are
    redundant: the last cycle before every read starts from the oracle's complete state, as tests/test_gpu_leg_state_msgs.py does."""
    teacher_forced = case.startswith("octopod")
    p, n = (synthetic_octopod_params("ripple", 5, 8), 19) if teacher_forced else (default_hexapod_params("ripple"), 47)
    L, D = p.leg_count, max(dofs_of(p))
    rng = np.random.default_rng(223)
    lin, ang = rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n)
    eng, ob = Engine(p, n), OracleBatch(p, n)
    for o in (eng, ob):
        o.set_velocity(lin, ang)
        o.set_joint_effort(np.zeros((n, L * D)))
    worst, done = 0.0, 0
    for k in (1, 1, 30, 45, 60):
        if teacher_forced:
            if k > 1:
                eng.step(k - 1)
                ob.step(k - 1, 8)
            eng.set_state(ob.get_state())
        else:
            eng.step(k - 1) if k > 1 else None
            ob.step(k - 1, 8) if k > 1 else None
        eng.step(1)
        ob.step(1, 8)
        done += k
        lf, _ = eng.frame_transforms(body=False)
        want = ob.leg_apply_fk(None).reshape(n, L, 7)
        err = float(np.abs(lf["tip"] - want).max())
        worst = max(worst, err)
        assert err <= TOL_FRAME, f"tip frame after {done} cycles: max |d| = {err:.3e}"
        np.testing.assert_allclose(lf["tip"][..., :3], eng.leg_state_msgs()["model_tip_position"], rtol=0, atol=1e-12)
    parity_report(f"[frame_transforms] {case}, {n} instances x {L} legs, 5 reads up to {done} cycles: max |tip - oracle applyFK| {worst:.1e}")
    eng.close()


def posed_turning_hexapods(Engine, n, seed, cycles):
    """IMU posing + manual pose input (the body rotation is not the identity) and every robot turning (the odometry yaw leaves zero)."""
    p = default_hexapod_params("ripple")
    p.imu_posing = 1
    p.rotation_pid_gains[:] = [0.8, 0.1, 0.05]
    p.max_translation[:] = [0.02, 0.015, 0.01]
    p.max_rotation[:] = [0.05, 0.04, 0.06]
    rng = np.random.default_rng(seed)
    inp = make_inputs(p, n, seed, imu=True)
    inp["ang"] = rng.uniform(0.5, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    inp["tv"], inp["rv"] = rng.uniform(-1, 1, size=(n, 3)), rng.uniform(-1, 1, size=(n, 3))
    eng = Engine(p, n)
    apply(eng, inp)
    eng.step(cycles)
    return p, eng


def test_body_records_and_the_odom_ideal_frame(Engine):
    """Tests 3 and 4: the body records against the numpy reading of get_body_state / get_odometry outputs, 1e-12, with a posed body and a
    turned odometry; SHC_FRAME_ODOM_IDEAL = odom_to_base_link.addPose(child) of the SHC_FRAME_BASE_LINK records, 1e-12, the body records the
    same for both frames."""
    n = 47
    p, eng = posed_turning_hexapods(Engine, n, 227, 240)
    stats = {}
    for more in (0, 1, 57):
        if more:
            eng.step(more)
        lf, bf = eng.frame_transforms()
        check_body_against_numpy(bf, eng, f"after {240 + more} cycles", stats)
        wl, wb = eng.frame_transforms(frame="odom_ideal")
        assert wb.tobytes() == bf.tobytes()
        o2b = bf["odom_to_base_link"]
        ej = float(np.abs(wl["joint"][:, :, :3] - fn.add_pose(o2b[:, None, None, :], lf["joint"][:, :, :3])).max())
        et = float(np.abs(wl["tip"] - fn.add_pose(o2b[:, None, :], lf["tip"])).max())
        stats["odom_ideal joint"], stats["odom_ideal tip"] = max(stats.get("odom_ideal joint", 0.0), ej), max(stats.get("odom_ideal tip", 0.0), et)
        assert ej <= TOL_BODY and et <= TOL_BODY, (ej, et)
        assert (wl["joint"][:, :, 3:] == 0.0).all()
    pose, _, _ = eng.body_state()
    odo = eng.odometry()
    yaw = 2.0 * np.arctan2(odo[:, 6], odo[:, 3])
    assert np.abs(pose[:, 4:]).max(axis=1).min() > 1e-3, "the body rotation is meant to differ from the identity on every robot"
    assert np.abs(yaw).min() > 0.2, "the odometry yaw is meant to be well away from zero on every robot"
    assert np.abs(bf["pose_euler"]).max() > 1e-2 and np.abs(bf["base_link_to_walk_plane"][:, :3]).max() > 1e-3
    parity_report(f"[frame_transforms] body records, IMU posing + manual pose input, {n} turning hexapods (|yaw| {np.abs(yaw).min():.2f} .. "
                  f"{np.abs(yaw).max():.2f} rad): max |d| " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(stats.items())))
    eng.close()


def walking_hexapods(Engine, n, seed, cycles):
    p = default_hexapod_params("ripple")
    eng = Engine(p, n)
    apply(eng, make_inputs(p, n, seed))
    eng.step(cycles)
    eng.synchronize()
    return p, eng


def test_ranges_forms_and_refusals(Engine):
    """Test 6: sub-ranges are slices of the full read; legs-only and body-only calls; the device form writes the bytes of the host form and
    nothing past the records asked for; count = 0; invalid arguments and resident mode are refused."""
    import torch
    n = 47
    p, eng = walking_hexapods(Engine, n, 229, 60)
    for frame in ("base_link", "odom_ideal"):
        full_l, full_b = eng.frame_transforms(frame=frame)
        for first, count in ((0, 1), (n - 1, 1), (7, 13), (19, 2), (9, 11), (0, n)):
            pl, pb = eng.frame_transforms(first, count, frame=frame)
            assert pl.shape == (count, 6) and pb.shape == (count,)
            assert pl.tobytes() == full_l[first:first + count].tobytes(), (first, count)
            assert pb.tobytes() == full_b[first:first + count].tobytes(), (first, count)
        ol, none = eng.frame_transforms(3, 29, frame=frame, body=False)
        assert none is None and ol.tobytes() == full_l[3:32].tobytes()
        none, ob_ = eng.frame_transforms(3, 29, frame=frame, legs=False)
        assert none is None and ob_.tobytes() == full_b[3:32].tobytes()
        el, eb = eng.frame_transforms(5, 0, frame=frame)
        assert el.shape == (0, 6) and eb.shape == (0,)
        sentinel = -12345.678
        for first, count in ((0, n), (7, 13)):
            lbuf = torch.full(((count * 6 + 3) * 42,), sentinel, dtype=torch.float64, device="cuda")
            bbuf = torch.full(((count + 3) * 20,), sentinel, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            assert eng.frame_transforms(first, count, frame=frame, out_legs=lbuf.data_ptr(), out_body=bbuf.data_ptr()) is None
            eng.synchronize()
            hl, hb = lbuf.cpu().numpy(), bbuf.cpu().numpy()
            assert hl[:count * 6 * 42].tobytes() == full_l[first:first + count].tobytes() and (hl[count * 6 * 42:] == sentinel).all()
            assert hb[:count * 20].tobytes() == full_b[first:first + count].tobytes() and (hb[count * 20:] == sentinel).all()
            lbuf.fill_(sentinel)
            torch.cuda.synchronize()
            assert eng.frame_transforms(first, count, frame=frame, out_legs=lbuf.data_ptr()) is None   # legs only, on the device
            eng.synchronize()
            assert lbuf.cpu().numpy()[:count * 6 * 42].tobytes() == full_l[first:first + count].tobytes()
    full_l, full_b = eng.frame_transforms()
    lib, h = eng.L, eng.h
    la, ba = np.zeros((n, 6), dtype=LEG_FRAMES_DTYPE), np.zeros(n, dtype=BODY_FRAMES_DTYPE)
    lp, bp = la.ctypes.data_as(C.c_void_p), ba.ctypes.data_as(C.c_void_p)
    call = lib.shc_engine_get_frame_transforms
    assert call(h, 0, n, 0, None, None, 0) == SHC_ERR_INVALID_ARG
    assert call(h, -1, 2, 0, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert call(h, 1, n, 0, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert call(h, 0, -1, 0, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert call(h, n + 1, 0, 0, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert call(h, 0, n, 2, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert call(h, 0, n, -1, lp, bp, 0) == SHC_ERR_INVALID_ARG
    assert not la.view(np.float64).any() and not ba.view(np.float64).any()   # a refused call writes nothing
    assert call(h, 0, n, 0, lp, bp, 0) == 0 and la.tobytes() == full_l.tobytes() and ba.tobytes() == full_b.tobytes()
    eng.resident_begin(ring_depth=4, max_cycles=50)
    try:
        assert call(h, 0, n, 0, lp, bp, 0) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    again_l, again_b = eng.frame_transforms()   # served again once resident mode has ended
    assert again_l.shape == (n, 6) and again_b.shape == (n,)
    eng.close()


def test_split_stream_batch_read_right_after_step(Engine):
    """Test 6, last part: 41 000 hexapods (steps run as two launches on two streams); one call into device buffers right after step, no join
    by the caller.  Every robot's tip position against model_tip_position and desired velocity against get_body_state; the robots at both
    ends and on both sides of the split against the numpy reading."""
    import torch
    p = default_hexapod_params("ripple")
    n, cycles = 41000, 25
    rng = np.random.default_rng(233)
    eng = Engine(p, n)
    eng.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
    eng.set_joint_effort(np.zeros((n, 18)))
    lbuf = torch.zeros(n * 6 * 42, dtype=torch.float64, device="cuda")
    bbuf = torch.zeros(n * 20, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(cycles):
        eng.step(1)
    eng.frame_transforms(out_legs=lbuf.data_ptr(), out_body=bbuf.data_ptr())
    eng.synchronize()
    lf = lbuf.cpu().numpy().view(LEG_FRAMES_DTYPE).reshape(n, 6)
    bf = bbuf.cpu().numpy().view(BODY_FRAMES_DTYPE).reshape(n)
    np.testing.assert_allclose(lf["tip"][..., :3], eng.leg_state_msgs()["model_tip_position"], rtol=0, atol=1e-12)
    pose, vel, _ = eng.body_state()
    assert np.array_equal(bf["desired_velocity"], vel) and np.abs(vel).max() > 0
    pick = np.unique(np.concatenate([np.arange(40), np.arange(n // 2 - 40, n // 2 + 40), np.arange(n - 40, n), rng.choice(n, 96, replace=False)]))
    q = eng.joints()[0]
    stats = {}
    compared, n_near = check_legs_against_numpy(lf[pick], p, q[pick], "split-stream batch", stats)
    assert n_near < NEAR_CAP * compared
    want = fn.body_frames(eng.odometry()[pick], pose[pick], vel[pick])
    for name in ("odom_to_base_link", "base_link_to_walk_plane", "pose_euler"):
        assert np.abs(bf[name][pick] - want[name]).max() <= TOL_BODY, name
    eng.close()


def test_reading_does_not_disturb_the_run(Engine):
    """Test 7: the state records and the aux blobs are identical before and after a read (both frames, host and device form), and a run with
    a read after every cycle ends byte-identical to a run without reads."""
    import torch
    n = 23
    p, a = posed_turning_hexapods(Engine, n, 239, 40)
    _, b = posed_turning_hexapods(Engine, n, 239, 40)
    a.synchronize()
    before, aux = state_bytes(a), a.get_aux_state()
    lbuf = torch.zeros(n * 6 * 42, dtype=torch.float64, device="cuda")
    bbuf = torch.zeros(n * 20, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a.frame_transforms()
    a.frame_transforms(frame="odom_ideal")
    a.frame_transforms(2, 9, out_legs=lbuf.data_ptr(), out_body=bbuf.data_ptr())
    a.synchronize()
    assert state_bytes(a) == before and a.get_aux_state() == aux
    for c in range(120):
        a.step(1)
        b.step(1)
        a.frame_transforms(frame=c % 2)
    for e in (a, b):
        e.synchronize()
    assert state_bytes(a) == state_bytes(b)
    assert a.get_aux_state() == b.get_aux_state()
    for x, y in zip(a.joints(), b.joints()):
        assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


def test_fleet_records_in_caller_order(Engine):
    """Test 8: hexapods (6 x 3) and octopods (8 x 5) interleaved in one fleet on one device: records arrive in the caller's instance order,
    each robot's rows are its part engine's, and leg records [6, 8) of the hexapods are all zero."""
    from syropod_highlevel_controller_amd.fleet import MixedFleet
    morphs = [default_hexapod_params("tripod"), synthetic_octopod_params("ripple", 5, 8)]
    n = 29
    mid = (np.arange(n) % 3 == 1).astype(np.int32)
    rng = np.random.default_rng(241)
    fleet = MixedFleet(morphs, mid)
    assert (fleet.max_legs, fleet.max_dof) == (8, 5)
    fleet.set_velocity(rng.uniform(-0.7, 0.7, size=(n, 2)), rng.uniform(-1, 1, size=n))
    fleet.set_joint_effort(np.zeros((n, 8, 5)))
    fleet.step(45)
    fleet.synchronize()
    for frame in ("base_link", "odom_ideal"):
        lf, bf = fleet.frame_transforms(frame=frame)
        assert lf.shape == (n, 8) and bf.shape == (n,)
        only_l, none = fleet.frame_transforms(frame=frame, body=False)
        assert none is None and only_l.tobytes() == lf.tobytes()
        none, only_b = fleet.frame_transforms(frame=frame, legs=False)
        assert none is None and only_b.tobytes() == bf.tobytes()
        seen = np.zeros(n, dtype=bool)
        for handle, m, _, ids in fleet.parts():
            pl, pb = BatchEngine.view(handle, morphs[m], len(ids)).frame_transforms(frame=frame)
            L = morphs[m].leg_count
            assert pl.shape == (len(ids), L) and (mid[ids] == m).all()
            assert lf[ids, :L].tobytes() == pl.tobytes() and bf[ids].tobytes() == pb.tobytes()
            assert lf[ids, L:].tobytes() == bytes(len(ids) * (8 - L) * 336)
            assert np.abs(pl["tip"]).max() > 0 and np.abs(pb["odom_to_base_link"][:, :2]).max() > 0
            seen[ids] = True
        assert seen.all()
    fleet.close()
