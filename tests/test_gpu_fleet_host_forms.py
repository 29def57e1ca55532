"""GPU (-m gpu): the fleet's host forms (shc_fleet_set_velocity / _set_imu / _set_pose_input / _set_tip_force / _set_joint_effort and
shc_fleet_get_joint_state / _get_walk_state / _get_leg_state_msgs / _get_frame_transforms / _scan_health) against what they are made of: every
part's own engine, reached through a view, with the translation between the caller's padded order and the part's dense order done in numpy
(array[ids] cut to the part's (legs, dof) on the way in; rows placed at ids with NaN / zero padding on the way out).  The device forms are tested
against the host forms (tests/test_gpu_fleet_device_io.py); this test anchors the host forms themselves.  Every comparison is byte equality.

Fleet: the 46 robots in three bins of tests/test_gpu_fleet_device_io.py - the caller's order differs from every part's, every part ends in a
partly filled wavefront, and two bins are padded in each direction."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd.engine import (BODY_FRAMES_DTYPE, FRAME_IDS, HEALTH_NEAR_LIMIT, LEG_FRAMES_DTYPE, LEG_STATE_MSG_DTYPE, ROBOT_HEALTH_DTYPE,
                                                     SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_OK, BatchEngine, HealthCriteria)
from test_gpu_fleet_device_io import DOF, LEGS, MD, ML, MORPH, N, SENTINEL, host_set, input_set, joint_bytes, make, morphologies, robot_records, views

pytestmark = pytest.mark.gpu
assert len(morphologies()) == 3 and len(MORPH) == N


def part_set(fleet, a):
    """The definition of the host setters: every part's engine is given array[ids], cut to the part's (legs, dof); a missing member is held."""
    for handle, m, _dev, ids in fleet.parts():
        view, L, D = BatchEngine.view(handle, fleet.params[m], len(ids)), LEGS[m], DOF[m]
        rows = lambda k: np.ascontiguousarray(a[k][ids]) if k in a else None
        if "linear_xy" in a or "angular" in a:
            view.set_velocity(rows("linear_xy"), rows("angular"))
        if "imu_orientation_wxyz" in a or "imu_angular_velocity" in a:
            view.set_imu(rows("imu_orientation_wxyz"), rows("imu_angular_velocity"))
        if "pose_translation_velocity" in a or "pose_rotation_velocity" in a:
            view.set_pose_input(rows("pose_translation_velocity"), rows("pose_rotation_velocity"))
        if "tip_force" in a:
            view.set_tip_force(np.ascontiguousarray(a["tip_force"][ids, :L]))
        if "joint_effort" in a:
            view.set_joint_effort(np.ascontiguousarray(a["joint_effort"][ids, :L, :D]))


def assert_same(a, b, what):
    ra, rb = robot_records(a), robot_records(b)
    for i in range(a.n):
        assert ra[i] == rb[i], f"{what}: robot {i} (bin {MORPH[i]}) holds other records after the fleet's host setters than after its part's own"
    sentinel = np.float64(SENTINEL).tobytes()
    assert not any(sentinel in part for rec in ra for part in rec), f"{what}: a padding entry of a per-leg input reached the state"


def test_setters():
    """A through the five host setters, B part by part through the engines' own, and C - first set only - to show that the second set is no no-op
    (velocity, IMU, force and effort inputs are no part of the state record: they show in the cycles that follow)."""
    a, b, c = make(3)
    first = input_set(11)
    host_set(a, first)
    part_set(b, first)
    part_set(c, first)
    assert_same(a, b, "right after the inputs")
    for f in (a, b, c):
        f.step(40)
    assert_same(a, b, "40 cycles later")
    assert joint_bytes(a) == joint_bytes(b) == joint_bytes(c)
    second = input_set(12)
    for held in ("linear_xy", "imu_orientation_wxyz", "pose_translation_velocity", "pose_rotation_velocity", "joint_effort"):
        del second[held]
    host_set(a, second)
    part_set(b, second)
    assert_same(a, b, "after a second set with held members")
    for f in (a, b, c):
        f.step(10)
    assert_same(a, b, "10 cycles after the second set")
    assert joint_bytes(a) == joint_bytes(b)
    assert joint_bytes(c) != joint_bytes(b), "the second input set changed nothing: the comparison above shows nothing"
    assert a.io_nbytes == 0, "a host setter allocated device I/O staging"
    for f in (a, b, c):
        f.close()


def filled(shape, dtype):
    """A host buffer every byte of which is 0xAB."""
    out = np.empty(shape, dtype=dtype)
    out.view(np.uint8).reshape(-1)[:] = 0xAB
    return out


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_get(fleet, frame, crit):
    """The five C entry points, called directly, into buffers of 0xAB bytes."""
    L, h, n = fleet.L, fleet.h, fleet.n
    out = {"q": filled((n, ML, MD), np.float64), "qd": filled((n, ML, MD), np.float64), "walk_state": filled(n, np.int32),
           "leg_state_msgs": filled((n, ML), LEG_STATE_MSG_DTYPE), "leg_frames": filled((n, ML), LEG_FRAMES_DTYPE), "body_frames": filled(n, BODY_FRAMES_DTYPE),
           "health": filled(n, ROBOT_HEALTH_DTYPE)}
    criteria = HealthCriteria(int(crit[0]), 0, float(crit[1]), float(crit[2]))
    assert L.shc_fleet_get_joint_state(h, ptr(out["q"]), ptr(out["qd"])) == SHC_OK
    assert L.shc_fleet_get_walk_state(h, ptr(out["walk_state"])) == SHC_OK
    assert L.shc_fleet_get_leg_state_msgs(h, ptr(out["leg_state_msgs"])) == SHC_OK
    assert L.shc_fleet_get_frame_transforms(h, FRAME_IDS[frame], ptr(out["leg_frames"]), ptr(out["body_frames"])) == SHC_OK
    assert L.shc_fleet_scan_health(h, C.byref(criteria), ptr(out["health"])) == SHC_OK
    return out


def expected(fleet, frame, crit):
    """The same seven arrays from the parts' own getters, placed at ids in numpy: NaN where a bin lacks the leg or joint, zero records for the
    legs it lacks, nothing else."""
    n = fleet.n
    want = {"q": np.full((n, ML, MD), np.nan), "qd": np.full((n, ML, MD), np.nan), "walk_state": np.zeros(n, np.int32),
            "leg_state_msgs": np.zeros((n, ML), LEG_STATE_MSG_DTYPE), "leg_frames": np.zeros((n, ML), LEG_FRAMES_DTYPE), "body_frames": np.zeros(n, BODY_FRAMES_DTYPE),
            "health": np.zeros(n, ROBOT_HEALTH_DTYPE)}
    seen = np.zeros(n, dtype=bool)
    for handle, m, _dev, ids in fleet.parts():
        view, L, D = BatchEngine.view(handle, fleet.params[m], len(ids)), LEGS[m], DOF[m]
        q, qd = view.joints()
        want["q"][ids, :L, :D], want["qd"][ids, :L, :D] = q.reshape(len(ids), L, D), qd.reshape(len(ids), L, D)
        want["walk_state"][ids] = view.body_state()[2]
        want["leg_state_msgs"][ids, :L] = view.leg_state_msgs()
        lf, bf = view.frame_transforms(frame=frame)
        want["leg_frames"][ids, :L], want["body_frames"][ids] = lf, bf
        want["health"][ids] = view.scan_health(*crit)[0]
        seen[ids] = True
    assert seen.all()
    return want


def near_limit_criteria(fleet):
    """NEAR_LIMIT with a threshold between the two middle values of the robots' limit proximities: some robots are flagged, not all."""
    prox = np.unique(fleet.scan_health()["min_limit_proximity"])
    assert len(prox) >= 2
    crit = (HEALTH_NEAR_LIMIT, float(0.5 * (prox[len(prox) // 2 - 1] + prox[len(prox) // 2])), 0.0)
    flagged = (fleet.scan_health(*crit)["flags"] & HEALTH_NEAR_LIMIT) != 0
    assert 0 < flagged.sum() < fleet.n
    return crit


def walked(devices=(0,)):
    (f,) = make(1, devices=devices)
    host_set(f, input_set(13))
    f.step(40)
    return f


def test_getters():
    """Every word of every buffer is written: the rows at their ids, the bits of std::nan("") in the q / qd padding, all-zero records for missing
    legs.  Both frames; health criteria that flag some robots.  The same getters on a fleet whose two device slots name one device (six parts
    instead of three) return the same bytes."""
    a, twice = walked(), walked(devices=(0, 0))
    assert len(a.parts()) == 3 and len(twice.parts()) == 6
    crit = near_limit_criteria(a)
    twice.scan_health()        # (a scan refreshes the derived tips: the same on both fleets)
    twice.scan_health(*crit)
    nan = np.float64(np.nan).tobytes()
    for frame in ("base_link", "odom_ideal"):
        got, want, six = host_get(a, frame, crit), expected(a, frame, crit), host_get(twice, frame, crit)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), f"{k} (frame {frame}) differs from the parts' rows placed at their ids"
            assert got[k].tobytes() == six[k].tobytes(), f"{k} (frame {frame}) differs on the fleet of six parts"
        hexapod = int(np.flatnonzero(MORPH == 0)[0])
        assert got["q"][hexapod, 6:].tobytes() == nan * (2 * MD) and got["q"][hexapod, 0, 3:].tobytes() == nan * 2
        assert not got["leg_state_msgs"][hexapod, 6:].tobytes().strip(b"\0") and not got["leg_frames"][hexapod, 6:].tobytes().strip(b"\0")
    assert a.io_nbytes == 0 and twice.io_nbytes == 0, "a host getter allocated device I/O staging"
    a.close()
    twice.close()


def test_edges():
    """What a NULL argument and a part in resident mode are answered with.  Two things that must not move are NOT observed here and rest on
    reading the code (fleet_inputs_walk of csrc/shc_fleet_io.hpp): that a per-robot host setter given NULLs still joins split steps (only the
    SHC_ERR_BUSY side of entering every part shows from outside), and that the device form skips a setter none of whose members is given."""
    a = walked()
    L, h = a.L, a.h
    arrays = input_set(14)
    q, ws = filled((N, ML, MD), np.float64), filled(N, np.int32)
    health, msgs = filled(N, ROBOT_HEALTH_DTYPE), filled((N, ML), LEG_STATE_MSG_DTYPE)
    # NULL arguments
    before = robot_records(a)
    assert L.shc_fleet_set_velocity(h, None, None) == SHC_OK and L.shc_fleet_set_imu(h, None, None) == SHC_OK
    assert L.shc_fleet_set_pose_input(h, None, None) == SHC_OK
    assert L.shc_fleet_set_tip_force(h, None) == SHC_OK and L.shc_fleet_set_joint_effort(h, None) == SHC_OK
    assert robot_records(a) == before
    assert L.shc_fleet_get_joint_state(h, None, None) == SHC_OK
    assert L.shc_fleet_get_joint_state(h, ptr(q), None) == SHC_OK and q.tobytes() == a.joints()[0].tobytes()
    assert L.shc_fleet_get_frame_transforms(h, 0, None, None) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_get_leg_state_msgs(h, None) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_scan_health(h, None, None) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_get_walk_state(h, None) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_scan_health(h, None, ptr(health)) == SHC_OK          # no criteria: the default thresholds
    assert L.shc_fleet_scan_health(h, C.byref(HealthCriteria(0, 0, 0.0, 0.0)), ptr(health)) == SHC_OK and health.tobytes() == a.scan_health().tobytes()
    lf = filled((N, ML), LEG_FRAMES_DTYPE)
    assert L.shc_fleet_get_frame_transforms(h, 7, ptr(lf), None) == SHC_ERR_INVALID_ARG   # unknown frame
    # a part in resident mode: a per-robot setter enters every part's engine even with nothing to set, a per-leg setter given NULL enters none
    hexapods = views(a)[0][0]
    hexapods.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert L.shc_fleet_set_velocity(h, None, None) == SHC_ERR_BUSY and L.shc_fleet_set_imu(h, None, None) == SHC_ERR_BUSY
        assert L.shc_fleet_set_pose_input(h, None, None) == SHC_ERR_BUSY
        assert L.shc_fleet_set_velocity(h, ptr(arrays["linear_xy"]), ptr(arrays["angular"])) == SHC_ERR_BUSY
        assert L.shc_fleet_set_tip_force(h, None) == SHC_OK and L.shc_fleet_set_joint_effort(h, None) == SHC_OK
        assert L.shc_fleet_set_tip_force(h, ptr(arrays["tip_force"])) == SHC_ERR_BUSY
        assert L.shc_fleet_set_joint_effort(h, ptr(arrays["joint_effort"])) == SHC_ERR_BUSY
        ws[:] = -7
        assert L.shc_fleet_get_joint_state(h, None, None) == SHC_ERR_BUSY
        assert L.shc_fleet_get_walk_state(h, ptr(ws)) == SHC_ERR_BUSY
        assert L.shc_fleet_get_leg_state_msgs(h, ptr(msgs)) == SHC_ERR_BUSY
        assert L.shc_fleet_scan_health(h, None, ptr(health)) == SHC_ERR_BUSY
        assert L.shc_fleet_get_frame_transforms(h, 0, ptr(lf), None) == SHC_ERR_BUSY
        assert (ws == -7).all(), "the part that objects is the first: nothing was written"
    finally:
        hexapods.resident_end()
    assert L.shc_fleet_get_walk_state(h, ptr(ws)) == SHC_OK and ws.tobytes() == a.walk_state().tobytes()
    assert a.io_nbytes == 0
    a.close()
