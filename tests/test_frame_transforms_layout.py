"""The record layout behind BatchEngine.frame_transforms (no GPU): the numpy dtypes follow params.LegFrames / BodyFrames, which follow the
header; the entry points are declared and exported; and tests/frames_numpy.py - the numpy reading of publishFrameTransforms the GPU tests
compare against - agrees with scipy's Rotation on every rotation as a rotation."""
import ctypes as C

import numpy as np

import frames_numpy as fn
from syropod_highlevel_controller_amd import engine, synthetic_octopod_params
from syropod_highlevel_controller_amd.params import SHC_FRAME_JOINTS, BodyFrames, LegFrames, LinkParams


def header_fields(struct):
    """(name, shape) of every member of `struct` in the header, in declaration order."""
    fields = engine.HEADER.structs[struct]
    assert all(typ == "double" for typ, _, _ in fields)
    return [(name, dims) for _, name, dims in fields]


def ctypes_shape(typ):
    shape = []
    while typ is not C.c_double:
        shape.append(typ._length_)
        typ = typ._type_
    return tuple(shape)


def test_ctypes_mirrors_match_the_header():
    legs, body = header_fields("shc_leg_frames"), header_fields("shc_body_frames")
    assert legs == [("joint", (SHC_FRAME_JOINTS, 7)), ("tip", (7,))]
    assert [(n, ctypes_shape(t)) for n, t in LegFrames._fields_] == legs
    assert [(n, ctypes_shape(t)) for n, t in BodyFrames._fields_] == body
    assert [n for n, _ in body] == ["odom_to_base_link", "base_link_to_walk_plane", "pose_euler", "desired_velocity"]
    assert C.sizeof(LegFrames) == 336 == 8 * 42 == 8 * sum(int(np.prod(s)) for _, s in legs)     # 42 doubles, no padding
    assert C.sizeof(BodyFrames) == 160 == 8 * 20 == 8 * sum(int(np.prod(s)) for _, s in body)    # 20 doubles, no padding
    offset = 0
    for struct, fields in ((LegFrames, legs), (BodyFrames, body)):
        offset = 0
        for name, shape in fields:
            assert getattr(struct, name).offset == offset, name
            offset += 8 * int(np.prod(shape))


def test_numpy_dtypes_follow_the_ctypes_mirrors():
    for struct, dt in ((LegFrames, engine.LEG_FRAMES_DTYPE), (BodyFrames, engine.BODY_FRAMES_DTYPE)):
        assert dt.itemsize == C.sizeof(struct)
        assert list(dt.names) == [n for n, _ in struct._fields_]
        for name, typ in struct._fields_:
            sub, offset = dt.fields[name][:2]
            assert offset == getattr(struct, name).offset, name
            assert sub.base == np.float64 and sub.shape == ctypes_shape(typ), name
    rec = LegFrames()
    rec.joint[4][6], rec.joint[1][0], rec.tip[3] = 1.5, -2.0, 0.25
    a = np.frombuffer(bytes(rec), dtype=engine.LEG_FRAMES_DTYPE)
    assert a["joint"][0, 4, 6] == 1.5 and a["joint"][0, 1, 0] == -2.0 and a["tip"][0, 3] == 0.25
    assert np.frombuffer(bytes(rec), dtype=np.float64)[7 * 4 + 6] == 1.5
    b = BodyFrames()
    b.pose_euler[2], b.desired_velocity[0] = 0.5, -1.0
    assert np.frombuffer(bytes(b), dtype=np.float64)[16] == 0.5 and np.frombuffer(bytes(b), dtype=engine.BODY_FRAMES_DTYPE)["desired_velocity"][0, 0] == -1.0


def test_new_entry_points_are_declared_and_exported():
    for sym in ("shc_engine_get_frame_transforms", "shc_fleet_get_frame_transforms"):
        assert engine.HEADER.functions[sym][0] == "int" and sym in engine.EXPORTED_SYMBOLS
        assert hasattr(engine.lib(), sym)
    assert engine.HEADER.constants["SHC_FRAME_BASE_LINK"] == 0 and engine.HEADER.constants["SHC_FRAME_ODOM_IDEAL"] == 1
    assert engine.FRAME_IDS == {"base_link": 0, "odom_ideal": 1}
    assert engine.lib().shc_abi_version() == 6


def as_scipy(q_wxyz):
    from scipy.spatial.transform import Rotation
    q = np.asarray(q_wxyz)
    return Rotation.from_quat(np.concatenate([q[..., 1:], q[..., :1]], axis=-1))


def test_numpy_reading_agrees_with_scipy_on_random_chains():
    """Random DH chains (every link constant and joint angle random, so every branch of the matrix-to-quaternion is taken): each frame's
    rotation is the rotation scipy composes from the same DH factors, its position the chain's translation; the quaternions are unit."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(7)
    p = synthetic_octopod_params("ripple", 5, 8)
    for l in range(8):
        for k in range(6):
            p.link[l][k] = LinkParams(rng.uniform(-0.1, 0.1), rng.uniform(-np.pi, np.pi), rng.uniform(0.0, 0.2), rng.uniform(-np.pi, np.pi))
    n = 40
    q = rng.uniform(-np.pi, np.pi, size=(n, 8 * 5))
    joint, tip, near = fn.robot_frames(p, q)
    assert joint.shape == (n, 8, 5, 7) and tip.shape == (n, 8, 7) and near.shape == (n, 8, 6)
    branches = set()
    for l in range(8):
        def dh(lk, theta):
            rot = Rotation.from_euler("z", theta) * Rotation.from_euler("x", lk.alpha)
            return rot, np.stack([lk.r * np.cos(theta), lk.r * np.sin(theta), np.full_like(theta, lk.d)], axis=-1)
        rot, pos = dh(p.link[l][0], np.full(n, p.link[l][0].theta))
        for k in range(6):
            got = joint[:, l, k] if k < 5 else tip[:, l]
            np.testing.assert_allclose(np.linalg.norm(got[:, 3:], axis=-1), 1.0, rtol=0, atol=1e-14)
            want = rot * Rotation.from_euler("z", q[:, l * 5 + k]) if k < 5 else rot
            assert (want.inv() * as_scipy(got[:, 3:])).magnitude().max() < 1e-12, (l, k)
            np.testing.assert_allclose(got[:, :3], pos, rtol=0, atol=1e-14)
            m = rot.as_matrix()
            branches |= set(np.where(np.trace(m, axis1=1, axis2=2) > 0, 3, np.argmax(np.diagonal(m, axis1=1, axis2=2), axis=1)).tolist())
            if k < 5:
                step_rot, step_pos = dh(p.link[l][k + 1], p.link[l][k + 1].theta + q[:, l * 5 + k])
                pos = pos + rot.apply(step_pos)
                rot = rot * step_rot
    assert branches == {0, 1, 2, 3}


def test_numpy_pose_algebra_agrees_with_scipy():
    """addPose, operator~ and quaternionToEulerAngles of random poses against scipy: compositions as rotations + vectors, the Euler angles by
    rebuilding the rotation from them (roll, pitch, yaw = extrinsic x, y, z)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(11)
    n = 500
    def poses():
        q = rng.normal(size=(n, 4))
        return np.concatenate([rng.uniform(-2, 2, size=(n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1)
    a, b = poses(), poses()
    ab = fn.add_pose(a, b)
    ra, rb = as_scipy(a[:, 3:]), as_scipy(b[:, 3:])
    np.testing.assert_allclose(ab[:, :3], a[:, :3] + ra.apply(b[:, :3]), rtol=0, atol=1e-13)
    assert ((ra * rb).inv() * as_scipy(ab[:, 3:])).magnitude().max() < 1e-12
    inv = fn.inverse_pose(a)
    np.testing.assert_allclose(fn.add_pose(a, inv)[:, :3], 0.0, atol=1e-13)
    assert (ra * as_scipy(inv[:, 3:])).magnitude().max() < 1e-12
    e = fn.quat_to_euler(a[:, 3:])
    assert (ra.inv() * Rotation.from_euler("xyz", e)).magnitude().max() < 1e-9
    small = Rotation.from_euler("xyz", rng.uniform(-0.3, 0.3, size=(n, 3)))   # the posing range: the angles themselves come back
    qs = small.as_quat()
    np.testing.assert_allclose(fn.quat_to_euler(np.concatenate([qs[:, 3:], qs[:, :3]], axis=1)), small.as_euler("xyz"), rtol=0, atol=1e-12)
