"""StateController::publishFrameTransforms (state_controller.cpp:963-1047) restated in numpy from the reference alone, for the tests of
BatchEngine.frame_transforms.  Nothing here comes from the package's csrc or from oracle/: the inputs are what the existing getters return
(joints(), body pose, odometry, desired velocity) and the DH / base constants of the Params.

  Leg::applyFK (model.cpp:945-972)      joint k's transform = createDHMatrix of its reference link with theta + the angle of the joint that
                                        actuates that link (standard_includes.h:466-474); joint 1 hangs off the base link (angle 0)
  Joint / Tip::getPoseRobotFrame        Pose::Identity().transform(product of those matrices from the base) (model.h:594-608, :674-688)
  Pose::transform(Matrix4d)             position = the matrix's translation; rotation = (Quaterniond(R) * identity).normalized() (pose.h:135-146),
                                        Quaterniond(Matrix3d) being Eigen 3.3's trace method with its branch order
  joint rotation                        joint_robot_frame.rotation_ * AngleAxisd(desired_position_, UnitZ()) (state_controller.cpp:1023-1024)
  Pose::addPose / operator~             pose.h:167-173 / :112-115, rotating as Eigen's QuaternionBase::_transformVector does
  quaternionToEulerAngles               standard_includes.h:248-291 on Eigen 3.3's eulerAngles(2, 1, 0)

All functions take a leading batch axis.  Poses are (x, y, z, qw, qx, qy, qz)."""
import numpy as np

FRAME_JOINTS = 5
BRANCH_EPS = 1e-6   # a rotation matrix this close to a branch boundary of the matrix-to-quaternion may come out with the other sign


def dh_matrix(d, theta, r, alpha):
    """createDHMatrix (standard_includes.h:466-474); theta may be an array (n,): returns (n, 4, 4)."""
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    m = np.zeros(theta.shape + (4, 4))
    ct, st, ca, sa = np.cos(theta), np.sin(theta), np.cos(alpha), np.sin(alpha)
    m[:, 0] = np.stack([ct, -st * ca, st * sa, r * ct], axis=-1)
    m[:, 1] = np.stack([st, ct * ca, -ct * sa, r * st], axis=-1)
    m[:, 2] = np.array([0.0, sa, ca, d])
    m[:, 3] = np.array([0.0, 0.0, 0.0, 1.0])
    return m


def quat_from_matrix(R):
    """Eigen 3.3 Quaterniond(Matrix3d) (Shoemake's trace method), R (n, 3, 3) -> (n, 4) as w x y z."""
    R = np.asarray(R, dtype=np.float64)
    out = np.zeros((R.shape[0], 4))
    for n, m in enumerate(R):
        t = m[0, 0] + m[1, 1] + m[2, 2]
        if t > 0.0:
            t = np.sqrt(t + 1.0)
            w = 0.5 * t
            t = 0.5 / t
            out[n] = (w, (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t)
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
            q = [0.0, 0.0, 0.0]
            q[i] = 0.5 * t
            t = 0.5 / t
            w = (m[k, j] - m[j, k]) * t
            q[j] = (m[j, i] + m[i, j]) * t
            q[k] = (m[k, i] + m[i, k]) * t
            out[n] = (w, q[0], q[1], q[2])
    return out


def near_branch_boundary(R, eps=BRANCH_EPS):
    """True where R lies within eps of a branch boundary of quat_from_matrix: trace = 0, or - on the trace <= 0 side - a tie between the two
    largest diagonal entries."""
    R = np.asarray(R, dtype=np.float64)
    d = np.sort(np.diagonal(R, axis1=-2, axis2=-1), axis=-1)
    t = d.sum(axis=-1)
    return (np.abs(t) < eps) | ((t < eps) & (d[..., 2] - d[..., 1] < eps))


def quat_normalized(q):
    return q / np.sqrt((q * q).sum(axis=-1, keepdims=True))


def quat_mul(a, b):
    aw, ax, ay, az = np.moveaxis(np.asarray(a, dtype=np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, dtype=np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], axis=-1)


def quat_conj(q):
    return np.asarray(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def quat_rotate(q, v):
    """QuaternionBase::_transformVector: v + 2 w (u x v) + u x (2 u x v)."""
    q, v = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64)
    u = q[..., 1:]
    uv = 2.0 * np.cross(u, v)
    return v + q[..., :1] * uv + np.cross(u, uv)


def quat_to_matrix(q):
    """QuaternionBase::toRotationMatrix."""
    w, x, y, z = np.moveaxis(np.asarray(q, dtype=np.float64), -1, 0)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    m = np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)], axis=-1)
    return m.reshape(m.shape[:-1] + (3, 3))


def add_pose(a, b):
    """Pose::addPose (pose.h:167-173): a.addPose(b)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.concatenate([a[..., :3] + quat_rotate(a[..., 3:], b[..., :3]), quat_mul(a[..., 3:], b[..., 3:])], axis=-1)


def inverse_pose(a):
    """Pose::operator~ (pose.h:112-115)."""
    a = np.asarray(a, dtype=np.float64)
    c = quat_conj(a[..., 3:])
    return np.concatenate([quat_rotate(c, -a[..., :3]), c], axis=-1)


def quat_to_euler(q):
    """quaternionToEulerAngles(q, intrinsic = false) (standard_includes.h:248-291): Eigen 3.3's eulerAngles(2, 1, 0) of the rotation matrix,
    the reference's flip fix-up, returned as (roll, pitch, yaw)."""
    m = quat_to_matrix(q)
    out = np.zeros(m.shape[:-2] + (3,))
    for idx in np.ndindex(*m.shape[:-2]):
        c = m[idx]
        r0 = np.arctan2(c[1, 0], c[0, 0])          # i = 2, j = 1, k = 0, odd permutation
        c2 = np.sqrt(c[2, 2] * c[2, 2] + c[2, 1] * c[2, 1])
        if r0 < 0.0:
            r0 += np.pi
            r1 = np.arctan2(-c[2, 0], -c2)
        else:
            r1 = np.arctan2(-c[2, 0], c2)
        s1, c1 = np.sin(r0), np.cos(r0)
        r2 = np.arctan2(s1 * c[0, 2] - c1 * c[1, 2], c1 * c[1, 1] - s1 * c[0, 1])
        if abs(r1) > np.pi / 2 or abs(r2) > np.pi / 2:   # "flipped" (:270-289)
            r0 -= np.pi
            if r1 > np.pi / 2.0:
                r1 = -r1 + np.pi
            elif r1 < np.pi / 2.0:
                r1 = -r1 - np.pi
            if r2 > np.pi / 2.0:
                r2 -= np.pi
            elif r2 < np.pi / 2.0:
                r2 += np.pi
        out[idx] = (r2, r1, r0)
    return out


def pose_of_transform(T):
    """Pose::Identity().transform(T) (pose.h:135-146), T (n, 4, 4) -> (n, 7)."""
    return np.concatenate([T[:, :3, 3], quat_normalized(quat_from_matrix(T[:, :3, :3]))], axis=-1)


def leg_frames(p, leg, q):
    """The children of base_link leg `leg` contributes (state_controller.cpp:1009-1046) for desired joint positions q (n, dof of this leg):
    (joint (n, dof, 7), tip (n, 7), near (n, dof + 1) - whether the frame's rotation matrix lies near a branch boundary, tip last)."""
    q = np.asarray(q, dtype=np.float64)
    n, dof = q.shape
    assert dof == p.leg_dof[leg]
    base = p.link[leg][0]
    T = dh_matrix(base.d, np.zeros(n) + base.theta, base.r, base.alpha)   # joint 1: the base link's DH matrix
    joint, near = np.zeros((n, dof, 7)), np.zeros((n, dof + 1), dtype=bool)
    for k in range(dof):
        f = pose_of_transform(T)
        near[:, k] = near_branch_boundary(T[:, :3, :3])
        half = 0.5 * q[:, k]
        aa = np.stack([np.cos(half), np.zeros(n), np.zeros(n), np.sin(half)], axis=-1)   # Quaterniond(AngleAxisd(q, UnitZ))
        joint[:, k] = np.concatenate([f[:, :3], quat_mul(f[:, 3:], aa)], axis=-1)
        lk = p.link[leg][k + 1]
        T = T @ dh_matrix(lk.d, lk.theta + q[:, k], lk.r, lk.alpha)
    near[:, dof] = near_branch_boundary(T[:, :3, :3])
    return joint, pose_of_transform(T), near


def robot_frames(p, q):
    """Every leg of every robot: q (n, legs * longest DOF) as BatchEngine.joints() returns it -> (joint (n, legs, FRAME_JOINTS, 7) with the
    slots past a leg's own DOF zero, tip (n, legs, 7), near (n, legs, FRAME_JOINTS + 1) with the tip last)."""
    L = p.leg_count
    D = max(p.leg_dof[l] for l in range(L))
    q = np.asarray(q, dtype=np.float64).reshape(-1, L, D)
    n = q.shape[0]
    joint, tip, near = np.zeros((n, L, FRAME_JOINTS, 7)), np.zeros((n, L, 7)), np.zeros((n, L, FRAME_JOINTS + 1), dtype=bool)
    for l in range(L):
        d = p.leg_dof[l]
        j, t, nr = leg_frames(p, l, q[:, l, :d])
        joint[:, l, :d], tip[:, l] = j, t
        near[:, l, :d], near[:, l, FRAME_JOINTS] = nr[:, :d], nr[:, d]
    return joint, tip, near


def body_frames(odometry, pose, velocity):
    """The per-robot record from get_odometry / get_body_state outputs (n, 7), (n, 7), (n, 3): a dict with the fields of BodyFrames."""
    pose = np.asarray(pose, dtype=np.float64)
    return {"odom_to_base_link": add_pose(odometry, pose), "base_link_to_walk_plane": inverse_pose(pose),
            "pose_euler": quat_to_euler(pose[..., 3:]), "desired_velocity": np.asarray(velocity, dtype=np.float64)}
