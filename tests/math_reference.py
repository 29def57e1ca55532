"""The 50-digit reference for the device math primitives (csrc/shc_math.hpp, the grouped forms of shc_cycle.hpp), the cases they
are tested on, and the checks - shared by test_math_primitives.py (host half of tests/math_probe.hip, the oracle) and
test_gpu_math_primitives.py (device half), so both sides face the same cases and the same bounds.

Every op is restated in mpmath at mp.dps = 50 and evaluated on exactly the doubles the probe receives.
  * ops with a mathematical definition are written from it: sin / cos, the rotation a quaternion represents (R(q) v), the
    solution of A x = b (mp LU), the Bernstein sums, a / |a|, conj(q) / |q|^2 ...
  * ops whose convention is the contract are written from the algorithm, in exact arithmetic with the double thresholds the
    reference compares against: Eigen 3.3's eulerAngles + the reference's flip fix-up (standard_includes.h:248-291), Shoemake's
    trace method (Eigen's Quaterniond(Matrix3d)), Eigen's slerp with its 1 - eps threshold, FromTwoVectors.
A reference function takes the inputs as mpf and returns (outputs, branch signature, amplitude):
  * branch signature: the decisions the algorithm took (None when it has none).  When the signature changes under a move of
    any one input by +-KNIFE_ULPS ulp, a correctly rounded implementation may take either branch: the case is a knife edge.
  * amplitude: the size of the largest intermediate of a cancelling sum (|a| |b| for a product that may cancel), so that the
    rounding of intermediates is in the scale even where the result is small.

Where the numbers of the checks come from (none is taken from the code under test):
  stated   a bound the product's own comment states: sincos_joint (shc_math.hpp), fast_rcp / fast_rsqrt (<= 1 ulp).
  derived  |got - ref|_inf <= k * scale, scale = max(condition, ulp(max(|ref|_inf, amplitude))), where condition is the largest
           change of the mp reference's own output when one input moves by one ulp, and k is the number of roundings on the
           longest path through the op (table K below; a transcendental counts with its OpenCL full-profile bound, the public
           bound that covers both libm and ocml: sin / cos / acos 4, atan2 6, sqrt and division 1).  spd_solve: kappa(A) eps |x|.
  rotation at a knife edge: the result represents the same rotation as the reference's to the derived tolerance, and the range
           promises that do not depend on the branch hold.
  pin      exact values where the reference's text decides (each cites its line).
"""
import math
from collections import namedtuple

import numpy as np
from mpmath import mp, mpf

mp.dps = 50
PI = mp.pi
KPI = mpf(math.pi)          # the double M_PI the reference compares against
EPS = 2.0 ** -52
KNIFE_ULPS = 4
KDLS = 0.02                 # model.h:19 (shc::kDls)

# check: "compare" | "rotation" | "pin" | "underflow" (angle_axis_vector: |v|^2 underflows) | "window" (from_two_vectors, c in [-1, -1 + 1e-12)) | "stated"
Case = namedtuple("Case", "edge x check")


def ulp(x):
    x = abs(float(x))
    return math.ulp(x) if math.isfinite(x) else float("inf")


def nxt(x, n=1):
    """the double n ulps above (n < 0: below) x"""
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


SQH = math.sqrt(0.5)        # the double nearest sqrt(1/2)

# ------------------------------------------------------------------------------------------------ mp building blocks


def m_dot(a, b):
    return sum((x * y for x, y in zip(a, b)), mpf(0))


def m_norm(a):
    return mp.sqrt(m_dot(a, a))


def m_cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def m_qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def m_matrix(q):
    """q (x) q^* as a matrix: the rotation of q when |q| = 1; Eigen's toRotationMatrix for any q (it does not normalise)"""
    w, x, y, z = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def m_rotate(q, v):
    """Eigen's _transformVector: v + 2 w (u x v) + 2 u x (u x v), = R(q) v for |q| = 1 and toRotationMatrix(q) v for any q"""
    m = m_matrix(q)
    return [m_dot(m[i], v) for i in range(3)]


def m_euler_matrix(e, intrinsic):
    def rx(a):
        return mp.matrix([[1, 0, 0], [0, mp.cos(a), -mp.sin(a)], [0, mp.sin(a), mp.cos(a)]])

    def ry(a):
        return mp.matrix([[mp.cos(a), 0, mp.sin(a)], [0, 1, 0], [-mp.sin(a), 0, mp.cos(a)]])

    def rz(a):
        return mp.matrix([[mp.cos(a), -mp.sin(a), 0], [mp.sin(a), mp.cos(a), 0], [0, 0, 1]])
    return rx(e[0]) * ry(e[1]) * rz(e[2]) if intrinsic else rz(e[2]) * ry(e[1]) * rx(e[0])


# ------------------------------------------------------------------------------------------------ the reference ops


def r_sincos(x):
    return [mp.sin(x[0]), mp.cos(x[0])], None, 0


def r_euler_to_quat(intrinsic):
    def f(e):
        qx = [mp.cos(e[0] / 2), mp.sin(e[0] / 2), 0, 0]
        qy = [mp.cos(e[1] / 2), 0, mp.sin(e[1] / 2), 0]
        qz = [mp.cos(e[2] / 2), 0, 0, mp.sin(e[2] / 2)]
        return (m_qmul(m_qmul(qx, qy), qz) if intrinsic else m_qmul(m_qmul(qz, qy), qx)), None, 1
    return f


def r_quat_to_euler(intrinsic):
    """Eigen 3.3 eulerAngles(0,1,2) / (2,1,0) on toRotationMatrix(q), then the reference's fix-up (standard_includes.h:270-289)."""
    def f(q):
        m = m_matrix(q)
        if intrinsic:   # i, j, k = 0, 1, 2 (even)
            r0 = mp.atan2(m[1][2], m[2][2])
            c2 = mp.sqrt(m[0][0] ** 2 + m[0][1] ** 2)
            first = r0 > 0
            if first:
                r0 -= KPI
                r1 = mp.atan2(-m[0][2], -c2)
            else:
                r1 = mp.atan2(-m[0][2], c2)
            s1, c1 = mp.sin(r0), mp.cos(r0)
            r2 = mp.atan2(s1 * m[2][0] - c1 * m[1][0], c1 * m[1][1] - s1 * m[2][1])
            r0, r1, r2 = -r0, -r1, -r2
        else:           # i, j, k = 2, 1, 0 (odd)
            r0 = mp.atan2(m[1][0], m[0][0])
            c2 = mp.sqrt(m[2][2] ** 2 + m[2][1] ** 2)
            first = r0 < 0
            if first:
                r0 += KPI
                r1 = mp.atan2(-m[2][0], -c2)
            else:
                r1 = mp.atan2(-m[2][0], c2)
            s1, c1 = mp.sin(r0), mp.cos(r0)
            r2 = mp.atan2(s1 * m[0][2] - c1 * m[1][2], c1 * m[1][1] - s1 * m[0][1])
        h = KPI / 2
        sig = (first, abs(r1) > h, abs(r2) > h, r1 > h, r1 < h, r2 > h, r2 < h)
        if sig[1] or sig[2]:
            r0 -= KPI
            if r1 > h:
                r1 = -r1 + KPI
            elif r1 < h:
                r1 = -r1 - KPI
            if r2 > h:
                r2 -= KPI
            elif r2 < h:
                r2 += KPI
        return ([r0, r1, r2] if intrinsic else [r2, r1, r0]), sig, 4
    return f


def m_normalized(a):
    z = m_dot(a, a)
    return [c / mp.sqrt(z) for c in a] if z > 0 else list(a)


def r_from_two_vectors(x):
    """Eigen 3.3 FromTwoVectors on the normalised inputs; inside the anti-parallel window the axis is not part of the contract
    (Eigen: an SVD null vector; the product and the oracle: fixed orthogonal axes), so only w is returned there."""
    v0, v1 = m_normalized(x[:3]), m_normalized(x[3:])
    c = m_dot(v1, v0)
    if c < mpf(-1.0) + mpf(1e-12):
        c = max(c, mpf(-1))
        w2 = (1 + c) / 2
        return [mp.sqrt(w2), mpf("nan"), mpf("nan"), mpf("nan")], ("window",), 1
    ax = m_cross(v0, v1)
    s = mp.sqrt((1 + c) * 2)
    # the one cancelling sum is 1 + c: c carries the absolute rounding of a three-term dot product of unit vectors, so s^2 = 2 (1 + c) is off
    # by eps / (1 + c) relatively and so is every component of the result - the amplitude 1 / (1 + c) puts ulp(1) / (1 + c) into the scale
    return [s / 2] + [a / s for a in ax], ("plain",), 1 / (1 + c)


def r_quat_from_matrix(m):
    """Shoemake's trace method as Eigen's Quaterniond(Matrix3d) writes it."""
    t = m[0] + m[4] + m[8]
    q = [None] * 3
    if t > 0:
        t = mp.sqrt(t + 1)
        w = t / 2
        t = mpf(0.5) / t
        q = [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t]
        sig = ("trace",)
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 4]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1)
        q[i] = t / 2
        t = mpf(0.5) / t
        w = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
        sig = ("diag", i)
    return [w] + q, sig, 2


def r_angle_axis_vector(q):
    """AngleAxisd(q).axis() * angle(): angle = 2 atan2(|v|, |w|), axis = v / |v| with the sign of w (w = -0.0 counts as >= 0)."""
    n = m_norm(q[1:])
    if n == 0:
        return [mpf(0)] * 3, ("zero",), 0
    ang = 2 * mp.atan2(n, abs(q[0]))
    if q[0] < 0:
        n = -n
    return [c / n * ang for c in q[1:]], ("w<0" if q[0] < 0 else "w>=0",), 0


def m_slerp(a, t, b):
    one = mpf(1.0 - 2.220446049250313e-16)
    d = m_dot(a, b)
    ad = abs(d)
    if ad >= one:
        s0, s1, br = 1 - t, t, "lerp"
    else:
        th = mp.acos(ad)
        s0, s1, br = mp.sin((1 - t) * th) / mp.sin(th), mp.sin(t * th) / mp.sin(th), "slerp"
    if d < 0:
        s1 = -s1
    return [s0 * x + s1 * y for x, y in zip(a, b)], (br, d < 0), abs(s0) * max(map(abs, a)) + abs(s1) * max(map(abs, b))


def r_slerp(x):
    return m_slerp(x[:4], x[4], x[5:])


def r_normalized(x):
    return m_normalized(x), (m_dot(x, x) > 0,), 0


def r_inverse(q):
    n2 = m_dot(q, q)
    return ([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2] if n2 > 0 else [mpf(0)] * 4), (n2 > 0,), 0


def r_rotate(x):
    q, v = x[:4], x[4:]
    return m_rotate(q, v), None, (1 + 2 * m_dot(q, q)) * max(map(abs, v))


def r_correct_rotation(x):
    t, r = x[:4], x[4:]
    neg = m_dot(t, r) < 0
    return [-c if neg else c for c in t], (neg,), 0


def m_pose_amp(a, b):
    return max(map(abs, a[:3])) + (1 + 2 * m_dot(a[3:], a[3:])) * max(map(abs, b[:3])) + 1


def r_add_pose(x):
    a, b = x[:7], x[7:]
    return [p + r for p, r in zip(a[:3], m_rotate(a[3:], b[:3]))] + m_qmul(a[3:], b[3:]), None, m_pose_amp(a, b)


def r_remove_pose(x):
    a, b = x[:7], x[7:]
    inv = r_inverse(b[3:])[0]
    return ([p + r for p, r in zip(a[:3], m_rotate(a[3:], [-c for c in b[:3]]))] + m_qmul(a[3:], inv)), None, \
        m_pose_amp(a, b) + max(map(abs, inv)) * max(map(abs, a[3:]))


def r_interpolate_pose(x):
    a, c, t = x[:7], x[7], x[8:]
    q, sig, amp = m_slerp(a[3:], c, t[3:])
    return [tp * c + ap * (1 - c) for ap, tp in zip(a[:3], t[:3])] + q, sig, amp + max(map(abs, a[:3])) + max(map(abs, t[:3]))


def r_inverse_transform_vector(x):
    a, v = x[:7], x[7:]
    qc = [a[3], -a[4], -a[5], -a[6]]
    d = [vi - pi for vi, pi in zip(v, a[:3])]
    return m_rotate(qc, d), None, (1 + 2 * m_dot(qc, qc)) * (max(map(abs, v)) + max(map(abs, a[:3])))


def r_projection(x):
    a, b = x[:3], x[3:]
    if m_dot(a, a) == 0 or m_dot(b, b) == 0:
        return [mpf(0)] * 3, ("zero",), 0
    return [c * (m_dot(a, b) / m_dot(b, b)) for c in b], ("plain",), m_norm(a)


def r_rejection(x):
    p, sig, amp = r_projection(x)
    return [a - c for a, c in zip(x[:3], p)], sig, max(amp, max(map(abs, x[:3])))


def r_smooth_step(x):
    c = x[0]
    return [6 * c ** 5 - 15 * c ** 4 + 10 * c ** 3], None, 6 * abs(c) ** 5 + 15 * c ** 4 + 10 * abs(c) ** 3


def c_int(x):
    return int(math.trunc(x))          # C's double -> int conversion truncates towards zero


def c_rem(a, b):
    return int(math.fmod(a, b))        # C's % takes the sign of the dividend


def r_round_to_int(x):                 # standard_includes.h:93
    v = float(x[0])
    return [mpf(c_int(v + 0.5) if v >= 0 else -c_int(0.5 - v))], None, 0


def r_round_to_even_int(x):            # standard_includes.h:98 (int(x) % 2 is -1 for negative odd values: they round UP to the even above)
    i = c_int(float(x[0]))
    return [mpf(i if c_rem(i, 2) == 0 else i + 1)], None, 0


def r_mod_i(x):                        # standard_includes.h:76
    a, b = c_int(float(x[0])), c_int(float(x[1]))
    return [mpf(c_rem(c_rem(a, b) + b, b))], None, 0


def r_signd(x):                        # standard_includes.h:88: sign(0) = -1
    return [mpf(1 if x[0] > 0 else -1)], None, 0


def r_clampd(x):                       # standard_includes.h:109
    return [max(x[1], min(x[0], x[2]))], None, 0


def r_quartic_bezier(x):
    p, t = [x[3 * i:3 * i + 3] for i in range(5)], x[15]
    s = 1 - t
    b = [s ** 4, 4 * t * s ** 3, 6 * t * t * s * s, 4 * t ** 3 * s, t ** 4]
    return [sum(b[i] * p[i][a] for i in range(5)) for a in range(3)], None, sum(abs(b[i]) * max(map(abs, p[i])) for i in range(5))


def r_quartic_bezier_dot(x):
    p, t = [x[3 * i:3 * i + 3] for i in range(5)], x[15]
    s = 1 - t
    b = [4 * s ** 3, 12 * s * s * t, 12 * s * t * t, 4 * t ** 3]
    return [sum(b[i] * (p[i + 1][a] - p[i][a]) for i in range(4)) for a in range(3)], None, \
        sum(abs(b[i]) * (max(map(abs, p[i])) + max(map(abs, p[i + 1]))) for i in range(4))


def r_rcp(x):
    return [1 / x[0]], None, 0


def r_rsqrt(x):
    return [1 / mp.sqrt(x[0])], None, 0


def r_spd(n):
    def f(x):
        a = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                a[i, j] = x[i * n + j]
        return list(mp.lu_solve(a, mp.matrix(x[n * n:]))), None, 0
    return f


def spd_kappa(x, n):
    a = mp.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):          # the product reads the lower triangle only
            a[i, j] = a[j, i] = mpf(x[i * n + j])
    ev = mp.eigsy(a, eigvals_only=True)
    return max(ev) / min(ev)


def r_tip_rotation_delta(x):
    q, sig, _ = r_from_two_vectors(x)
    if sig == ("window",):
        return [mpf("nan")] * 3, sig, 0
    out, s2, _ = r_angle_axis_vector(m_normalized(q))
    return out, sig + s2, 4 * r_from_two_vectors(x)[2]      # the angle-axis vector is up to pi long


# op name -> (reference, k, where the k roundings are).  The count follows the longest dependent path of the product's form; sums of
# n products count n (each product and each partial sum rounds, the fused forms round less).
K = {
    "sincos_joint_reduce": (r_sincos, None, "stated bound"),
    "sincos_joint_noreduce": (r_sincos, None, "stated bound (1 ulp: no reduction error)"),
    "euler_to_quat_extrinsic": (r_euler_to_quat(False), 12, "half angle 0 + sincos_joint 2 (1 ulp each of sin, cos) + two quaternion products 5 each (4 products + 3 sums, norm-wise 5)"),
    "euler_to_quat_intrinsic": (r_euler_to_quat(True), 12, "as extrinsic"),
    "quat_to_euler_extrinsic": (r_quat_to_euler(False), 24, "matrix entry 4 + atan2 6 + sincos_joint 1 + s1 m - c1 m 3 + atan2 6 + +-pi 1, fix-up 2, result 1"),
    "quat_to_euler_intrinsic": (r_quat_to_euler(True), 24, "as extrinsic"),
    "from_two_vectors": (r_from_two_vectors, 14, "normalized 5 (dot 3, sqrt 1, division 1) + dot 3 + (1 + c) 2 2 + sqrt 1 + reciprocal 1 + product 1, cross 2 in parallel"),
    "quat_from_matrix": (r_quat_from_matrix, 8, "trace 2 + 1 + sqrt 1 + 0.5 / t 1 + difference 1 + product 1, result 1"),
    "angle_axis_vector": (r_angle_axis_vector, 14, "norm 4 (3 products / sums + sqrt) + atan2 6 + doubling 0 + division 1 + product 1, result 2"),
    "slerp": (r_slerp, 22, "dot 4 + acos 4 + t theta 2 + sin 4 + sin theta 4 (parallel) + division 1 + two products and a sum 3, result 4"),
    "normalized_v3": (r_normalized, 5, "dot 3 + sqrt 1 + division 1"),
    "normalized_quat": (r_normalized, 6, "dot 4 + sqrt 1 + division 1"),
    "inverse": (r_inverse, 5, "dot 4 + division 1"),
    "rotate": (r_rotate, 10, "cross 2 + doubling 0 + cross 2 + scale 1 + two sums 2, amplitude-wise 3 more for the cancelling cross terms"),
    "correct_rotation": (r_correct_rotation, 0, "sign only: exact"),
    "add_pose": (r_add_pose, 11, "rotate 10 + sum 1; quaternion product 5 in parallel"),
    "remove_pose": (r_remove_pose, 11, "rotate 10 + sum 1; inverse 5 + product 5 in parallel"),
    "interpolate_pose": (r_interpolate_pose, 22, "slerp 22; the lerp 4 in parallel"),
    "inverse_transform_vector": (r_inverse_transform_vector, 11, "difference 1 + rotate 10"),
    "projection": (r_projection, 8, "dot 3 + dot 3 (parallel) + division 1 + product 1, result 3"),
    "rejection": (r_rejection, 9, "projection 8 + difference 1"),
    "smooth_step": (r_smooth_step, 8, "c^3 2 + Horner 4 + product 1, result 1"),
    "round_to_int": (r_round_to_int, 0, "pin"),
    "round_to_even_int": (r_round_to_even_int, 0, "pin"),
    "mod_i": (r_mod_i, 0, "pin"),
    "signd": (r_signd, 0, "pin"),
    "clampd": (r_clampd, 0, "selection only: exact"),
    "quartic_bezier": (r_quartic_bezier, 12, "1 - t 1 + Bernstein weight 4 + product 1 + four sums 4, result 2"),
    "quartic_bezier_dot": (r_quartic_bezier_dot, 10, "1 - t 1 + weight 3 + node difference 1 (parallel) + three fused steps 3, result 2"),
    "fast_rcp": (r_rcp, None, "stated bound"),
    "fast_rsqrt": (r_rsqrt, None, "stated bound"),
    "tip_rotation_delta": (r_tip_rotation_delta, 34, "from_two_vectors 14 + normalized 6 + angle_axis_vector 14"),
}
for _n in range(3, 7):
    # LDL^T without pivoting on an SPD matrix is backward stable with a constant of the order n (Higham, Accuracy and Stability of
    # Numerical Algorithms, Thm 10.3/10.4: |dA| <= gamma_{3n+1} |R^T||R|): forward error <= (3n + 1) kappa(A) eps |x| to first order; the
    # reciprocal-multiply form adds one rounding per pivot use (n more).
    for _form in ("fast", "exact"):
        K[f"spd_solve{_n}_{_form}"] = (r_spd(_n), 4 * _n + 1, "backward-stable LDL^T: 3n + 1 (Higham Thm 10.3) + n reciprocal-multiplies; times kappa(A) eps |x|")

DEVICE_ONLY = ("fast_rcp", "fast_rsqrt") + tuple(f"spd_solve{n}_fast" for n in range(3, 7))

# ------------------------------------------------------------------------------------------------ evaluation + checks


def evaluate(op, x):
    """(ref outputs as mpf, signature, scale, knife): scale and knife from one-ulp / KNIFE_ULPS-ulp moves of each input."""
    f = K[op][0]
    xm = [mpf(v) for v in x]
    out, sig, amp = f(xm)
    if K[op][1] is None or K[op][1] == 0:
        return out, sig, 0.0, False
    if op.startswith("spd_solve"):
        n = int(op[9])
        xn = max(abs(o) for o in out)
        return out, sig, float(spd_kappa(x, n) * EPS * xn), False
    fin = [o for o in out if mp.isfinite(o)]
    cond = mpf(0)
    knife = False
    for j, v in enumerate(x):
        if not math.isfinite(v):
            continue
        for step in (1, -1, KNIFE_ULPS, -KNIFE_ULPS):
            y = list(xm)
            y[j] = mpf(nxt(v, step))
            o2, s2, _ = f(y)
            if s2 != sig:
                knife = True
            elif abs(step) == 1:
                for a, b in zip(out, o2):
                    if mp.isfinite(a) and mp.isfinite(b):
                        cond = max(cond, abs(a - b))
    mag = max([abs(o) for o in fin] + [mpf(amp)])
    return out, sig, max(float(cond), ulp(mag)), knife


def euler_rotation_error(op, x, got):
    """largest entry of R(got angles) - toRotationMatrix(q): zero when the triple represents the rotation of q"""
    intrinsic = op.endswith("intrinsic")
    m = m_matrix([mpf(v) for v in x])
    r = m_euler_matrix([mpf(float(g)) for g in got], intrinsic)
    return max(abs(r[i, j] - m[i][j]) for i in range(3) for j in range(3))


def sincos_bound(x, ref, reduce):
    """shc_math.hpp: |error| <= |n| 2^-87 + 1 ulp(result), n = rint(x 2 / pi); the REDUCE = false form has n = 0."""
    n = abs(int(mp.nint(mpf(x) * 2 / PI))) if reduce else 0
    return [n * 2.0 ** -87 + ulp(r) for r in ref]


def check_case(op, case, got, allow_pin_tolerance=False):
    """-> (ok, error in units of the case's tolerance (or ulps for stated bounds), message).  got: the outputs as doubles."""
    x, check = case.x, case.check
    ref, sig, scale, knife = evaluate(op, x)
    k = K[op][1]
    got = [float(g) for g in got]
    if check == "pin":
        ok = all((math.isnan(g) and mp.isnan(r)) or g == float(r) for g, r in zip(got, ref))      # (-0 == +0: the sign of a zero is not pinned)
        return ok, 0.0 if ok else float("inf"), f"pin: got {got}, the reference's text gives {[float(r) for r in ref]}"
    if check == "underflow":    # the product's |v|^2 underflows: exactly 0 (named difference from Eigen's stableNorm path), never anything else
        ok = all(g == 0.0 for g in got)
        return ok, 0.0 if ok else float("inf"), f"underflow: got {got}, expected exact zeros (the reference would give {[float(r) for r in ref]})"
    if check == "stated":
        if op.startswith("sincos"):
            b = sincos_bound(x[0], ref, op.endswith("_reduce"))
            errs = [abs(mpf(g) - r) / bb for g, r, bb in zip(got, ref, b)]
            e = float(max(errs))
            return e <= 1.0, e, f"sincos_joint({x[0]!r}): error {e:.3g} x the stated bound |n| 2^-87 + 1 ulp"
        e = float(abs(mpf(got[0]) - ref[0]) / ulp(ref[0]))
        return e <= 1.0, e, f"{op}({x[0]!r}) is {e:.3g} ulp from the mp value (stated: <= 1 ulp)"
    if check == "window":       # from_two_vectors with c in [-1, -1 + 1e-12): unit result, and rotate(q, a^) lands within 2 (pi - 2 acos(w)) of b^
        a, b = m_normalized([mpf(v) for v in x[:3]]), m_normalized([mpf(v) for v in x[3:]])
        q = [mpf(g) for g in got]
        unit = abs(m_norm(q) - 1)
        ra = m_rotate(q, a)
        ang = mp.atan2(m_norm(m_cross(ra, b)), m_dot(ra, b))
        # both rotate(q, a^) and b^ lie pi - theta from -a^ (theta = 2 acos(w) = acos(c)), in possibly different planes through a^: at most
        # twice that apart.  Rounding: w = sqrt((1 + c) / 2) carries the absolute error of c (~4 eps) through the square root.
        bound = 2 * (PI - 2 * mp.acos(ref[0])) + 2 * mp.sqrt(16 * EPS)
        ok = unit <= 8 * EPS and ang <= bound
        return ok, float(ang / bound), f"window: |q| - 1 = {float(unit):.3g}, angle(rotate(q, a), b) = {float(ang):.3g} (bound {float(bound):.3g})"
    tol = k * scale
    if check == "rotation":
        if op.startswith("quat_to_euler"):
            # tolerance: the triple's own rounding (k ulp of its largest angle, <= 3 pi / 2) seen through the rotation matrix (entries are
            # 1-Lipschitz in each angle, three angles) + the matrix entries' rounding of the unnormalised q
            e = euler_rotation_error(op, x, got)
            t = 3 * k * ulp(4.8) + 4 * EPS * float(m_dot([mpf(v) for v in x], [mpf(v) for v in x]))
            rng = all(abs(g) <= 1.5 * math.pi + k * ulp(4.8) for g in got)      # what the fix-up can return at most: 3 pi / 2
            return (e <= t and rng), float(e / t), f"rotation: matrix differs by {float(e):.3g} (tolerance {t:.3g}), range ok = {rng}"
        d = min(max(abs(mpf(g) - r) for g, r in zip(got, ref)), max(abs(mpf(g) + r) for g, r in zip(got, ref)))
        t = tol if not knife else max(tol, k * ulp(max(abs(r) for r in ref)))
        return d <= t, float(d / t) if t else float(d), f"rotation: +-q differs by {float(d):.3g} (tolerance {t:.3g})"
    # compare
    errs = [abs(mpf(g) - r) for g, r in zip(got, ref) if not (mp.isnan(r) and math.isnan(g))]
    if any(mp.isnan(r) != math.isnan(g) for g, r in zip(got, ref)):
        return False, float("inf"), f"NaN pattern differs: got {got}, reference {[float(r) for r in ref]}"
    e = max(errs) if errs else mpf(0)
    if tol == 0:
        return e == 0, 0.0 if e == 0 else float("inf"), f"exact op: got {got}, reference {[float(r) for r in ref]}"
    return e <= tol, float(e / tol), f"compare: error {float(e):.3g}, tolerance k * scale = {k} * {scale:.3g}"


def max_ulps(op, case, got):
    """the error of `got` in ulps of the reference's largest output (what DESIGN.md tabulates); None where there is no finite reference"""
    ref = K[op][0]([mpf(v) for v in case.x])[0]
    fin = [(abs(mpf(float(g)) - r), r) for g, r in zip(got, ref) if mp.isfinite(r) and math.isfinite(float(g))]
    if not fin or case.check in ("rotation", "window"):
        return None
    mag = max(abs(r) for _, r in fin)
    return float(max(e for e, _ in fin) / ulp(mag)) if mag > 0 else 0.0


# ------------------------------------------------------------------------------------------------ cases


def _rq(rng):
    q = rng.normal(size=4)
    return (q / np.linalg.norm(q)).tolist()


def _qe(e, intrinsic=False):
    """the double quaternion of an Euler triple (inputs for the quat_to_euler edges)"""
    return [float(c) for c in r_euler_to_quat(intrinsic)([mpf(v) for v in e])[0]]


def sincos_cases(reduce):
    out = []
    if reduce:
        for k in range(-16, 17):
            for name, step in (("pi/4", math.pi / 4), ("pi/2", math.pi / 2)):
                c = float(mpf(k) * (PI / 4 if name == "pi/4" else PI / 2))
                for d in (-2, -1, 0, 1, 2):
                    out.append(Case(f"double nearest {k} {name} {d:+d} ulp", [nxt(c, d)], "stated"))
        for k in (1, 3, 5, 7, 9, 21):       # rint ties of x 2 / pi: x = (k / 2) (pi / 2) and its neighbours
            c = float(mpf(k) / 2 * PI / 2)
            out += [Case(f"rint tie {k}/2 {d:+d} ulp", [s * nxt(c, d)], "stated") for d in (-1, 0, 1) for s in (1, -1)]
        rng = np.random.default_rng(11)
        out += [Case("random [-7, 7]", [float(v)], "stated") for v in rng.uniform(-7, 7, 400)]
        out += [Case("random [-100, 100]", [float(v)], "stated") for v in rng.uniform(-100, 100, 200)]
    else:
        q = math.pi / 4
        out += [Case(f"+-pi/4 boundary {d:+d} ulp", [s * nxt(q, d)], "stated") for d in (-2, -1, 0) for s in (1, -1)]
        rng = np.random.default_rng(12)
        out += [Case("random [-pi/4, pi/4]", [float(v)], "stated") for v in rng.uniform(-q, q, 400)]
    for v, name in ((0.0, "+0"), (-0.0, "-0"), (5e-324, "smallest denormal"), (-5e-324, "-smallest denormal"), (1e-310, "denormal"),
                    (2.0 ** -27, "2^-27"), (-2.0 ** -27, "-2^-27"), (2.0 ** -1022, "2^-1022"), (-2.0 ** -1022, "-2^-1022")):
        out.append(Case(name, [v], "stated"))
    return out


def quat_to_euler_cases(intrinsic):
    """Hand-written edges first (each names its edge and its check), then seeded random unit quaternions (check decided by evaluate)."""
    h, u = math.pi / 2, math.ulp(math.pi / 2)
    out = [Case("(sqrt 1/2, 0, sqrt 1/2, 0): pitch pi/2 through the rounding of m00 / m22" + ("" if intrinsic else ": the -3 pi / 2 pin"),
                [SQH, 0.0, SQH, 0.0], "rotation"),
           Case("(sqrt 1/2, 0, -sqrt 1/2, 0): pitch -pi/2", [SQH, 0.0, -SQH, 0.0], "rotation")]
    for s in (1, -1):
        for d in (-2, -1, 0, 1, 2):
            out.append(Case(f"pitch {s:+d} pi/2 {d:+d} ulp (gimbal lock)", _qe([0.0, s * (h + d * u), 0.0], intrinsic), "rotation"))
            out.append(Case(f"pitch {s:+d} pi/2 {d:+d} ulp with yaw 0.3, roll -0.2", _qe([-0.2, s * (h + d * u), 0.3], intrinsic), "rotation"))
    for axis, name in ((2, "yaw"), (0, "roll")):
        for a, an in ((0.0, "0"), (h, "pi/2"), (-h, "-pi/2"), (math.pi, "pi"), (-math.pi, "-pi"), (nxt(math.pi, -1), "pi - ulp"), (nxt(-math.pi, 1), "-pi + ulp")):
            e = [0.0, 0.0, 0.0]
            e[axis] = a
            out.append(Case(f"{name} = {an} alone (first-angle fold)", _qe(e, intrinsic), "rotation"))
            e[1] = 0.4
            e[2 - axis] = -0.7
            if (name, an) == ("roll", "-pi/2") and not intrinsic:
                continue    # pinned on its own (test_math_primitives.py): r2 lands on M_PI / 2 exactly under a flip and neither arm of the fix-up takes it
            out.append(Case(f"{name} = {an} with pitch 0.4", _qe(e, intrinsic), "rotation"))
    # m10 = 2 (x y + z w) = +-0 with m00 = 1 - 2 (y^2 + z^2) of either sign
    out += [Case("m10 = +0, m00 > 0 (identity)", [1.0, 0.0, 0.0, 0.0], "compare"),
            Case("m10 = -0, m00 > 0", [1.0, 0.0, 0.0, -0.0], "compare"),
            Case("m10 = +0, m00 < 0 (half turn about y)", [0.0, 0.0, 1.0, 0.0], "rotation"),
            Case("m10 = -0, m00 < 0", [-0.0, 0.0, 1.0, 0.0], "rotation"),
            Case("m10 = +0, m00 < 0 (half turn about z)", [0.0, 0.0, 0.0, 1.0], "rotation"),
            Case("m10 = -0, m00 < 0 (half turn about z)", [-0.0, 0.0, 0.0, 1.0], "rotation"),
            Case("m10 = -denormal, m00 = 1", [1.0, 0.0, 0.0, -2.5e-324 * 2], "compare"),
            Case("m10 = -denormal, m00 in (0, 1)", [0.8, 0.0, 0.6, -1e-320], "rotation"),
            Case("zero quaternion (matrix = identity)", [0.0, 0.0, 0.0, 0.0], "compare")]
    rng = np.random.default_rng(21)
    for i in range(6):
        q = _rq(rng)
        out.append(Case(f"generic q #{i}", q, "compare"))
        out.append(Case(f"-q of generic #{i}", [-c for c in q], "compare"))
        out.append(Case(f"generic #{i} scaled by 1 + 1e-8", [c * (1 + 1e-8) for c in q], "compare"))
        out.append(Case(f"generic #{i} scaled by 1 - 1e-8", [c * (1 - 1e-8) for c in q], "compare"))
    return out


def random_cases(op, n=150):
    """seeded random draws in the ranges the walking path uses them in; check = None: decided by evaluate (compare, or rotation at a knife edge)"""
    rng = np.random.default_rng(abs(hash_name(op)) % (2 ** 32))
    out = []
    for _ in range(n):
        if op.startswith("quat_to_euler"):
            x = _rq(rng)
        elif op.startswith("euler_to_quat"):
            x = rng.uniform(-math.pi, math.pi, 3).tolist()
        elif op in ("from_two_vectors", "tip_rotation_delta", "projection", "rejection"):
            x = (rng.normal(size=6) * 10.0 ** rng.integers(-3, 3)).tolist()
        elif op == "quat_from_matrix":
            x = [float(v) for row in m_matrix([mpf(c) for c in _rq(rng)]) for v in row]
        elif op in ("angle_axis_vector", "normalized_quat", "inverse"):
            x = _rq(rng) if op == "angle_axis_vector" else rng.normal(size=4).tolist()
        elif op == "slerp":
            x = _rq(rng) + [float(rng.uniform(0, 1))] + _rq(rng)
        elif op == "normalized_v3":
            x = rng.normal(size=3).tolist()
        elif op == "rotate":
            x = _rq(rng) + rng.normal(size=3).tolist()
        elif op == "correct_rotation":
            x = _rq(rng) + _rq(rng)
        elif op in ("add_pose", "remove_pose"):
            x = rng.normal(size=3).tolist() + _rq(rng) + rng.normal(size=3).tolist() + _rq(rng)
        elif op == "interpolate_pose":
            x = rng.normal(size=3).tolist() + _rq(rng) + [float(rng.uniform(0, 1))] + rng.normal(size=3).tolist() + _rq(rng)
        elif op == "inverse_transform_vector":
            x = rng.normal(size=3).tolist() + _rq(rng) + rng.normal(size=3).tolist()
        elif op == "smooth_step":
            x = [float(rng.uniform(0, 1))]
        elif op in ("quartic_bezier", "quartic_bezier_dot"):
            x = rng.normal(size=15).tolist() + [float(rng.uniform(0, 1))]
        elif op == "clampd":
            lo = float(rng.normal())
            x = [float(rng.normal()), lo, lo + float(rng.uniform(0, 2))]
        else:
            raise KeyError(op)
        out.append(Case("random", x, None))
    return out


def hash_name(s):
    return int.from_bytes(s.encode(), "little") % 1000003       # a seed per op that does not depend on PYTHONHASHSEED


def _unit(v):
    n = math.sqrt(sum(c * c for c in v))
    return [c / n for c in v]


def from_two_vectors_cases():
    g = _unit([0.3, -0.5, 0.8])
    out = [Case("parallel, same length", [0.0, 0.0, 1.0, 0.0, 0.0, 1.0], "compare"),
           Case("parallel, generic direction, lengths 2 and 5", [2 * c for c in g] + [5 * c for c in g], "compare"),
           Case("zero vector first: (sqrt 1/2, 0, 0, 0) (Eigen normalized() leaves 0, c = 0, axis 0)", [0.0, 0.0, 0.0, 0.0, 0.0, 1.0], "pin"),
           Case("zero vector second", [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], "pin"),
           Case("both zero", [0.0] * 6, "pin"),
           Case("lengths 1e-150 and 1e150", [1e-150 * c for c in _unit([1, 2, 2])] + [1e150 * c for c in _unit([-2, 1, 2])], "compare"),
           Case("lengths 1e150 and 1e-150", [1e150 * c for c in _unit([1, 2, 2])] + [1e-150 * c for c in _unit([2, 1, -2])], "compare")]
    for i, name in enumerate("xyz"):
        a = [0.0, 0.0, 0.0]
        a[i] = 1.0
        out.append(Case(f"exactly anti-parallel along {name}", a + [-c for c in a], "window"))
        out.append(Case(f"exactly anti-parallel along -{name}, lengths 3 and 0.5", [-3 * c for c in a] + [0.5 * c for c in a], "window"))
    out.append(Case("anti-parallel along a generic direction", g + [-c for c in g], "window"))
    # c = -cos(d) ~ -1 + d^2 / 2: the window's edge 1e-12 is d = sqrt(2e-12) = 1.414e-6
    for d, name, check in ((1e-7, "c + 1 = 5e-15: inside the window", "window"), (1.2e-6, "c + 1 = 7.2e-13: inside", "window"),
                           (1.40e-6, "c + 1 = 9.8e-13: just inside", "window"), (1.43e-6, "c + 1 = 1.02e-12: just outside", "compare"),
                           (1e-5, "c + 1 = 5e-11: outside", "compare")):
        b = [-(g[0] * math.cos(d) + 0.0), -g[1] * math.cos(d), -g[2] * math.cos(d)]
        o = _unit([g[1], -g[0], 0.0])       # orthogonal to g
        b = [bi + math.sin(d) * oi for bi, oi in zip(b, o)]
        out.append(Case(name, g + b, check))
    return out


def quat_from_matrix_cases():
    def mat(q):
        return [float(v) for row in m_matrix([mpf(c) for c in q]) for v in row]
    out = []
    # trace = 0 exactly: rotation by 2 pi / 3 ... the trace is 1 + 2 cos(angle): angle = 2 pi / 3 about z gives diag (-1/2, -1/2, 1)
    out.append(Case("trace exactly 0 (diag -1/2, -1/2, 1)", [-0.5, -math.sqrt(0.75), 0.0, math.sqrt(0.75), -0.5, 0.0, 0.0, 0.0, 1.0], "rotation"))
    out.append(Case("trace +ulp", [nxt(-0.5, 1), -math.sqrt(0.75), 0.0, math.sqrt(0.75), -0.5, 0.0, 0.0, 0.0, 1.0], "rotation"))
    out.append(Case("trace -ulp", [nxt(-0.5, -1), -math.sqrt(0.75), 0.0, math.sqrt(0.75), -0.5, 0.0, 0.0, 0.0, 1.0], "rotation"))
    for ax, name in (([1, 0, 0], "x"), ([0, 1, 0], "y"), ([0, 0, 1], "z")):
        out.append(Case(f"180 degrees about {name}", mat([0.0] + [float(c) for c in ax]), "rotation"))
    out.append(Case("180 degrees about (1, 1, 0) / sqrt 2 (diagonal tie m[4] == m[0])", mat([0.0, SQH, SQH, 0.0]), "rotation"))
    out.append(Case("180 degrees about (1, 1, 1) / sqrt 3 (both diagonal ties)", [-1 / 3, 2 / 3, 2 / 3, 2 / 3, -1 / 3, 2 / 3, 2 / 3, 2 / 3, -1 / 3], "rotation"))
    out.append(Case("180 degrees about (0, 1, 1) / sqrt 2 (tie m[8] == m[4])", mat([0.0, 0.0, SQH, SQH]), "rotation"))
    out.append(Case("identity", mat([1.0, 0.0, 0.0, 0.0]), "compare"))
    # chain frames of legs with alpha = +-pi/2 (chain_frame_pose: R1 [X Y Z] after DH steps whose sin alpha / cos alpha are the doubles of +-pi/2)
    for sa_sign in (1, -1):
        for yaw, q1, q2 in ((0.0, 0.0, 0.0), (math.pi / 3, 0.4, -0.9), (-2.6, -0.7, 1.3), (math.pi, 0.0, math.pi / 2)):
            out.append(Case(f"chain frame, alpha = {sa_sign:+d} pi/2, base yaw {yaw:.3g}, q = ({q1}, {q2})", _chain_matrix(yaw, [q1, q2], sa_sign * math.pi / 2), "rotation"))
    return out


def _chain_matrix(yaw, qs, alpha):
    """the matrix chain_frame_pose hands to quat_from_matrix, built the way fk does in doubles: Rz(yaw) then per link Rz(q) Rx(alpha)"""
    def rz(a):
        return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])

    def rx(a):
        return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    m = rz(yaw)
    for q in qs:
        m = m @ rz(q) @ rx(alpha)
    return [float(v) for v in m.reshape(-1)]


def slerp_cases():
    rng = np.random.default_rng(31)
    a = _rq(rng)
    out = []
    one = 1.0 - 2.220446049250313e-16

    def b_with_dot(d):
        """a unit b with a . b = d (to rounding): d a + sqrt(1 - d^2) o, o orthogonal to a"""
        o = np.array([-a[1], a[0], -a[3], a[2]])
        return (d * np.array(a) + math.sqrt(max(0.0, 1 - d * d)) * o).tolist()
    for t in (0.0, 1.0, 0.5, 1e-17):
        out.append(Case(f"d = 1 (b = a), t = {t}", a + [t] + a, "rotation"))
        out.append(Case(f"d = -1 (b = -a), t = {t}", a + [t] + [-c for c in a], "rotation"))
        for s in (1, -1):
            out.append(Case(f"d = {s:+d}(1 - eps) region (angle 2.1e-8), t = {t}", a + [t] + b_with_dot(s * math.cos(2.1e-8)), "rotation"))
            out.append(Case(f"d = {s:+d} just below 1 - eps (angle 3e-8), t = {t}", a + [t] + b_with_dot(s * math.cos(3e-8)), "rotation"))
        out.append(Case(f"d = 0, t = {t}", a + [t] + b_with_dot(0.0), "compare"))
        out.append(Case(f"d = -0.6 (the short way), t = {t}", a + [t] + b_with_dot(-0.6), "compare"))
    # exact thresholds on axis-aligned quaternions: a = (1, 0, 0, 0), b = (d, sqrt(1 - d^2), 0, 0): the dot product is exactly d
    for d, name in ((one, "d = 1 - eps exactly"), (nxt(one, -1), "d one ulp below 1 - eps"), (-one, "d = -(1 - eps)"), (nxt(-one, 1), "d one ulp above -(1 - eps)")):
        out.append(Case(name + ", t = 0.5", [1.0, 0.0, 0.0, 0.0, 0.5, d, math.sqrt(1 - d * d), 0.0, 0.0], "rotation"))
    return out


def angle_axis_cases():
    out = [Case("vector part 0, w = 1", [1.0, 0.0, 0.0, 0.0], "compare"), Case("vector part 0, w = -1", [-1.0, 0.0, 0.0, 0.0], "compare"),
           Case("vector part 1e-300: its square underflows, the plain norm is 0 and the result 0, where Eigen's stableNorm fallback gives 2e-300", [1.0, 1e-300, 0.0, 0.0], "underflow"),
           Case("vector part 1e-9", [1.0, 0.0, 1e-9, 0.0], "compare"), Case("vector part 1e-9, w = -1", [-1.0, 0.0, 1e-9, 0.0], "compare"),
           Case("w = -0.0 (counts as w >= 0)", [-0.0, 0.6, 0.0, 0.8], "compare"), Case("w = +0.0", [0.0, 0.6, 0.0, 0.8], "compare"),
           Case("w < 0", [-0.5, 0.5, -0.5, 0.5], "compare"), Case("w > 0", [0.5, 0.5, -0.5, 0.5], "compare")]
    return out


def integer_cases():
    halves = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, 3.0, -3.0, 4.0, -4.0, -3.5, -4.5, -1.0, -2.0, -0.9, 7.9, -7.9, 1e6 + 0.5]
    out = {"round_to_int": [Case(f"x = {v!r}", [v], "pin") for v in halves],
           "round_to_even_int": [Case(f"x = {v!r} (int(x) % 2 is negative for negative odd x)", [v], "pin") for v in halves],
           "mod_i": [Case(f"mod({a}, {b})", [float(a), float(b)], "pin") for a in (-13, -12, -7, -1, 0, 1, 7, 12, 13, 100) for b in (1, 2, 6, 12, 100)],
           "signd": [Case(f"sign({v!r}) (sign(0) = -1, standard_includes.h:88)", [v], "pin") for v in (0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, float("inf"), -float("inf"))],
           "clampd": [Case(n, x, "pin") for n, x in (("inside", [0.3, 0.0, 1.0]), ("below", [-2.0, 0.0, 1.0]), ("above", [2.0, 0.0, 1.0]), ("at lo", [0.0, 0.0, 1.0]),
                                                    ("lo == hi", [5.0, 1.0, 1.0]), ("-0 against +0", [-0.0, 0.0, 1.0]))]}
    return out


def zero_pins():
    return {"normalized_v3": [Case("normalized(0) = 0 (Eigen 3.3 normalized(): unchanged when the squared norm is 0)", [0.0, 0.0, 0.0], "pin"),
                              ],
            "normalized_quat": [Case("normalized(0) = 0", [0.0] * 4, "pin")],
            "inverse": [Case("inverse(0) = 0 (Eigen: zero quaternion stays zero)", [0.0] * 4, "pin")],
            "projection": [Case("a = 0 (standard_includes.h:175)", [0.0, 0.0, 0.0, 1.0, 2.0, 3.0], "pin"), Case("b = 0", [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], "pin")],
            "rejection": [Case("b = 0: a itself", [1.0, 2.0, 3.0, 0.0, 0.0, 0.0], "pin")],
            "smooth_step": [Case("c = 0", [0.0], "pin"), Case("c = 1", [1.0], "compare"), Case("c = 0.5", [0.5], "compare"), Case("c = 1e-200", [1e-200], "compare")],
            "correct_rotation": [Case("dot = 0 exactly: unchanged (< 0 is strict, standard_includes.h:213)", [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], "pin"),
                                 Case("dot < 0: negated", [1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0], "pin")],
            "quartic_bezier": [Case(f"t = {t}", [float(i) for i in range(15)] + [t], "compare") for t in (0.0, 1.0, 0.5)],
            "quartic_bezier_dot": [Case(f"t = {t}", [float(i * i) for i in range(15)] + [t], "compare") for t in (0.0, 1.0, 0.5)]}


def rcp_cases(n_sweep=100000):
    xs, names = [], []
    for v in (4e-4, 1e-3, 1.0, 1e6):
        xs.append(v), names.append(f"{v!r} (lambda^2 ... 1e6)")
    for e in range(-12, 21):
        for d in (-1, 0, 1):
            xs.append(nxt(2.0 ** e, d)), names.append(f"2^{e} {d:+d} ulp")
    rng = np.random.default_rng(41)
    sweep = np.exp(rng.uniform(math.log(4e-4), math.log(1e6), n_sweep))
    return [Case(n, [float(x)], "stated") for n, x in zip(names, xs)] + [Case("log-uniform sweep", [float(x)], "stated") for x in sweep]


def _hexapod_leg_jacobian(q, link=(0.05, 0.15, 0.3)):
    """linear Jacobian of a 3-joint leg (coxa about z, femur / tibia about y-like axes) in doubles, joint angles q: z_i x (p_e - p_i)"""
    c0, s0 = math.cos(q[0]), math.sin(q[0])
    rad = np.array([c0, s0, 0.0])
    z1 = np.array([s0, -c0, 0.0])
    p1 = link[0] * rad
    a1, a2 = q[1], q[1] + q[2]
    p2 = p1 + link[1] * (math.cos(a1) * rad + math.sin(a1) * np.array([0, 0, 1.0]))
    pe = p2 + link[2] * (math.cos(a2) * rad + math.sin(a2) * np.array([0, 0, 1.0]))
    return np.stack([np.cross([0, 0, 1.0], pe), np.cross(z1, pe - p1), np.cross(z1, pe - p2)], axis=1)


def spd_cases(n):
    """A = J^T J + lambda^2 I (lambda = kDls), b = J^T d + lambda^2 g, as the DLS step forms them"""
    rng = np.random.default_rng(50 + n)
    out = []

    def case(name, j, check="compare"):
        a = j.T @ j + KDLS * KDLS * np.eye(n)
        b = j.T @ rng.normal(size=j.shape[0]) * 0.01 + KDLS * KDLS * rng.normal(size=n)
        out.append(Case(name, a.reshape(-1).tolist() + b.tolist(), check))
    pad = np.zeros((3, n))
    j = _hexapod_leg_jacobian([0.3, 0.0, 0.0])      # femur and tibia in line: their columns are parallel (rank 2)
    pad[:, :3] = j
    case("fully stretched leg (rank 2)", pad.copy())
    pad[:] = 0
    pad[:, 0] = pad[:, 1] = pad[:, 2] = [0.0, 0.0, 0.5]
    case("all columns parallel (rank 1)", pad.copy())
    case("J = 0 (A = lambda^2 I)", np.zeros((3, n)))
    case("column scales spread by 1e3", rng.normal(size=(6, n)) * np.logspace(-1.5, 1.5, n))
    for i in range(40):
        case("random J", rng.normal(size=(6 if i % 2 else 3, n)) * 0.3)
    return out


def all_cases(op):
    """every case of one op: hand-written edges, then the seeded random draws"""
    if op.startswith("sincos_joint"):
        return sincos_cases(op.endswith("_reduce"))
    if op.startswith("quat_to_euler"):
        return quat_to_euler_cases(op.endswith("intrinsic")) + random_cases(op)
    if op in ("fast_rcp", "fast_rsqrt"):
        return rcp_cases()
    if op.startswith("spd_solve"):
        return spd_cases(int(op[9]))
    ints = integer_cases()
    if op in ints:
        return ints[op] + (random_cases(op) if op == "clampd" else [])
    edges = {"from_two_vectors": from_two_vectors_cases, "quat_from_matrix": quat_from_matrix_cases, "slerp": slerp_cases,
             "angle_axis_vector": angle_axis_cases}.get(op, lambda: [])()
    if op == "tip_rotation_delta":
        edges = [c for c in from_two_vectors_cases() if c.check == "compare"]
    if op.startswith("euler_to_quat"):
        h = math.pi / 2
        edges = [Case(f"angles {e}", e, "compare") for e in ([0.0, 0.0, 0.0], [0.0, h, 0.0], [0.0, -h, 0.0], [math.pi, 0.0, 0.0], [0.0, 0.0, -math.pi], [h, h, h], [-0.0, 0.0, 1e-300])]
    return edges + zero_pins().get(op, []) + random_cases(op)


def resolve(op, case):
    """a random case (check None) takes compare, or rotation when the mp reference alone finds it on a knife edge; returns (case, used_fallback)"""
    if case.check is not None:
        return case, False
    _, sig, _, knife = evaluate(op, case.x)
    if knife or sig == ("window",):
        return case._replace(check="window" if sig == ("window",) else "rotation"), True
    return case._replace(check="compare"), False


def pack(cases):
    return np.ascontiguousarray([c.x for c in cases], dtype=np.float64)


# the grouped forms: the whole quat_to_euler edge list + cases on the two sides of the `neg` prediction (m10 of either sign, +-0, denormal)
def grouped_quat_cases():
    return [c.x for c in quat_to_euler_cases(False)] + [c.x for c in random_cases("quat_to_euler_extrinsic", 64)]


def grouped_euler_cases():
    return [c.x for c in all_cases("euler_to_quat_extrinsic")]


def neg_predicate(q):
    """the grouped form's prediction of the sign of r0, on the doubles it computes (shc_cycle.hpp): plain double arithmetic, products first"""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    m10 = ty * x + tz * w
    m00 = 1.0 - (ty * y + tz * z)
    return (m10 < 0.0 or (m10 == 0.0 and math.copysign(1, m10) < 0 and math.copysign(1, m00) < 0)), m10, m00
