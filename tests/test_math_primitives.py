"""CPU: every math primitive of csrc/shc_math.hpp called directly - the host (x86) half of tests/math_probe.hip, compiled with the
product's flags - against the 50-digit reference of tests/math_reference.py, on seeded random draws and on the hand-written edges
(the doubles nearest k pi / 2, gimbal lock, the first-angle fold, anti-parallel vectors, Shoemake's branch switches, slerp's 1 - eps
fallback ...).  The oracle's orc_test_* primitives face the same edge lists, so the checker is checked where the product is.
The device half runs the same cases through the same checks in test_gpu_math_primitives.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from mpmath import mpf

import math_reference as R
from oracle_lib import _ptr, lib as oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))


def load_probe(tmp_dir):
    from syropod_highlevel_controller_amd import engine
    so = engine.compile_with_product_flags(os.path.join(HERE, "math_probe.hip"), os.path.join(str(tmp_dir), "libmath_probe.so"))
    P = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    P.shc_probe_op_name.restype = C.c_char_p
    P.shc_probe_op_widths.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    P.shc_probe_run.argtypes = [C.c_int, dp, C.c_int, dp, C.c_int]
    P.shc_probe_run_grouped.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp]
    P.ops = {P.shc_probe_op_name(i).decode(): i for i in range(P.shc_probe_op_count())}
    return P


def run_op(P, op, cases, device):
    """one call (on the device: one launch) over all cases of an op -> (n, nout) doubles"""
    nin, nout = C.c_int(), C.c_int()
    assert P.shc_probe_op_widths(P.ops[op], C.byref(nin), C.byref(nout)) == 0
    x = R.pack(cases)
    assert x.shape == (len(cases), nin.value), (op, x.shape, nin.value)
    out = np.full((len(cases), nout.value), np.nan)
    rc = P.shc_probe_run(P.ops[op], _ptr(x), len(cases), _ptr(out), int(device))
    assert rc == 0, f"shc_probe_run({op}) returned {rc}"
    return out


def check_op(op, cases, got, what):
    """every case through its check; -> (largest error in ulps of the reference, share of random cases on the knife-edge fallback)"""
    fails, worst, fallback, n_random = [], 0.0, 0, 0
    for c, g in zip(cases, got):
        rc, used = R.resolve(op, c)
        n_random += c.check is None
        fallback += used
        ok, err, msg = R.check_case(op, rc, g)
        if not ok:
            fails.append(f"  [{c.edge}] x = {c.x!r}: {msg}")
        u = R.max_ulps(op, rc, g)
        if u is not None and math.isfinite(u):
            worst = max(worst, u)
    assert not fails, f"{what} {op}: {len(fails)} of {len(cases)} cases miss their check\n" + "\n".join(fails[:12])
    return worst, (fallback / n_random if n_random else 0.0)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return load_probe(tmp_path_factory.mktemp("math_probe"))


HOST_OPS = [op for op in R.K if op not in R.DEVICE_ONLY]


def test_probe_exports_every_op(probe):
    assert set(probe.ops) == set(R.K), set(probe.ops) ^ set(R.K)


@pytest.mark.parametrize("op", HOST_OPS)
def test_host_form_against_the_mp_reference(probe, op):
    """sincos_joint_reduce is held to |n| 2^-87 + 1 ulp of the result.  With fn * pio2_1t taken as a plain rounded product the host form was 1.09 x
    that bound off at the doubles within 2 ulp of +-11 pi / 2 (cos(17.278759594743864): 7.7e-26 against 11 * 2^-87 = 7.1e-26), and the device form
    1.21 x at +-12 pi / 4 and +-12 pi / 2 (60 cases: the compiler fused r - w into an fma, after which (r - y) - w is not y's rounding error); the
    reduction now recovers the product's rounding with an fma and keeps contraction off (shc_math.hpp, pio2_reduce)."""
    cases = R.all_cases(op)
    worst, share = check_op(op, cases, run_op(probe, op, cases, device=False), "host")
    print(f"host {op}: {len(cases)} cases, max error {worst:.3g} ulp (k = {R.K[op][1]}), knife-edge fallback on {share:.2%} of the random cases")
    # the representation check may stand in for the component-wise one on at most 1 % of the random cases; the share is the mp reference's alone
    assert share <= 0.01, f"{op}: {share:.2%} of the random cases fall back to the rotation check"


def test_sincos_joint_stated_bound_at_multiples_of_half_pi(probe):
    """|n| 2^-87 + 1 ulp of the result at the doubles nearest k pi / 2 for k = 1, 2, 5, where the reduced argument cancels - and the reason shc_math.hpp no longer says "< 1 ulp": cos(1.5707963267948966) is ~3e5 ulp of its own value off."""
    x = [float(mpf(k) * R.PI / 2) for k in (1, 2, 5)]
    got = run_op(probe, "sincos_joint_reduce", [R.Case("k pi / 2", [v], "stated") for v in x], device=False)
    for v, (s, c), k in zip(x, got, (1, 2, 5)):
        small, ref = (c, R.mp.cos(mpf(v))) if k % 2 else (s, R.mp.sin(mpf(v)))
        err = abs(mpf(small) - ref)
        assert err <= k * 2.0 ** -87 + R.ulp(ref), (v, float(err))
        assert err > R.ulp(ref), "the two-part reduction is within 1 ulp here: the header's bound can be tightened to '< 1 ulp' again"


def test_pitch_of_minus_three_half_pi_is_pinned(probe):
    """quaternionToEulerAngles((sqrt 1/2, 0, sqrt 1/2, 0)) = (0, -3 pi / 2, 0): the same rotation as pitch +pi/2, outside the documented -pi:pi.
    The reference's text decides it: the doubles give m00 = m22 = -2.2e-16, so r0 = pi, r1 = pi/2 - 2.2e-16 (below M_PI / 2) and r2 = pi, the fix-up
    runs for r2 and its `else if (result[1] < M_PI/2.0)` arm (standard_includes.h:277) maps r1 to -r1 - pi.  Product and oracle are faithful to
    it; a clean-up of that arm must fail here."""
    q = [R.SQH, 0.0, R.SQH, 0.0]
    ref = [float(v) for v in R.r_quat_to_euler(False)([mpf(v) for v in q])[0]]
    assert abs(ref[1] + 1.5 * math.pi) < 1e-15 and abs(ref[0]) < 1e-15 and abs(ref[2]) < 1e-15
    got = run_op(probe, "quat_to_euler_extrinsic", [R.Case("pin", q, "rotation")], device=False)[0]
    orc = np.zeros(3)
    oracle_lib().orc_test_quat_to_euler(_ptr(np.array(q)), 0, _ptr(orc))
    for name, e in (("product", got), ("oracle", orc)):
        # r1's atan2 is the only rounding before the exact-to-1-ulp -r1 - pi: 6 ulp of pi/2 (the public bound of atan2) + 1 ulp of the result
        assert abs(e[1] - ref[1]) <= 6 * math.ulp(1.57) + math.ulp(4.7), (name, e)
        assert abs(e[0]) <= 2 * math.ulp(3.14) and abs(e[2]) <= 2 * math.ulp(3.14), (name, e)


def test_grouped_sign_prediction_cannot_miss_with_a_sign_exact_atan2():
    """quat_to_euler_zyx_grouped predicts r0 < 0 from (m10, m00) and falls back to the sequential form when atan2 disagrees.  With an atan2
    whose sign is right the prediction cannot miss: m00 = 1 - (2 y y + 2 z z) <= 1, so |atan2(m10, m00)| >= |m10| never underflows to zero, and
    the +-0 cases are the ones the predicate spells out.  Enumerated here over every class of (m10, m00 <= 1), zeros, denormals and infinities
    included; the fallback is therefore reachable on the device only through a quirk of its atan2, which test_gpu_math_primitives.py looks for."""
    vals = [0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-200, 1e-9, 0.5, 1.0, 1e9, 1e300, math.inf]
    m10s = vals + [-v for v in vals]
    m00s = [v for v in vals if v <= 1.0] + [-v for v in vals]
    for m10 in m10s:
        for m00 in m00s:
            neg = m10 < 0.0 or (m10 == 0.0 and math.copysign(1, m10) < 0 and math.copysign(1, m00) < 0)
            assert (math.atan2(m10, m00) < 0.0) == neg, (m10, m00)
    for q in R.grouped_quat_cases():       # and on the test's own cases, with the doubles the kernel forms
        neg, m10, m00 = R.neg_predicate(q)
        if not (math.isnan(m10) or math.isnan(m00)):
            assert (math.atan2(m10, m00) < 0.0) == neg, q


def test_roll_on_half_pi_under_a_flip_is_pinned(probe):
    """A second quirk of the fix-up, found by this suite: for (roll, pitch, yaw) = (-pi/2, 0.4, -0.7) Eigen's triple is flipped (yaw < 0) and its
    third angle is roll + pi, which rounds to the double M_PI / 2 exactly.  The fix-up's arms are `> M_PI/2.0` and `< M_PI/2.0`
    (standard_includes.h:281-288): neither takes it, and the roll comes back as +pi/2 - a triple that is NOT the input rotation (half a turn of
    roll off), where exact arithmetic (the mp reference) returns -pi/2.  Product and oracle are faithful to the reference's text; pinned."""
    q = R._qe([-math.pi / 2, 0.4, -0.7])
    ref = [float(v) for v in R.r_quat_to_euler(False)([mpf(v) for v in q])[0]]
    assert abs(ref[0] + math.pi / 2) < 1e-15
    got = run_op(probe, "quat_to_euler_extrinsic", [R.Case("pin", q, "rotation")], device=False)[0]
    orc = np.zeros(3)
    oracle_lib().orc_test_quat_to_euler(_ptr(np.array(q)), 0, _ptr(orc))
    for name, e in (("product", got), ("oracle", orc)):
        assert e[0] == math.pi / 2, (name, e)
        assert abs(e[1] - 0.4) <= 24 * math.ulp(4.8) and abs(e[2] + 0.7) <= 24 * math.ulp(4.8), (name, e)


# ------------------------------------------------------------------------------------------------ the oracle on the same edge lists

def _orc(fn, *args, n):
    out = np.zeros(n)
    fn(*args, _ptr(out))
    return out


ORACLE_OPS = ["euler_to_quat_extrinsic", "euler_to_quat_intrinsic", "quat_to_euler_extrinsic", "quat_to_euler_intrinsic", "from_two_vectors",
              "slerp", "quat_from_matrix", "quartic_bezier", "quartic_bezier_dot"]


@pytest.mark.parametrize("op", ORACLE_OPS)
def test_oracle_primitives_on_the_same_cases(op):
    """Where oracle and product differ by design the check is the one both must meet: inside FromTwoVectors' anti-parallel window each has its own
    deterministic orthogonal axis (Eigen's comes from an SVD), and the "window" check asserts only the unit norm and where a^ lands."""
    L = oracle_lib()
    cases = R.all_cases(op)
    got = []
    for c in cases:
        x = np.array(c.x)
        if op.startswith("euler_to_quat"):
            got.append(_orc(L.orc_test_euler_to_quat, _ptr(x), int(op.endswith("intrinsic")), n=4))
        elif op.startswith("quat_to_euler"):
            got.append(_orc(L.orc_test_quat_to_euler, _ptr(x), int(op.endswith("intrinsic")), n=3))
        elif op == "from_two_vectors":
            got.append(_orc(L.orc_test_from_two_vectors, _ptr(x[:3].copy()), _ptr(x[3:].copy()), n=4))
        elif op == "slerp":
            got.append(_orc(L.orc_test_slerp, _ptr(x[:4].copy()), float(x[4]), _ptr(x[5:].copy()), n=4))
        elif op == "quat_from_matrix":
            got.append(_orc(L.orc_test_quat_from_matrix, _ptr(x), n=4))
        else:
            b, db = np.zeros(3), np.zeros(3)
            L.orc_test_quartic_bezier(_ptr(x[:15].copy()), float(x[15]), _ptr(b), _ptr(db))
            got.append(b if op == "quartic_bezier" else db)
    worst, _ = check_op(op, cases, got, "oracle")
    print(f"oracle {op}: {len(cases)} cases, max error {worst:.3g} ulp")
