"""GPU: the device half of tests/math_probe.hip - every math primitive of csrc/shc_math.hpp as the kernels run it (one launch per op over all
its cases) - against the 50-digit reference, with the cases and checks of test_math_primitives.py; the device-only forms (fast_rcp, fast_rsqrt,
spd_solve<N, false>); and the two lane-grouped forms of shc_cycle.hpp, which must be bit-identical to the scalar device form at every L."""
import math

import numpy as np
import pytest

import math_reference as R
from conftest import parity_report
from oracle_lib import _ptr
from test_math_primitives import HOST_OPS, check_op, load_probe, run_op

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return load_probe(tmp_path_factory.mktemp("math_probe_gpu"))


def _host_device_ulps(host, dev):
    """largest host-versus-device difference in ulps of the host value (reported, not asserted: libm and ocml are not claimed equal)"""
    worst = 0.0
    for h, d in zip(np.asarray(host).reshape(-1), np.asarray(dev).reshape(-1)):
        if math.isfinite(h) and math.isfinite(d) and h != d:
            worst = max(worst, abs(h - d) / R.ulp(h))
    return worst


@pytest.mark.parametrize("op", HOST_OPS)
def test_device_form_against_the_mp_reference(probe, op):
    """(sincos_joint_reduce: see test_math_primitives.test_host_form_against_the_mp_reference for the bound it is held to.)"""
    cases = R.all_cases(op)
    dev = run_op(probe, op, cases, device=True)
    host = run_op(probe, op, cases, device=False)
    parity_report(f"math primitive {op}: host vs device max {_host_device_ulps(host, dev):.3g} ulp over {len(cases)} cases")
    worst, share = check_op(op, cases, dev, "device")
    parity_report(f"math primitive {op}: device max error {worst:.3g} ulp of the mp reference (k = {R.K[op][1]})")
    assert share <= 0.01


@pytest.mark.parametrize("op", R.DEVICE_ONLY)
def test_device_only_forms(probe, op):
    """fast_rcp / fast_rsqrt: the hardware estimate + two Newton steps, <= 1 ulp of the mp value as shc_math.hpp states, on lambda^2 = 4e-4 ... 1e6,
    powers of two +-1 ulp and a log-uniform sweep of 1e5 values; spd_solve<N, false> (which uses them) to kappa(A) eps |x|."""
    cases = R.all_cases(op)
    dev = run_op(probe, op, cases, device=True)
    if op in ("fast_rcp", "fast_rsqrt"):        # vectorised: 1e5 mp evaluations one by one are not needed for a one-rounding reference
        x = R.pack(cases)[:, 0].astype(np.longdouble)
        ref = 1 / x if op == "fast_rcp" else 1 / np.sqrt(x)
        # the 64-bit-mantissa reference is within 2^-11 ulp of the true value: cases within that of the 1-ulp bound go to mp
        err = np.abs(dev[:, 0].astype(np.longdouble) - ref) / np.array([R.ulp(float(r)) for r in ref])
        worst = float(err.max())
        for i in np.nonzero(err > 0.99)[0]:
            ok, e, msg = R.check_case(op, cases[i], dev[i])
            assert ok, msg
        for i in range(200):                        # and the hand-written edges through mp itself
            ok, e, msg = R.check_case(op, cases[i], dev[i])
            assert ok, f"[{cases[i].edge}] {msg}"
        parity_report(f"math primitive {op}: device max error {worst:.3g} ulp over {len(cases)} values (stated: <= 1)")
        return
    worst, _ = check_op(op, cases, dev, "device")
    parity_report(f"math primitive {op}: device max error {worst:.3g} ulp of |x| (bound (4 N + 1) kappa(A) eps)")


@pytest.mark.parametrize("L", [3, 4, 5, 6, 7, 8])
def test_grouped_forms_are_bit_identical_to_the_scalar_form(probe, L):
    """quat_to_euler_zyx_grouped / euler_to_quat_zyx_grouped in the cycle kernel's group layout, one case per Group<L>: every lane of every group holds
    exactly the bits of the scalar quat_to_euler / euler_to_quat of the same lane (shc_cycle.hpp promises the same instructions on the same operands).
    Cases: the whole quat_to_euler edge list, m10 on both sides of the sign prediction with +-0 and denormals; full wavefronts and a last wavefront that
    is partly filled (mirror lanes).  The fallback ((r0 < 0) != neg) cannot be provoked from the inputs with a sign-exact atan2
    (test_math_primitives.test_grouped_sign_prediction_cannot_miss_with_a_sign_exact_atan2): whether ocml's atan2 ever disagrees with the prediction
    is reported here from the scalar form's outputs."""
    rpw = 64 // L
    for which, cases, nin, nres in ((0, R.grouped_quat_cases(), 4, 3), (1, R.grouped_euler_cases(), 3, 4)):
        for n in (len(cases) - len(cases) % rpw, len(cases) - len(cases) % rpw - 1, len(cases)):        # whole waves; last group missing; as it comes
            x = np.ascontiguousarray(cases[:n], dtype=np.float64)
            out = np.full((n, L, 2 * nres), np.nan)
            rc = probe.shc_probe_run_grouped(which, L, _ptr(x), n, _ptr(out))
            assert rc == 0, rc
            g, s = R.bits(out[:, :, :nres]), R.bits(out[:, :, nres:])
            bad = np.argwhere(g != s)
            assert bad.size == 0, f"L = {L}, form {which}, n = {n}: case {cases[bad[0][0]]} lane {bad[0][1]}: grouped {out[bad[0][0], bad[0][1]]}"
            assert (R.bits(out) == R.bits(out[:, :1, :])).all(), "the lanes of a group disagree"
    parity_report(f"math primitive grouped forms L = {L}: bit-identical to the scalar device form")
