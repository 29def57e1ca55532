"""GPU: the device half of tests/leg_probe.hip - the per-leg kinematics of csrc/shc_leg.hpp as the kernels run them (one launch per op and NJ over all its
cases, each case's LegConst read from global memory into registers) - against the 50-digit reference, with the cases and checks of
test_leg_primitives.py; and the device-only forms: the reciprocal (`_fast`) solves every kernel uses, apply_ik_core with empty hooks, bearing_bracket.

Knife-edge shares of the random cases (from the mp reference alone, asserted on the CPU in test_leg_primitives.py before anything runs here): 0 % for
every op and NJ.  apply_ik: the random cases' deviations stay at least 3e-4 m from the 5 mm tolerance (asserted >= 1e-6 m there)."""
import math

import numpy as np
import pytest

import leg_reference as R
from conftest import parity_report
from test_leg_primitives import HOST_OPS, check_op, load_probe, op_nj, run_op

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return load_probe(tmp_path_factory.mktemp("leg_probe_gpu"))


def _host_device_ulps(host, dev):
    """largest host-versus-device difference in ulps of the host value (reported, not asserted: libm and ocml are not claimed equal)"""
    worst = 0.0
    for h, d in zip(np.asarray(host).reshape(-1), np.asarray(dev).reshape(-1)):
        if math.isfinite(h) and math.isfinite(d) and h != d and h != 0.0:
            worst = max(worst, abs(h - d) / R.ulp(h))
    return worst


@pytest.mark.parametrize("op,nj", op_nj(HOST_OPS))
def test_device_form_against_the_mp_reference(probe, op, nj):
    cases = R.all_cases(op, nj)
    dev = run_op(probe, op, nj, cases, device=True)
    host = run_op(probe, op, nj, cases, device=False)
    parity_report(f"leg primitive {op} NJ = {nj}: host vs device max {_host_device_ulps(host, dev):.3g} ulp over {len(cases)} cases")
    worst, worst_abs, share = check_op(op, nj, cases, dev, "device")
    parity_report(f"leg primitive {op} NJ = {nj}: device max error {worst:.3g} ulp of the mp reference's largest output ({worst_abs:.3g} absolute)")
    assert share <= 0.01


@pytest.mark.parametrize("op,nj", op_nj(R.DEVICE_ONLY))
def test_device_only_forms(probe, op, nj):
    """the `_fast` solves (fast_rcp / fast_rsqrt in place of the division and the square root: what every cycle kernel runs) on the cases of their `_exact`
    twins and to the same tolerance; apply_ik_core: q, qd, the tip and the proximity to the propagated tolerance, `failed` and `retried` exactly; bearing_bracket:
    the sector exactly, either neighbour on a sector's edge.  Denormal directions: the rotated components round to whole denormals but never both to zero, so the
    fall-through to a fixed sector is not reached.  Two named differences: below 2.2e-308 that rounding can move a direction within
    5e-324 / |v| rad of a sector's edge into the neighbouring sector - (5e-324, -5e-322), 0.07 degrees from the edge at 179.5, is sector 4 where atan2 gives 3 (a
    knife edge by the +-4 ulp rule, counted and reported below; nothing differs from 1e-300 up); and atan2's signed zero at (+-0, -0), where the text gives sector 4
    and the product sector 0, pinned by the check "signed_zero"."""
    cases = R.all_cases(op, nj)
    dev = run_op(probe, op, nj, cases, device=True)
    worst, worst_abs, share = check_op(op, nj, cases, dev, "device")
    parity_report(f"leg primitive {op} NJ = {nj}: device max error {worst:.3g} ulp of the mp reference's largest output ({worst_abs:.3g} absolute) over {len(cases)} cases")
    assert share <= 0.01
    if op.startswith("bearing_bracket"):
        fell = [c.edge for c, g in zip(cases, dev) if c.check == "decision" and "denormal" in c.edge and g[0] != float(R.evaluate(op, nj, c.x)[0][0])]
        parity_report(f"leg primitive {op}: denormal directions off the reference's sector (all on a sector's edge): {len(fell)}")


@pytest.mark.parametrize("nj", (4, 5))
def test_padding_joints_are_pinned_on_the_device(probe, nj):
    """behind the tip of a shorter leg lin, dq (exact and fast solves) and q, qd (update_joints, apply_ik) are exactly 0"""
    n = 0
    for op in ("leg_const", "jacobian_columns", "ik_step_fast", "ik_step_rotation_fast", "solve_ik_delta_fast", "ik_step_exact", "update_joints", "apply_ik"):
        cases = [c for c in R.all_cases(op, nj) if int(c.x[R.n_params(nj) - 1]) < nj]
        assert len(cases) >= 3, op
        for c, g in zip(cases, run_op(probe, op, nj, cases, device=True)):
            assert not R.padding_pins(op, nj, c.x, [float(v) for v in g]), (op, c.edge)
            n += 1
    assert n > 60
