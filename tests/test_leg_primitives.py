"""CPU: the per-leg kinematics of csrc/shc_leg.hpp called directly - the host (x86) half of tests/leg_probe.hip, compiled with the product's flags -
against the 50-digit reference of tests/leg_reference.py: the reference project's own formulas (the 6 x 6 damped inverse, not the product's N x N
push-through form) on legs of the default hexapod, the synthetic octopod and the mixed-DOF robot, at seeded random joint states and at the
hand-written edges (stretched legs, a tip on the joint-1 axis, joints on their centres and limits, zero-range joints, padding joints, clamps on and
one ulp beside their thresholds ...).  The oracle faces the same edge lists where it has an entry point.  The device half, the fast (reciprocal)
forms, apply_ik and bearing_bracket run in test_gpu_leg_primitives.py.

Knife edges (the reference's branch signature changes under a move of one dynamic input by +-4 ulp), share of the random cases per op, from the mp
reference alone (seeds: leg_reference.seed_of): 0 % for every op at NJ = 3, 4, 5 - fk_chain, jacobian_columns, update_joints, tip_force_raw and
bearing_bracket_* 0 / 64 (fk_chain 0 / 63), fk_tip_pose 0 / 64, ik_step_*, ik_step_rotation_*, solve_ik_delta_* 0 / 64, apply_ik 0 / 12; the cap is 1 %.
apply_ik: no random case's per-axis deviation lies within 1e-6 m of the 5 mm tolerance; the smallest distance at NJ = 3 / 4 / 5 is 3.15e-3 / 3.75e-3 /
3.05e-4 m (test_apply_ik_random_cases_stay_clear_of_the_tolerance computes, prints and asserts it).
Hand-written edges that sit on a decision on purpose (costs of exactly 0, dq / dt on max_vel, q + v dt on a limit, directions on a sector's edge) carry the
check "decision" and are not counted in the share; a hand-written edge with the check "compare" that turns out to be a knife edge fails."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from mpmath import mpf

import leg_reference as R
from oracle_lib import _ptr, lib as oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))

def load_probe(tmp_dir):
    from syropod_highlevel_controller_amd import engine
    so = engine.compile_with_product_flags(os.path.join(HERE, "leg_probe.hip"), os.path.join(str(tmp_dir), "libleg_probe.so"))
    P = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    P.shc_leg_probe_op_name.restype = C.c_char_p
    P.shc_leg_probe_op_widths.argtypes = [C.c_int, C.c_int, ip, ip, ip, ip]
    P.shc_leg_probe_run.argtypes = [C.c_int, C.c_int, dp, dp, C.c_int, dp, C.c_int]
    P.ops = {P.shc_leg_probe_op_name(i).decode(): i for i in range(P.shc_leg_probe_op_count())}
    return P


def run_op(P, op, nj, cases, device):
    """one call (on the device: one launch) over all cases of an op at one NJ -> (n, nout) doubles"""
    npar, nin, nout, host = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert P.shc_leg_probe_op_widths(P.ops[op], nj, C.byref(npar), C.byref(nin), C.byref(nout), C.byref(host)) == 0
    params, dyn = R.pack(cases, nj)
    assert params.shape == (len(cases), npar.value) and (nin.value == 0 or dyn.shape == (len(cases), nin.value)), (op, params.shape, dyn.shape, nin.value)
    out = np.full((len(cases), nout.value), np.nan)
    rc = P.shc_leg_probe_run(P.ops[op], nj, _ptr(params), _ptr(dyn), len(cases), _ptr(out), int(device))
    assert rc == 0, f"shc_leg_probe_run({op}, NJ = {nj}) returned {rc}"
    return out


def check_op(op, nj, cases, got, what):
    """every case through its check -> (largest error in ulps of the reference's largest output, largest absolute error, share of the random cases on a knife edge)"""
    fails, worst, worst_abs, knives, n_random = [], 0.0, 0.0, 0, 0
    for c, g in zip(cases, got):
        rc, knife = R.resolve(op, nj, c)
        n_random += c.check is None
        knives += knife
        ok, err, msg, _ = R.check_case(op, nj, rc, g)
        if not ok:
            fails.append(f"  [{c.edge}] {msg}")
        u, a = R.max_ulps(op, nj, rc, g), R.max_abs(op, nj, rc, g)
        if u is not None and math.isfinite(u):
            worst = max(worst, u)
        if a is not None and math.isfinite(a):
            worst_abs = max(worst_abs, a)
    assert not fails, f"{what} {op} NJ = {nj}: {len(fails)} of {len(cases)} cases miss their check\n" + "\n".join(fails[:8])
    return worst, worst_abs, (knives / n_random if n_random else 0.0)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return load_probe(tmp_path_factory.mktemp("leg_probe"))


HOST_OPS = [op for op in R.K if op not in R.DEVICE_ONLY]
NJ_OF = {op: ((3,) if op.startswith("bearing_bracket") else R.NJS) for op in R.K}


def op_nj(ops):
    return [(op, nj) for op in ops for nj in NJ_OF[op]]


def test_probe_exports_every_op(probe):
    assert set(probe.ops) == set(R.K), set(probe.ops) ^ set(R.K)
    for op in R.K:
        host = C.c_int()
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        assert probe.shc_leg_probe_op_widths(probe.ops[op], 3, C.byref(a), C.byref(b), C.byref(c), C.byref(host)) == 0
        assert bool(host.value) == (op not in R.DEVICE_ONLY), op
        assert a.value == R.n_params(3)
    assert any(len(R.all_cases(op, nj)) % 64 for op, nj in op_nj(R.K)), "no op's case count leaves a partly filled last block"


@pytest.mark.parametrize("op,nj", op_nj(HOST_OPS))
def test_host_form_against_the_mp_reference(probe, op, nj):
    cases = R.all_cases(op, nj)
    worst, worst_abs, share = check_op(op, nj, cases, run_op(probe, op, nj, cases, device=False), "host")
    print(f"host {op} NJ = {nj}: {len(cases)} cases, max error {worst:.3g} ulp of the reference's largest output ({worst_abs:.3g} absolute), knife edges {share:.2%} of the random cases")
    assert share <= 0.01, f"{op}: {share:.2%} of the random cases are knife edges"


@pytest.mark.parametrize("op,nj", op_nj([op for op in R.DEVICE_ONLY if not op.endswith("_fast")]))
def test_knife_edge_share_of_the_device_only_ops(op, nj):
    """the share is a property of the inputs: computed here, from the mp reference alone, before anything runs on a GPU (the *_fast forms share the *_exact cases)"""
    share = R.knife_share(op, nj)
    print(f"{op} NJ = {nj}: knife edges {share:.2%} of the random cases")
    assert share <= 0.01


@pytest.mark.parametrize("nj", R.NJS)
def test_apply_ik_random_cases_stay_clear_of_the_tolerance(nj):
    """as test_gpu_reach.py asserts of its inputs: no random case's deviation lies within 1e-6 m of the 5 mm tolerance; and the hand-written edges hold what
    they are named for - a success and a failure beside the tolerance, and at NJ = 5 a constrained success, a retry after a deviation, a retry on a proximity of 0"""
    m = R.apply_ik_margin(nj)
    print(f"apply_ik NJ = {nj}: the random cases' deviations stay {m:.3g} m from the tolerance")
    assert m >= 1e-6
    seen = set()
    for c in R.all_cases("apply_ik", nj):
        if c.check in (None, "window"):
            continue
        out, sig, _ = R._ref("apply_ik", nj, c.x)
        success, failed, retried = float(out[2 * nj]), bool(out[2 * nj + 1]), bool(out[2 * nj + 2])
        constrained = c.x[R.n_params(nj) + 2 * nj + 3] != 0
        seen.add((constrained, failed, retried, success == 0.0))
    assert (False, False, False, False) in seen and (False, True, False, True) in seen
    assert (False, False, False, True) in seen, "no unconstrained case ends on a proximity of exactly 0"
    if nj == 5:
        assert (True, False, False, False) in seen, "no constrained pass succeeds"
        assert any(s[0] and s[1] and s[2] for s in seen), "no constrained pass fails on a deviation and retries"
        assert (True, False, True, True) in seen or (True, False, True, False) in seen, "no retry fires without a deviation"


@pytest.mark.parametrize("nj", (4, 5))
def test_padding_joints_are_pinned(probe, nj):
    """behind the tip of a shorter leg: lin, dq of all three solves and q, qd through update_joints are exactly 0 (not small: a locked joint never moves), and
    the active part agrees with the reference of the leg_dof-joint leg, which has no such joint"""
    n = 0
    for op in ("leg_const", "jacobian_columns", "ik_step_exact", "ik_step_rotation_exact", "solve_ik_delta_exact", "update_joints"):
        cases = [c for c in R.all_cases(op, nj) if int(c.x[R.n_params(nj) - 1]) < nj]
        assert len(cases) >= 3, op
        got = run_op(probe, op, nj, cases, device=False)
        for c, g in zip(cases, got):
            assert not R.padding_pins(op, nj, c.x, [float(v) for v in g]), (op, c.edge)
            n += 1
    assert n > 50


# ------------------------------------------------------------------------------------------------ the oracle on the same edge lists

def _params_of(nj, x):
    """a Params whose leg 0 is the case's leg (the oracle takes the robot, not the leg)"""
    from syropod_highlevel_controller_amd.params import JointParams, LinkParams, default_hexapod_params
    P = default_hexapod_params("tripod")
    L = R.Leg(nj, x[:R.n_params(nj)])
    P.leg_dof[0] = L.dof
    P.link[0][0] = LinkParams(*[float(v) for v in L.base])
    for k in range(L.dof):
        d, r, alpha, theta = (float(v) for v in L.links[k])
        P.link[0][k + 1] = LinkParams(d, theta, r, alpha)
        P.joint[0][k] = JointParams(L.joints[k][0], L.joints[k][1], 0.0, 0.0, L.joints[k][2])
    return P, L.dof


def test_oracle_dh_matrix_on_the_leg_const_cases():
    """orc_test_dh_matrix on every base link: the entries LegConst::r1 / p1 hold, to the same 9 ulp"""
    L = oracle_lib()
    n = 0
    for nj in R.NJS:
        for c in R.all_cases("leg_const", nj):
            out, _, tol, _, _ = R.evaluate("leg_const", nj, c.x)
            m = np.zeros(16)
            L.orc_test_dh_matrix(*[float(v) for v in c.x[:4]], _ptr(m))
            m = m.reshape(4, 4)
            got = [m[i, j] for i in range(3) for j in range(3)] + [m[i, 3] for i in range(3)]
            for g, r, t in zip(got, out[:12], tol[:12]):
                assert abs(mpf(float(g)) - r) <= t, (c.edge, g, float(r))
            n += 1
    assert n > 20


@pytest.mark.parametrize("nj", R.NJS)
def test_oracle_leg_fk_on_the_chain_cases(nj):
    """orc_test_leg_fk (tip pose in the robot frame) against the bound fk_tip_pose is held to; +-q is the same rotation"""
    L = oracle_lib()
    worst = 0.0
    for c in R.all_cases("fk_tip_pose", nj):
        P, dof = _params_of(nj, c.x)
        q = np.array(c.x[R.n_params(nj):R.n_params(nj) + dof])
        tip, quat = np.zeros(3), np.zeros(4)
        L.orc_test_leg_fk(C.byref(P), 0, _ptr(q), _ptr(tip), _ptr(quat))
        out, _, tol, knife, _ = R.evaluate("fk_tip_pose", nj, c.x)
        got = list(tip) + list(quat)
        flip = list(tip) + [-v for v in quat]
        e = min(R._within(got, out, tol), R._within(flip, out, tol))
        assert e <= 1.0, f"oracle fk [{c.edge}]: {e:.3g} x the tolerance"
        worst = max(worst, e)
    print(f"oracle leg_fk NJ = {nj}: max {worst:.3g} x the tolerance")


@pytest.mark.parametrize("nj", R.NJS)
def test_oracle_ik_step_on_the_unconstrained_apply_ik_cases(nj):
    """orc_test_leg_ik_step = one applyIK(simulation) without a desired rotation: the unconstrained apply_ik cases with the velocity clamp off (simulation), held to
    the reference and tolerance of exactly those inputs"""
    L = oracle_lib()
    worst, n = 0.0, 0
    for c in R.all_cases("apply_ik", nj):
        p = R.n_params(nj)
        dyn = list(c.x[p:])
        if dyn[2 * nj + 3] != 0 or c.check == "window" or dyn[2 * nj + 8] == 0:
            continue
        dyn[2 * nj + 7] = 0.0          # simulation: no velocity clamp (model.cpp:812)
        x = list(c.x[:p]) + dyn
        P, dof = _params_of(nj, x)
        assert P.clamp_joint_positions
        q, qd, des = np.array(dyn[:dof]), np.array(dyn[nj:nj + dof]), np.array(dyn[2 * nj:2 * nj + 3])
        qo, qdo, tip = np.zeros(dof), np.zeros(dof), np.zeros(3)
        res = L.orc_test_leg_ik_step(C.byref(P), 0, _ptr(q), _ptr(qd), _ptr(des), 1, _ptr(qo), _ptr(qdo), _ptr(tip))
        out, sig, tol, knife, _ = R.evaluate("apply_ik", nj, x)
        if knife:
            continue
        pad = [0.0] * (nj - dof)
        got = list(qo) + pad + list(qdo) + pad + [res, float(out[2 * nj + 1]), 0.0] + list(tip)      # (the oracle's call does not report `failed`)
        e = R._within(got, out, tol)
        assert e <= 1.0, f"oracle applyIK [{c.edge}]: {e:.3g} x the tolerance; got {got}, reference {[float(v) for v in out]}"
        worst, n = max(worst, e), n + 1
    assert n >= 10
    print(f"oracle leg_ik_step NJ = {nj}: {n} cases, max {worst:.3g} x the tolerance")
