"""GPU (-m gpu): the reach probe (include/shc_batch.h, "Reach probe": shc_engine_probe_reach, shc_fleet_probe_reach_device) against its
definition - the oracle's setDesiredTipPose + applyIK(simulation) walked along the line step by step - against the engine's own per-leg
calls, and as a pass that moves bytes and writes nothing into an engine.

The base scenario is walking_pair of test_gpu_leg_api.py (make_inputs(p, n, 81), 137 cycles, the engine's state set from the oracle's).
Candidates (C = 3), with o the tip position FK gives for the stored joints and u unit vectors from default_rng(5): o + 0.02 u (near: almost
every leg gets there), o + 0.6 u * (1, 1, 0.3) (far: no leg gets there), and the near one with NaN on the odd legs (not asked).

What the oracle said about these inputs on the CPU, before any of this ran on a GPU (S = 16 unless noted; legs full / partial / zero; the
margin is the smallest | max|tip - desired| - 5 mm | over every executed step, which the test asserts to be above 1e-6 m):
    hexapod n = 23          near 134 / 2 / 2      far 0 / 65 / 73     margin 2.5e-5 m
    hexapod n = 23, S = 1   near 131 / - / 7      far 0 / - / 138     margin 3.7e-5 m
    octopod 8 x 5 n = 9     near 72 / 0 / 0       far 0 / 44 / 28     margin 2.1e-5 m
    mixed DOF n = 11        near 66 / 0 / 0       far 0 / 43 / 23     margin 3.0e-5 m   (make_inputs seed 83, see MIXED_SEED)
"""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (REACH_FIELD_NAMES, SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError, device_count,
                                                     reach_columns, reach_spec)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_leg_api import walking_pair
from test_gpu_mixed_dof import padded
from test_gpu_parity import make_inputs
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

ALL = tuple(REACH_FIELD_NAMES)
IK_TOLERANCE = 0.005       # model.h: IK_TOLERANCE, the deviation applyIK refuses
SENTINEL = 1e30
TOL = 1e-9                 # the bar of test_gpu_leg_api.py:86-94 for this pattern, engine against oracle
# make_inputs' seed of the mixed-DOF pair, fixed from the oracle alone: with 81 an executed step of the oracle's lies 5.4e-7 m from the tolerance
# (borderline by the condition above: such inputs say nothing about the kernel), with 82 4.0e-6 m; 83 is the first seed whose margin is of the
# size of the other shapes' (3.0e-5 m)
MIXED_SEED = 83


def need_gpu():
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")


def max_dof(p):
    return max(p.leg_dof[l] for l in range(p.leg_count))


def pair(p, n, seed=81, cycles=137):
    """walking_pair; a robot whose legs differ in DOF takes the same velocities without the joint torques (make_inputs shapes those for equal legs)"""
    need_gpu()
    if len({p.leg_dof[l] for l in range(p.leg_count)}) == 1:
        return walking_pair(BatchEngine, p, n, seed, cycles)
    inp = make_inputs(p, n, seed)
    eng, ob = BatchEngine(p, n), OracleBatch(p, n)
    for o in (eng, ob):
        o.set_velocity(inp["lin"], inp["ang"])
    eng.step(cycles)
    eng.synchronize()
    ob.step(cycles, 8)
    eng.set_state(ob.get_state())
    return eng, ob


def candidates(origin, far=0.6):
    """(n, 3, L, 3): near, far, near with NaN on the odd legs"""
    n, L = origin.shape[:2]
    u = np.random.default_rng(5).normal(size=(n, L, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    near, away = origin + 0.02 * u, origin + far * u * np.array([1.0, 1.0, 0.3])
    masked = near.copy()
    masked[:, 1::2] = np.nan
    return np.ascontiguousarray(np.stack([near, away, masked], axis=1))


def oracle_reach(ob, p, saved, targets, S):
    """The definition, candidate by candidate from the saved state: {done, limit_proximity, tip, q, asked}, (n, C, L[, k]) each, and the
    smallest distance of an executed step's deviation from the tolerance."""
    n, cands, L, D = targets.shape[0], targets.shape[1], p.leg_count, max_dof(p)
    ob.set_state(saved)
    origin = ob.leg_apply_fk()[:, :3].reshape(n, L, 3)
    res = {"done": np.zeros((n, cands, L), dtype=np.int64), "limit_proximity": np.zeros((n, cands, L)), "tip": np.zeros((n, cands, L, 3)),
           "q": np.zeros((n, cands, L, D)), "asked": ~np.isnan(targets).any(axis=3)}
    margin = np.inf
    for c in range(cands):
        ob.set_state(saved)
        asked = res["asked"][:, c]
        t = np.where(asked[..., None], targets[:, c], origin)   # (a leg that is not asked still needs numbers: what it does is dropped)
        alive = asked.copy()
        for s in range(1, S + 1):
            w = float(s) / S
            desired = origin * (1.0 - w) + t * w
            pose = np.zeros((n * L, 7))
            pose[:, :3] = desired.reshape(-1, 3)
            ob.leg_set_desired_tip_pose(pose, apply_delta=False)
            r = ob.leg_apply_ik(True).reshape(n, L)
            tip = ob.leg_apply_fk()[:, :3].reshape(n, L, 3)
            q = padded(ob.joints()[0], p).reshape(n, L, D)
            if alive.any():
                margin = min(margin, float(np.abs(np.abs(tip - desired).max(axis=2) - IK_TOLERANCE)[alive].min()))
            res["limit_proximity"][:, c][alive], res["tip"][:, c][alive], res["q"][:, c][alive] = r[alive], tip[alive], q[alive]
            alive = alive & (r != 0.0)       # the test stops counting a leg at its first zero
            res["done"][:, c][alive] += 1
    ob.set_state(saved)
    return res, margin


def upload(a, dtype="float64"):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64 if np.dtype(dtype) == np.float64 else torch.float32).cuda()
    torch.cuda.synchronize()   # the engines run on streams of their own: the tensor is complete before a call
    return t


def probe(who, targets, S, fields=ALL, dtype="float64", **kw):
    """probe_reach and a wait: the (n, C, D) host array"""
    out = who.probe_reach(upload(targets, dtype), S, fields, **kw)
    who.synchronize()
    return out.cpu().numpy()


def split(got, fields, legs, dof):
    """{field: (n, C, legs[, k])} of a (n, C, D) result"""
    cols, width = reach_columns(fields, legs, dof)
    assert got.shape[2] == width
    out = {}
    for name in fields:
        block = got[:, :, cols[name]].reshape(got.shape[0], got.shape[1], legs, -1)
        out[name] = block[..., 0] if block.shape[3] == 1 else block
    return out


def assert_reach(got, want, S, what):
    """The comparison of cases 1 and 2: steps_done exactly, q / tip / limit proximity within TOL, NaN where a leg was not asked"""
    asked = want["asked"]
    assert np.array_equal(got["fraction"][asked], want["done"][asked] / float(S)), f"{what}: steps_done differs"
    for name in ("limit_proximity", "tip", "q"):
        err = float(np.abs(got[name][asked] - want[name][asked]).max())
        print(f"[reach {what}] max |d {name}| = {err:.3e}")
        assert err <= TOL, (what, name, err)
    for name in ALL:
        assert np.isnan(got[name][~asked]).all(), f"{what}: a leg that was not asked holds a value in {name}"


def outcome_classes(done, asked, S):
    """legs (full, partial, zero) per candidate"""
    return [(int((done[:, c][asked[:, c]] == S).sum()), int(((done[:, c] > 0) & (done[:, c] < S))[asked[:, c]].sum()), int((done[:, c][asked[:, c]] == 0).sum()))
            for c in range(done.shape[1])]


SHAPES = {"hexapod": (lambda: default_hexapod_params("tripod"), 23, 81), "octopod-5dof": (lambda: synthetic_octopod_params("ripple", 5, 8), 9, 81),
          "mixed-dof": (lambda: synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4)), 11, MIXED_SEED)}


# ------------------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("shape,S", [("hexapod", 16), ("hexapod", 1), ("octopod-5dof", 16), ("mixed-dof", 16)])
def test_against_the_oracle(shape, S):
    make, n, seed = SHAPES[shape]
    p = make()
    eng, ob = pair(p, n, seed)
    try:
        L, D = p.leg_count, max_dof(p)
        saved = ob.get_state()
        origin = ob.leg_apply_fk()[:, :3].reshape(n, L, 3)
        targets = candidates(origin)
        want, margin = oracle_reach(ob, p, saved, targets, S)
        classes = outcome_classes(want["done"], want["asked"], S)
        print(f"[reach {shape} S={S}] legs full / partial / zero per candidate {classes}, margin to the 5 mm tolerance {margin:.2e} m")
        # a property of the inputs, not a tolerance: no executed step of the oracle's lies within 1e-6 m of the tolerance, so a difference at
        # rounding level cannot change steps_done
        assert margin > 1e-6, margin
        full, partial, zero = (sum(c[k] for c in classes) for k in range(3))
        assert full > 0 and zero > 0 and (partial > 0 or S == 1), classes
        assert (~want["asked"]).any()
        got = split(probe(eng, targets, S), ALL, L, D)
        assert_reach(got, want, S, f"{shape} S={S}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 2. against the existing calls
def existing_calls(eng, targets, S):
    """Route (b), what a caller has today, with device arrays: per candidate a checkpoint restore, S x (shc_leg_set_desired_tip_pose +
    shc_leg_apply_ik(simulation = 1), every leg), then the joints and shc_leg_apply_fk.  Returns what oracle_reach returns."""
    import torch
    n, cands, L, D = targets.shape[0], targets.shape[1], eng.legs, eng.dof
    lib = eng.L
    ck = eng.checkpoint()
    origin = eng.leg_apply_fk()[:, :3].reshape(n, L, 3)
    res = {"done": np.zeros((n, cands, L), dtype=np.int64), "limit_proximity": np.zeros((n, cands, L)), "tip": np.zeros((n, cands, L, 3)),
           "q": np.zeros((n, cands, L, D)), "asked": ~np.isnan(targets).any(axis=3)}
    result = torch.zeros(n * L, dtype=torch.float64, device="cuda")
    tips = torch.zeros((n * L, 7), dtype=torch.float64, device="cuda")
    for c in range(cands):
        eng.restore(ck)
        asked = res["asked"][:, c]
        t = np.where(asked[..., None], targets[:, c], origin)
        alive = asked.copy()
        for s in range(1, S + 1):
            w = float(s) / S
            pose = np.zeros((n * L, 7))
            pose[:, :3] = (origin * (1.0 - w) + t * w).reshape(-1, 3)
            d_pose = upload(pose)
            assert lib.shc_leg_set_desired_tip_pose(eng.h, 0, n, -1, C.c_void_p(d_pose.data_ptr()), 0, 1) == SHC_OK
            assert lib.shc_leg_apply_ik(eng.h, 0, n, -1, 1, C.c_void_p(result.data_ptr()), 1) == SHC_OK
            assert lib.shc_leg_apply_fk(eng.h, 0, n, -1, None, C.c_void_p(tips.data_ptr()), 1) == SHC_OK
            eng.synchronize()
            r, tip = result.cpu().numpy().reshape(n, L), tips.cpu().numpy()[:, :3].reshape(n, L, 3)
            q = eng.joints()[0].reshape(n, L, D)
            res["limit_proximity"][:, c][alive], res["tip"][:, c][alive], res["q"][:, c][alive] = r[alive], tip[alive], q[alive]
            alive = alive & (r != 0.0)
            res["done"][:, c][alive] += 1
    eng.restore(ck)
    eng.synchronize()
    ck.close()
    return res


@pytest.fixture(scope="module")
def hexapods():
    """The hexapod pair of case 1 once more for the cases below: (engine, a twin with the same state, the candidates)"""
    p = default_hexapod_params("tripod")
    (eng, ob), (twin, _) = pair(p, 23), pair(p, 23)
    for e in (eng, twin):   # (leg_state() refreshes the derived tips, which the auxiliary blob carries)
        e.leg_state()
    targets = candidates(ob.leg_apply_fk()[:, :3].reshape(23, 6, 3))
    yield eng, twin, targets
    eng.close(), twin.close()


def test_against_the_existing_calls(hexapods):
    eng, twin, targets = hexapods
    before = state_bytes(twin)
    want = existing_calls(twin, targets, 16)
    assert state_bytes(twin) == before         # (route (b) ends on a restore: the twin is the twin again)
    got = split(probe(eng, targets, 16), ALL, 6, 3)
    assert_reach(got, want, 16, "hexapod, existing calls")


# ------------------------------------------------------------------------------------------------------------ 3. nothing written
def everything(eng):
    q, qd = eng.joints()
    ls = eng.leg_state()
    return state_bytes(eng), bytes(eng.get_aux_state()), q.tobytes() + qd.tobytes(), b"".join(np.ascontiguousarray(ls[k]).tobytes() for k in sorted(ls))


def test_nothing_is_written(hexapods):
    eng, twin, targets = hexapods
    before = everything(eng)
    assert before == everything(twin)
    saved = eng.get_state(), eng.get_aux_state()
    for S, fields, dtype in ((16, ALL, "float64"), (3, ("tip",), "float32")):
        probe(eng, targets, S, fields, dtype)
        assert everything(eng) == before, "the probe wrote into the engine"
    for e in (eng, twin):
        e.step(60)
        e.synchronize()
    after = everything(eng)
    assert after == everything(twin) and after != before, "60 cycles after a probe differ from 60 cycles without one"
    for e in (eng, twin):   # (back to the scenario, for the cases below)
        e.set_state(saved[0])
        e.set_aux_state(saved[1])
        e.leg_state()
    assert everything(eng) == everything(twin)


def test_nothing_is_written_between_split_steps():
    """40 970 hexapods = 4 097 wavefronts, the smallest batch whose steps run as two halves on two streams: the probe, called straight after
    step with no synchronise, joins them by events and reads the joints both halves left - its rows are those of a call made after a join -
    and the engine walks on to the bytes of a twin that never probed."""
    need_gpu()
    p = default_hexapod_params("tripod")
    n = 40970
    a, b = BatchEngine(p, n), BatchEngine(p, n)
    try:
        rng = np.random.default_rng(13)
        lin, ang = rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.4, 0.4, n)
        for e in (a, b):
            e.set_velocity(lin, ang)
            e.step(30)
        tips = a.leg_apply_fk()[:, :3].reshape(n, 6, 3)
        b.leg_apply_fk()
        targets = upload((tips + np.array([0.03, -0.02, 0.01]))[:, None], "float32")
        a.step(2)
        first = a.probe_reach(targets, 2, ("fraction", "tip"))       # no synchronise since the step: both halves are in flight
        a.join()
        a.synchronize()
        second = a.probe_reach(targets, 2, ("fraction", "tip"))      # the same joints, after a join and a wait
        a.step(2)
        a.synchronize()
        b.step(2)                                                    # the twin never probes
        b.step(2)
        b.synchronize()
        assert first.cpu().numpy().tobytes() == second.cpu().numpy().tobytes()
        assert (first[:, 0, :6] >= 0).all() and (first[:, 0, :6] > 0).any()
        assert state_bytes(a) == state_bytes(b) and bytes(a.get_aux_state()) == bytes(b.get_aux_state())
        qa, qb = a.joints(), b.joints()
        assert qa[0].tobytes() == qb[0].tobytes() and qa[1].tobytes() == qb[1].tobytes()
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ 4. bytes
def test_bytes(hexapods):
    import torch
    eng, _twin, targets = hexapods
    n, S = 23, 16
    full = probe(eng, targets, S)
    assert probe(eng, targets, S).tobytes() == full.tobytes(), "the same call twice"
    # permuting the candidates permutes the blocks
    order = [2, 0, 1]
    assert probe(eng, targets[:, order], S).tobytes() == np.ascontiguousarray(full[:, order]).tobytes()
    # a range returns the rows of the full call: inside a robot group, across two, the last partly filled group alone
    for first, count in ((3, 4), (7, 15), (20, 3), (0, 23), (22, 1)):
        assert probe(eng, targets[first:first + count], S, first=first, count=count).tobytes() == np.ascontiguousarray(full[first:first + count]).tobytes(), (first, count)
    # every selection of one field is the columns of the full call
    cols, width = reach_columns(ALL, 6, 3)
    for name in ALL:
        assert probe(eng, targets, S, (name,)).tobytes() == np.ascontiguousarray(full[:, :, cols[name]]).tobytes(), name
    # strided rows on both sides, sentinel-filled guard columns: never touched
    fields = ("tip", "fraction", "limit_proximity")
    D = reach_columns(fields, 6, 3)[1]
    for dtype, tdt in (("float64", torch.float64), ("float32", torch.float32)):
        big_in = torch.full((n, 3 * 18 + 5), SENTINEL, dtype=tdt, device="cuda")
        big_in[:, :3 * 18] = upload(targets.reshape(n, -1), dtype)
        big_out = torch.full((n, 3 * D + 7), SENTINEL, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        view_in, view_out = big_in[:, :3 * 18].unflatten(1, (3, 6, 3)), big_out[:, :3 * D].unflatten(1, (3, D))
        assert eng.probe_reach(view_in, S, fields, out=view_out) is view_out
        eng.synchronize()
        got = big_out.cpu().numpy()
        assert (got[:, 3 * D:] == np.dtype(dtype).type(SENTINEL)).all(), "a guard column was written"
        assert (big_in.cpu().numpy()[:, 3 * 18:] == np.dtype(dtype).type(SENTINEL)).all()
        assert got[:, :3 * D].tobytes() == probe(eng, targets.astype(dtype).astype(np.float64), S, fields, dtype).tobytes()
    # float32-representable targets: the float32 output is the float64 output cast, byte for byte (pad -2.5 is representable too)
    t32 = targets.astype(np.float32)
    wide = probe(eng, t32.astype(np.float64), S, ALL, "float64", pad=-2.5)
    narrow = probe(eng, t32, S, ALL, "float32", pad=-2.5)
    assert narrow.dtype == np.float32 and narrow.tobytes() == wide.astype(np.float32).tobytes()
    # pad: NaN targets, and the legs and joints a hexapod lacks in an 8 x 5 row geometry
    got = split(probe(eng, targets, S, ALL, "float64", pad=-2.5), ALL, 6, 3)
    for name in ALL:
        assert (got[name][:, 2, 1::2] == -2.5).all() and (got[name][:, 2, 0::2] != -2.5).all(), name
    t8 = np.full((n, 3, 8, 3), SENTINEL)
    t8[:, :, :6] = targets
    got8 = split(probe(eng, t8, S, ALL, "float64", pad=-2.5, legs=8, dof=5), ALL, 8, 5)
    for name in ALL:
        assert (got8[name][:, :, 6:] == -2.5).all(), f"{name}: a leg the robot lacks"
        own = got8[name][:, :, :6, :3] if name == "q" else got8[name][:, :, :6]
        assert np.ascontiguousarray(own).tobytes() == np.ascontiguousarray(got[name]).tobytes(), name
    assert (got8["q"][:, :, :6, 3:] == -2.5).all(), "a joint the robot lacks"


# ------------------------------------------------------------------------------------------------------------ 5. fleet
FLEET_N = 29
FLEET_MORPH = np.arange(FLEET_N, dtype=np.int32) % 3      # hexapod, 8 x 5, 4 x 4 interleaved


def fleet_morphologies():
    return [default_hexapod_params("tripod"), synthetic_octopod_params("ripple", 5, 8), synthetic_octopod_params("amble", 4, 4)]


def fleet_views(fleet):
    return [(BatchEngine.view(handle, fleet.params[m], len(ids)), ids) for handle, m, _, ids in fleet.parts()]


def test_fleet():
    need_gpu()
    import torch
    a = MixedFleet(fleet_morphologies(), FLEET_MORPH, (0,))
    try:
        assert (a.max_legs, a.max_dof) == (8, 5)
        rng = np.random.default_rng(14)
        a.set_velocity(rng.uniform(-0.4, 0.4, (FLEET_N, 2)), rng.uniform(-0.4, 0.4, FLEET_N))
        a.step(40)
        a.synchronize()
        tips = np.full((FLEET_N, 8, 3), SENTINEL)     # (the legs a robot lacks: never read into a result)
        for view, ids in fleet_views(a):
            tips[ids, :view.legs] = view.leg_apply_fk()[:, :3].reshape(len(ids), view.legs, 3)
        targets = candidates(tips, far=0.45)
        records = [(state_bytes(v), bytes(v.get_aux_state())) for v, _ in fleet_views(a)]
        S, fields = 8, ("fraction", "q", "tip", "limit_proximity")
        D = reach_columns(fields, 8, 5)[1]
        for dtype in ("float64", "float32"):
            d_targets = upload(targets, dtype)
            out = a.probe_reach(d_targets, S, fields, pad=-2.5)
            held = a.io_nbytes
            assert held > 0
            a.synchronize()
            got = out.cpu().numpy()
            assert got.shape == (FLEET_N, 3, D)
            again = a.probe_reach(d_targets, S, fields, pad=-2.5)
            a.synchronize()
            assert a.io_nbytes == held, "the probe allocated staging"
            assert again.cpu().numpy().tobytes() == got.tobytes()
            # every row is the part's own engine call, byte for byte, in the caller's order
            seen = np.zeros(FLEET_N, dtype=bool)
            for view, ids in fleet_views(a):
                own = view.probe_reach(upload(targets[ids], dtype), S, fields, pad=-2.5, legs=8, dof=5)
                view.synchronize()
                assert own.cpu().numpy().tobytes() == np.ascontiguousarray(got[ids]).tobytes(), f"part of {view.legs} legs"
                block = split(got[ids], fields, 8, 5)
                assert (block["fraction"][:, :, view.legs:] == -2.5).all() and (block["q"][:, :, :, view.dof:] == -2.5).all()
                assert (block["fraction"][:, 0, :view.legs] > 0).any()
                seen[ids] = True
            assert seen.all()
            # a producer on the caller's stream, order_after, the probe, order_before, a consumer on that stream: the calls compose
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                made = d_targets * 1.0
            a.order_after(s)
            ordered = a.probe_reach(made, S, fields, pad=-2.5)
            a.order_before(s)
            with torch.cuda.stream(s):
                copy = ordered.clone()
            s.synchronize()
            assert copy.cpu().numpy().tobytes() == got.tobytes()
        assert [(state_bytes(v), bytes(v.get_aux_state())) for v, _ in fleet_views(a)] == records, "the probe wrote into a part"
        with pytest.raises(ValueError):
            a.probe_reach(upload(targets[:-1]), S, fields)           # a fleet takes every robot
        with pytest.raises(ValueError):
            a.probe_reach(upload(targets[:, :, :6]), S, fields)      # the fleet's row geometry is 8 legs
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_a_fleet_on_two_devices_is_refused():
    need_gpu()
    if device_count() < 2:
        pytest.skip("one device")
    import torch
    a = MixedFleet(fleet_morphologies(), FLEET_MORPH, (0, 1))
    try:
        width = reach_columns(("fraction", "tip"), 8, 5)[1]
        t = torch.full((FLEET_N, 3, 8, 3), 0.25, dtype=torch.float32, device="cuda")
        out = torch.full((FLEET_N, 3, width), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        spec = reach_spec(("fraction", "tip"), 8, 5, 3, 16)
        assert a.L.shc_fleet_probe_reach_device(a.h, C.byref(spec), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())) == SHC_ERR_UNSUPPORTED
        assert a.io_nbytes == 0
        a.synchronize()
        assert (out.cpu().numpy() == np.float32(SENTINEL)).all()
    finally:
        a.close()


def spec_cases(legs, dof, width):
    ok = lambda **kw: reach_spec(("fraction", "tip"), legs, dof, **{"candidates": 3, "steps": 16, **kw})
    cases = {}
    for what, member, value in (("no field", "n_fields", 0), ("five fields", "n_fields", 5), ("an unknown dtype", "dtype", 2), ("reserved != 0", "reserved", 1)):
        s = ok()
        setattr(s, member, value)
        cases[what] = s
    cases["an unknown field"] = reach_spec((0, 4), legs, dof, 3, 16)
    cases["a repeated field"] = reach_spec(("tip", "tip"), legs, dof, 3, 16)
    cases["legs below the shape"] = reach_spec(("fraction", "tip"), legs - 1, dof, 3, 16)
    cases["dof below the shape"] = reach_spec(("fraction", "tip"), legs, dof - 1, 3, 16)
    cases["legs above SHC_MAX_LEGS"] = reach_spec(("fraction", "tip"), 9, dof, 3, 16)
    cases["no candidate"], cases["65 candidates"] = ok(candidates=0), ok(candidates=65)
    cases["no step"], cases["4097 steps"] = ok(steps=0), ok(steps=4097)
    cases["a row stride below C x D"] = ok(row_stride=3 * width - 1)
    cases["a target row stride below C x legs x 3"] = ok(target_row_stride=3 * legs * 3 - 1)
    return ok, cases


def test_engine_refusals(hexapods):
    import torch
    eng, _twin, targets = hexapods
    lib, n = eng.L, eng.n
    width = reach_columns(("fraction", "tip"), 6, 3)[1]
    t = upload(targets, "float32")
    out = torch.full((n, 3, width), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = everything(eng)
    ok, cases = spec_cases(6, 3, width)

    def call(spec, first=0, count=n, h=None, tp=None, op=None):
        return lib.shc_engine_probe_reach(eng.h if h is None else h, first, count, None if spec is None else C.byref(spec),
                                          C.c_void_p(t.data_ptr() if tp is None else tp), C.c_void_p(out.data_ptr() if op is None else op))
    for what, spec in cases.items():
        assert call(spec) == SHC_ERR_INVALID_ARG, what
        assert lib.shc_last_error(), what
    assert lib.shc_engine_probe_reach(None, 0, n, C.byref(ok()), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())) == SHC_ERR_INVALID_ARG
    assert call(None) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_probe_reach(eng.h, 0, n, C.byref(ok()), None, C.c_void_p(out.data_ptr())) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_probe_reach(eng.h, 0, n, C.byref(ok()), C.c_void_p(t.data_ptr()), None) == SHC_ERR_INVALID_ARG
    for first, count in ((-1, 2), (0, n + 1), (n, 1), (n + 1, 0), (5, -1), (20, 4)):
        assert call(ok(), first, count) == SHC_ERR_INVALID_ARG, (first, count)
    assert call(ok(), tp=t.data_ptr() + 2) == SHC_ERR_INVALID_ARG and call(ok(), op=out.data_ptr() + 2) == SHC_ERR_INVALID_ARG   # not aligned to a float
    assert call(ok(dtype="float64"), tp=t.data_ptr() + 4) == SHC_ERR_INVALID_ARG
    assert call(ok(), 7, 0) == SHC_OK and call(ok(), n, 0) == SHC_OK                      # count = 0 is a no-op
    # what the Python layer refuses itself
    with pytest.raises(ValueError):
        eng.probe_reach(t[:-1], 16)
    with pytest.raises(ValueError):
        eng.probe_reach(t, 16, ("fraction", "tip"), out=out[:, :, :width - 1])
    with pytest.raises(ValueError):
        eng.probe_reach(t.transpose(1, 2), 16)
    with pytest.raises(TypeError):
        eng.probe_reach(t.to(torch.float16), 16)
    with pytest.raises(TypeError):
        eng.probe_reach(t.cpu().numpy(), 16)
    with pytest.raises(ShcError):
        eng.probe_reach(t, 0)
    with pytest.raises(ShcError):
        eng.probe_reach(t, 16, ("tip", "tip"))
    eng.synchronize()
    assert out.cpu().numpy().tobytes() == np.full((n, 3, width), SENTINEL, dtype=np.float32).tobytes(), "a refused call wrote into out"
    assert everything(eng) == before
    eng.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert call(ok()) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    eng.synchronize()
    assert out.cpu().numpy().tobytes() == np.full((n, 3, width), SENTINEL, dtype=np.float32).tobytes()
    assert call(ok()) == SHC_OK                                                           # ... and the handle still works
    eng.synchronize()
    assert (out.cpu().numpy() != np.float32(SENTINEL)).all()


def test_fleet_refusals():
    need_gpu()
    import torch
    a = MixedFleet(fleet_morphologies(), FLEET_MORPH, (0,))
    try:
        lib = a.L
        width = reach_columns(("fraction", "tip"), 8, 5)[1]
        t = torch.full((FLEET_N, 3, 8, 3), 0.25, dtype=torch.float32, device="cuda")
        out = torch.full((FLEET_N, 3, width), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ok, cases = spec_cases(8, 5, width)

        def call(spec, tp=None, op=None):
            return lib.shc_fleet_probe_reach_device(a.h, None if spec is None else C.byref(spec), C.c_void_p(t.data_ptr() if tp is None else tp),
                                                    C.c_void_p(out.data_ptr() if op is None else op))
        for what, spec in cases.items():
            assert call(spec) == SHC_ERR_INVALID_ARG, what
            assert lib.shc_last_error(), what
        assert lib.shc_fleet_probe_reach_device(None, C.byref(ok()), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())) == SHC_ERR_INVALID_ARG
        assert call(None) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_probe_reach_device(a.h, C.byref(ok()), None, C.c_void_p(out.data_ptr())) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_probe_reach_device(a.h, C.byref(ok()), C.c_void_p(t.data_ptr()), None) == SHC_ERR_INVALID_ARG
        assert call(ok(), tp=t.data_ptr() + 2) == SHC_ERR_INVALID_ARG and call(ok(), op=out.data_ptr() + 2) == SHC_ERR_INVALID_ARG
        assert a.io_nbytes == 0                                                           # nobody got as far as preparing device I/O
        hexapods_ = fleet_views(a)[0][0]
        hexapods_.resident_begin(ring_depth=4, max_cycles=100)
        try:
            assert call(ok()) == SHC_ERR_BUSY
        finally:
            hexapods_.resident_end()
        a.synchronize()
        assert out.cpu().numpy().tobytes() == np.full((FLEET_N, 3, width), SENTINEL, dtype=np.float32).tobytes(), "a refused call wrote into out"
        assert call(ok()) == SHC_OK
        a.synchronize()
        assert a.io_nbytes > 0
    finally:
        a.close()
