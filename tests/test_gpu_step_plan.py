"""GPU (-m gpu): the step plan pass (include/shc_step_plan.h: shc_engine_get_step_plan, shc_fleet_get_step_plan_device;
BatchEngine.step_plan, MixedFleet.step_plan) against its definition restated in numpy (tests/plan_numpy.py, which tests/
test_step_plan_reference.py holds to the CPU oracle) on the records shc_engine_get_state returns, to 1e-12 - the teacher-forced tolerance of this
suite - with pad positions compared exactly; and against what the cycle kernel then does: sample h of SHC_PLAN_PATH must be the walker tip h
cycles later."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plan_numpy as pn
from syropod_highlevel_controller_amd import default_hexapod_params, engine, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (PLAN_FIELD_NAMES, SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_OK, BatchEngine, ShcError, device_count,
                                                     foothold_columns, plan_columns, plan_spec)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_fleet_device_io import views
from test_gpu_footholds import ALL as FH_ALL, TARGET, records as target_records, requests, rough, walking
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

ALL = tuple(PLAN_FIELD_NAMES)
TOL = 1e-12
H = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def need_gpu():
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")


def assert_rows(got, want, what):
    """got: the pass, float64; want: plan_numpy.rows with a NaN pad.  NaN exactly where want is NaN, elsewhere within TOL."""
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: pad and value disagree at (row, column) {tuple(np.argwhere(np.isnan(got) != nan)[0])}"
    err = np.abs(got[~nan] - want[~nan]).max(initial=0.0)
    assert err <= TOL, f"{what}: max |pass - definition| = {err:.3e}"
    return err


def definition(eng, fields, legs, horizon, first=0, count=None, **more):
    return pn.rows(eng.get_state(first, count), eng.params, eng.tables(), fields, legs, horizon, **more)


def to_the_window(robots, n, period, seed=5):
    """The drive of tests/test_step_plan_reference.py with four kinds of robot, i mod 4: 0 never commanded; 1 commanded from the start (MOVING in
    the window); 2 commanded when the window opens (STARTING in it); 3 commanded from the start and told to stop when the window opens
    (STOPPING in it).  `robots` is a BatchEngine or an OracleBatch.  The window is the `period` cycles that follow."""
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
    kind = np.arange(n) % 4
    early = (kind == 1) | (kind == 3)
    robots.set_velocity(lin * early[:, None], ang * early)
    robots.step(2 * period + 30)
    late = (kind == 1) | (kind == 2)
    robots.set_velocity(lin * late[:, None], ang * late)


# ------------------------------------------------------------------------------------------------------------ 1. hexapods, every cycle of a period
@pytest.fixture(scope="module")
def hexapods():
    """23 hexapods: two full robot groups of 10 and one of 3.  Compared after every cycle of one step period, then left mid-walk for the tests below."""
    need_gpu()
    p = default_hexapod_params("tripod")
    n = 23
    eng = BatchEngine(p, n)
    tables = eng.tables()
    period = int(tables.step.period)
    to_the_window(eng, n, period)
    seen, worst, failures = {k: 0 for k in pn.KINDS}, 0.0, []
    for c in range(period):
        eng.step(1)
        got = eng.step_plan(ALL, H, dtype="float64")
        state = eng.get_state()
        try:
            worst = max(worst, assert_rows(got, pn.rows(state, p, tables, ALL, 6, H), f"hexapods, cycle {c} of the window"))
        except AssertionError as e:            # (judged by the test below: a fixture that raises would hide which test it is about)
            failures.append(str(e))
        for k, m in pn.kinds(pn.plan(state, p, tables)).items():
            seen[k] += int(m.sum())
    yield eng, seen, worst, failures
    eng.close()


def test_hexapods_every_field_every_cycle_of_a_period(hexapods):
    eng, seen, worst, failures = hexapods
    assert not failures, f"{len(failures)} of the period's cycles differ, the first: {failures[0]}"
    print(f"[step plan] 23 hexapods x one period, every field, H = {H}: max |pass - definition| = {worst:.3e}; (leg, cycle) samples by kind: {seen}")
    assert all(seen[k] > 0 for k in pn.KINDS), seen
    got = eng.step_plan(ALL, H, dtype="float64")
    cols, width = plan_columns(ALL, 6, H)
    assert width == 6 * (3 * 15 + 4 * 3 + 2 + 3 * H) + 6
    it = got[:, cols["iteration"]]
    assert np.isnan(it[0::4]).all() and np.isfinite(it[1::4]).all()            # never commanded: every curve is pad; MOVING: every leg has one
    s1, st = got[:, cols["swing_1_nodes"]].reshape(23, 6, 15), got[:, cols["stance_nodes"]].reshape(23, 6, 15)
    moving = np.arange(23) % 4 == 1
    assert (np.isnan(s1[moving]).all(-1) != np.isnan(st[moving]).all(-1)).all()   # a stepping leg has the curves of its period and not the others
    assert np.isfinite(got[:, cols["default_tip"]]).all() and np.isfinite(got[:, cols["swing_clearance"]]).all()


# ------------------------------------------------------------------------------------------------------------ 2. the prediction against the cycle kernel
def test_the_path_is_what_the_cycle_kernel_then_does():
    """Robots at constant linear velocity and zero angular velocity on flat ground, three periods in: the curves then stay as they are, so sample h
    of the path taken after the first iteration of a swing is the walker tip after h more cycles.  No restatement is involved: this holds the
    node formulas of shc_step_plan.hpp to those of the cycle kernel."""
    need_gpu()
    p = default_hexapod_params("tripod")
    n = 12
    eng = BatchEngine(p, n)
    period = int(eng.tables().step.period)
    lin = np.random.default_rng(9).uniform(-0.5, 0.5, (n, 2))
    eng.set_velocity(lin, np.zeros(n))
    eng.step(3 * period)
    fields = ("iteration", "iterations", "swing_1_nodes", "path")
    cols, _ = plan_columns(fields, 6, H)
    for _ in range(period):                                                     # on to the first iteration of somebody's swing
        eng.step(1)
        plan = eng.step_plan(fields, H, dtype="float64")
        first = (plan[:, cols["iteration"]] == 1.0) & np.isfinite(plan[:, cols["swing_1_nodes"]].reshape(n, 6, 15)).all(-1)
        if first.any():
            break
    assert first.any(), "no leg began a swing within a period"
    path = plan[:, cols["path"]].reshape(n, 6, H, 3)
    left = (plan[:, cols["iterations"]] - plan[:, cols["iteration"]])           # cycles left in the running period
    assert (left[first] >= H).all() and np.isfinite(path[first]).all()          # a swing has 52 iterations: all 16 samples lie inside
    worst, compared = 0.0, 0
    for h in range(1, H + 1):
        eng.step(1)
        tip = eng.observations(("walker_tip",), dtype="float64").reshape(n, 6, 3)
        inside = left >= h                                                      # every leg, swinging or in stance, while its period lasts
        assert (np.isfinite(path[:, :, h - 1]).all(-1) == inside).all()
        worst = max(worst, float(np.abs(path[:, :, h - 1][inside] - tip[inside]).max()))
        compared += int(inside.sum())
    print(f"[step plan] path sample h against the walker tip h cycles later, h = 1 .. {H}: max |d| = {worst:.3e} m over {compared} samples, "
          f"{int(first.sum())} legs at the first iteration of a swing")
    assert worst <= TOL
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 3. float32, sub-range, layout
def test_float32_is_the_cast_of_float64(hexapods):
    eng = hexapods[0]
    f64, f32 = eng.step_plan(ALL, H, dtype="float64"), eng.step_plan(ALL, H, dtype="float32")
    assert f32.dtype == np.float32 and f32.shape == f64.shape
    want = f64.astype(np.float32)
    nan = np.isnan(want)
    assert (np.isnan(f32) == nan).all() and nan.any() and (f32.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_sub_range_into_columns_of_a_wider_tensor_and_a_permuted_subset(hexapods, dtype):
    import torch
    eng = hexapods[0]
    whole = eng.step_plan(ALL, H, dtype="float64", pad=-3.5)
    all_cols, _ = plan_columns(ALL, 6, H)
    first, count = 3, 15                                                        # starts and ends inside a robot group
    tdt = torch.float64 if dtype == "float64" else torch.float32
    for fields, horizon in ((ALL, H), (("path", "walk_plane_normal", "stance_nodes", "iteration", "stride_vector", "swing_2_nodes"), H),
                            (("swing_clearance", "target_tip"), 0)):
        cols, D = plan_columns(fields, 6, horizon)
        big = torch.full((count, D + 11), 1e30, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        assert eng.step_plan(fields, horizon, out=big[:, 5:5 + D], first=first, count=count, pad=-3.5) is None
        eng.synchronize()
        got = big.cpu().numpy()
        assert (np.delete(got, np.s_[5:5 + D], axis=1) == np.array(1e30, dtype=got.dtype)).all(), "columns outside [0, width) of a row were written"
        for name in fields:
            want = whole[first:first + count, all_cols[name]].astype(got.dtype)
            assert got[:, 5:5 + D][:, cols[name]].tobytes() == want.tobytes(), (name, dtype)
    host = eng.step_plan(("path", "default_tip"), 5, dtype=dtype, first=first, count=count, pad=-3.5)   # a shorter horizon: the first samples
    cols, _ = plan_columns(("path", "default_tip"), 6, 5)
    want = whole[first:first + count, all_cols["path"]].reshape(count, 6, H, 3)[:, :, :5].reshape(count, -1).astype(host.dtype)
    assert host[:, cols["path"]].tobytes() == want.tobytes()


def test_the_library_call_with_a_row_stride_on_the_host(hexapods):
    eng = hexapods[0]
    fields = ("stance_nodes", "walk_plane", "iterations")
    cols, W = plan_columns(fields, 6, 0)
    out = np.full((23, W + 3), -5.0)
    spec = plan_spec(fields, 6, 0, "float64", W + 3)
    assert eng.L.shc_engine_get_step_plan(eng.h, 0, 23, C.byref(spec), out.ctypes.data_as(C.c_void_p), 0) == SHC_OK
    assert_rows(out[:, :W], definition(eng, fields, 6, 0), "host form with a row stride")
    assert (out[:, W:] == -5.0).all()


# ------------------------------------------------------------------------------------------------------------ 4. morphologies, the chunked tile
MORPHS = {"8x5": (lambda: synthetic_octopod_params("ripple", 5, 8), 9, 8),                       # 8 robots per wavefront: two groups
          "3 legs in the 8-leg geometry": (lambda: synthetic_octopod_params("wave", 3, 3), 22, 8),   # 21 per wavefront; every field, H = 16, float64: the
                                                                                                     # row is served in runs of fields through the tile
          "mixed DOF": (lambda: synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4)), 9, 8)}


@pytest.mark.parametrize("morph", list(MORPHS))
def test_morphologies_and_padding(morph):
    need_gpu()
    make, n, legs = MORPHS[morph]
    p = make()
    eng = BatchEngine(p, n)
    tables = eng.tables()
    period, L = int(tables.step.period), p.leg_count
    to_the_window(eng, n, period)
    seen = {k: 0 for k in pn.KINDS}
    cols, width = plan_columns(ALL, legs, H)
    for c in range(0, period, 13):                                              # nine states spread over the window
        eng.step(13)
        state = eng.get_state()
        got = eng.step_plan(ALL, H, dtype="float64", legs=legs)
        assert_rows(got, pn.rows(state, p, tables, ALL, legs, H), f"{morph}, cycle {c + 13} of the window")
        for k, m in pn.kinds(pn.plan(state, p, tables)).items():
            seen[k] += int(m.sum())
    assert all(seen[k] > 0 for k in ("swing_first_half", "swing_second_half", "stance_standard", "not_stepping")), seen
    for name in ALL:                                                            # the legs the robot lacks hold the pad, also a numeric one
        if name not in pn.ROBOT_FIELDS:
            assert np.isnan(got[:, cols[name]].reshape(n, legs, -1)[:, L:]).all() and np.isfinite(got[:, cols["target_tip"]].reshape(n, legs, 3)[:, :L]).all()
    f32 = eng.step_plan(ALL, H, dtype="float32", legs=legs, pad=-2.5)
    want = pn.rows(eng.get_state(), p, tables, ALL, legs, H, pad=-2.5)
    assert ((f32 == np.float32(-2.5)) == (want == -2.5)).all()
    assert np.abs(f32.astype(np.float64) - want).max() <= 1e-6                  # (float32 holds the cast: the bits are held in the hexapod test)
    if legs > L:
        import torch
        big = torch.full((n, width + 7), 1e30, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.step_plan(ALL, H, out=big[:, 3:3 + width], legs=legs)
        eng.synchronize()
        dev = big.cpu().numpy()
        assert np.array_equal(dev[:, 3:3 + width], got, equal_nan=True) and (np.delete(dev, np.s_[3:3 + width], axis=1) == 1e30).all()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 5. rough terrain mode
def test_rough_terrain_external_targets_and_ground_contact():
    """The scenario of tests/test_gpu_footholds.py: hexapods in rough terrain mode, tip forces that put every leg in ground contact (step plane
    defined), then a tip-target request for every leg, every third in the odom_ideal frame, each with a clearance of its own that is not the
    swing height (0.02 m): 0.023, 0.026 .. 0.038 m on legs 0 .. 5.  Every cycle of a period; wherever a leg swings towards such a target the
    SWING_CLEARANCE column itself must have the target's length, not the parameter's."""
    (eng,), tips = walking(rough(default_hexapod_params("tripod")), 23, 8, count=1)
    try:
        p, tables = eng.params, eng.tables()
        rows = requests(tips, FH_ALL, 6, seed=1)
        own_clearance = 0.02 + 0.003 * (np.arange(6) + 1.0)
        rows[:, foothold_columns(FH_ALL, 6)[0]["swing_clearance"]] = own_clearance      # (one column per leg)
        assert abs(p.swing_height - 0.02) < 1e-12 and np.abs(own_clearance - p.swing_height).min() > 2e-3
        assert eng.set_footholds(rows, FH_ALL, TARGET, "request", legs=6) == 0    # (a STOPPED robot's go to its poser)
        seen = {"external target in a swing": 0, "ground contact in the second half": 0, "a swing without an external target": 0}
        fields = tuple(f for f in ALL if f != "path") + ("path",)
        clearance_at = plan_columns(fields, 6, H)[0]["swing_clearance"]
        for c in range(int(tables.step.period)):
            eng.step(1)
            got = eng.step_plan(fields, H, dtype="float64")
            state, ext = eng.get_state(), target_records(eng, TARGET)
            more = {"ext_defined": ext["defined"] != 0, "ext_clearance": ext["swing_clearance"]}
            assert_rows(got, pn.rows(state, p, tables, fields, 6, H, **more), f"rough terrain, cycle {c}")
            o = pn.plan(state, p, tables, **more)
            contact = pn.records(state)["leg"][:, :6]["step_plane_defined"] != 0
            seen["external target in a swing"] += int((more["ext_defined"] & o.swing).sum())
            # the column itself, not through the restatement: the target's clearance where a leg swings towards one, the swing height elsewhere
            length = np.linalg.norm(got[:, clearance_at].reshape(23, 6, 3), axis=-1)
            mine = more["ext_defined"] & o.swing
            assert (ext["swing_clearance"][mine] == np.broadcast_to(own_clearance, (23, 6))[mine]).all()
            assert np.abs(length[mine] - np.broadcast_to(own_clearance, (23, 6))[mine]).max(initial=0.0) <= 1e-15
            assert np.abs(length[~mine] - p.swing_height).max() <= 1e-15
            seen["a swing without an external target"] += int((o.swing & ~more["ext_defined"]).sum())
            seen["ground contact in the second half"] += int((contact & o.swing & ~o.first_half).sum())
        assert all(v > 0 for v in seen.values()), seen
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ 6. no side effects, refusals
def test_the_pass_changes_no_state(hexapods):
    eng = hexapods[0]
    eng.synchronize()
    before = state_bytes(eng), eng.get_aux_state()
    for dtype, kw in (("float64", {}), ("float32", {"first": 7, "count": 11}), ("float64", {"legs": 8})):
        assert np.isfinite(eng.step_plan(ALL, H, dtype=dtype, **kw)).any()
        assert (state_bytes(eng), eng.get_aux_state()) == before, "the step plan pass changed a state record or an auxiliary blob"


def test_engine_refusals_write_nothing(hexapods):
    import torch
    eng = hexapods[0]
    L, n = eng.L, eng.n
    fields = ("stride_vector", "walk_plane")
    W = 21
    out = torch.full((n, W + 4), 1e30, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = out.data_ptr()
    call = lambda spec, first=0, count=n, p=ptr, h=eng.h: L.shc_engine_get_step_plan(h, first, count, None if spec is None else C.byref(spec), p, 1)
    good = lambda **kw: plan_spec(fields, 6, 0, "float64", W + 4, **kw)
    assert call(good(), h=None) == SHC_ERR_INVALID_ARG and call(None) == SHC_ERR_INVALID_ARG and call(good(), p=None) == SHC_ERR_INVALID_ARG
    for bad in (plan_spec((), 6), plan_spec((0, 12), 6), plan_spec(("path", "path"), 6, 4), plan_spec(fields, 6, 0, 2), plan_spec(fields, 5), plan_spec(fields, 9),
                plan_spec(fields, 6, 0, "float64", W - 1), plan_spec(fields, 6, 17), plan_spec(fields, 6, -1), plan_spec(fields + ("path",), 6, 0),
                plan_spec(("path",), 6, 17)):
        assert call(bad) == SHC_ERR_INVALID_ARG
    s = good()
    s.reserved = 1
    assert call(s) == SHC_ERR_INVALID_ARG
    for first, count in ((-1, 3), (0, n + 1), (n, 1), (5, -1), (n + 1, 0)):
        assert call(good(), first, count) == SHC_ERR_INVALID_ARG, (first, count)
    assert call(good(), p=ptr + 4) == SHC_ERR_INVALID_ARG                                   # float64 needs 8 bytes
    assert call(plan_spec(fields, 6, 0, "float32", 2 * (W + 4)), p=ptr + 2) == SHC_ERR_INVALID_ARG   # float32 needs 4
    assert call(good(), first=n, count=0) == SHC_OK and call(good(), count=0) == SHC_OK     # count = 0: a no-op
    assert call(plan_spec(fields, 6, 16, "float64", W + 4)) == SHC_OK                       # the horizon is ignored without the path ...
    eng.synchronize()
    assert_rows(out.cpu().numpy()[:, :W], definition(eng, fields, 6, 0), "a horizon without the path")
    out.fill_(1e30)
    torch.cuda.synchronize()
    with pytest.raises(ShcError):
        eng.step_plan(("path",), 0)
    with pytest.raises(ShcError):
        eng.step_plan(("path",), 17)
    with pytest.raises(ValueError):
        eng.step_plan(fields, out=out[:5])                                                  # rows
    with pytest.raises(ValueError):
        eng.step_plan(fields, out=out[:, :W - 1])                                           # columns
    with pytest.raises(ValueError):
        eng.step_plan(fields, out=np.zeros((n, W)))                                         # a host array
    eng.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert call(good()) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    eng.synchronize()
    assert (out.cpu().numpy() == 1e30).all(), "a refused call wrote to the buffer"
    assert call(good()) == SHC_OK                                                           # ... and the handle still works
    eng.synchronize()
    assert_rows(out.cpu().numpy()[:, :W], definition(eng, fields, 6, 0), "after the refusals")


# ------------------------------------------------------------------------------------------------------------ 7. the fleet
def test_fleet_rows_are_the_parts_engine_rows_in_the_callers_order():
    import torch
    need_gpu()
    morph = np.array([0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0], dtype=np.int32)   # 13 hexapods, 10 octopods, interleaved
    n = len(morph)
    fleet = MixedFleet([default_hexapod_params("tripod"), synthetic_octopod_params("ripple", 5, 8)], morph)
    try:
        assert fleet.max_legs == 8
        rng = np.random.default_rng(4)
        lin, ang = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
        lin[::5], ang[::5] = 0.0, 0.0
        fleet.set_velocity(lin, ang)
        fleet.step(170)
        fleet.synchronize()
        fields = ("path", "walk_plane_normal", "swing_1_nodes", "stance_nodes", "swing_2_nodes", "iteration", "target_tip")
        cols, D = plan_columns(fields, 8, 12)
        held = None
        for dtype in (torch.float64, torch.float32):
            big = torch.full((n, D + 9), 1e30, dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            fleet.step_plan(big[:, 4:4 + D], fields, 12)
            fleet.synchronize()
            held = fleet.io_nbytes if held is None else held      # (the fleet's first device I/O call puts the caller ids on the device)
            assert fleet.io_nbytes == held, "the step plan pass allocated staging"
            got = big.cpu().numpy()
            assert (np.delete(got, np.s_[4:4 + D], axis=1) == np.array(1e30, dtype=got.dtype)).all()
            rows, covered = got[:, 4:4 + D], np.zeros(n, dtype=bool)
            for view, ids in views(fleet):
                part = view.step_plan(fields, 12, dtype=got.dtype, legs=8)
                assert np.array_equal(rows[ids], part, equal_nan=True), f"the rows of the {view.legs}-leg part differ from its engine's"
                if got.dtype == np.float64:
                    assert_rows(part, definition(view, fields, 8, 12), f"the {view.legs}-leg part")
                covered[ids] = True
            assert covered.all() and np.isfinite(rows[:, cols["target_tip"]].reshape(n, 8, 3)[morph == 1]).all()
            assert np.isnan(rows[:, cols["target_tip"]].reshape(n, 8, 3)[morph == 0][:, 6:]).all()
        out = torch.full((n, D), 1e30, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        call = lambda spec, p=out.data_ptr(), h=fleet.h: fleet.L.shc_fleet_get_step_plan_device(h, None if spec is None else C.byref(spec), p)
        assert call(plan_spec(fields, 8, 12, "float64"), h=None) == SHC_ERR_INVALID_ARG and call(None) == SHC_ERR_INVALID_ARG
        assert call(plan_spec(fields, 7, 12, "float64")) == SHC_ERR_INVALID_ARG                    # below shc_fleet_shape
        assert call(plan_spec(fields, 8, 0, "float64")) == SHC_ERR_INVALID_ARG and call(plan_spec(fields, 8, 17, "float64")) == SHC_ERR_INVALID_ARG
        assert call(plan_spec(fields, 8, 12, "float64", D - 1)) == SHC_ERR_INVALID_ARG
        hexapods = views(fleet)[0][0]
        hexapods.resident_begin(ring_depth=4, max_cycles=100)
        try:
            assert call(plan_spec(fields, 8, 12, "float64")) == SHC_ERR_BUSY
        finally:
            hexapods.resident_end()
        fleet.synchronize()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 1e30).all(), "a refused call wrote to the buffer"
        assert fleet.io_nbytes == held
    finally:
        fleet.close()


# ------------------------------------------------------------------------------------------------------------ 8. the façade
def test_facade_getters_are_the_columns_of_the_pass(tmp_path):
    need_gpu()
    so = engine.build_library()
    exe = str(tmp_path / "facade_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "facade_plan_main.cpp"),
                           so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = default_hexapod_params("tripod")
    pfile = str(tmp_path / "params.bin")
    open(pfile, "wb").write(bytes(p))
    cycles, v = 170, (0.3, -0.2, 0.25)
    out = subprocess.check_output([exe, pfile, str(cycles), *map(str, v)], text=True).strip().split("\n")
    assert "node 5 refused" in out
    # 1. every getter is the pass's column for that leg and component: the row the program read from its own engine in one call, bit for bit
    fields = tuple(f for f in ALL if f not in ("path", "iteration", "iterations"))
    cols, width = plan_columns(fields, 6)
    own = np.array([float(x) for x in next(line for line in out if line.startswith("row ")).split()[1:]])
    assert own.shape == (width,)
    lines = [line.split() for line in out if line.split()[0] in fields]
    assert len(lines) == 6 * (15 + 6)
    finite = 0
    for name, leg, i, *xyz in lines:
        leg, i, xyz = int(leg), int(i), np.array([float(x) for x in xyz])
        block = own[cols[name]] if name in pn.ROBOT_FIELDS else own[cols[name]].reshape(6, -1)[leg]
        assert np.array_equal(xyz, block[3 * i:3 * i + 3], equal_nan=True), (name, leg, i)
        finite += int(np.isfinite(xyz).all())
    assert 6 * (5 + 6) < finite < len(lines)                                   # a curve per leg at least, and some pad
    # 2. ... and that row is the plan of a robot walked the same way by an engine of this process (free-running: the tolerance of smoke())
    eng = BatchEngine(p, 1)
    try:
        eng.set_velocity(np.array([[v[0], v[1]]]), np.array([v[2]]))
        for _ in range(cycles):                                                # the façade's loop: one cycle per updateWalk / updateModel
            eng.step(1)
        row = eng.step_plan(fields, dtype="float64")[0]
        assert (np.isnan(row) == np.isnan(own)).all() and np.abs(row - own)[np.isfinite(own)].max() <= 1e-6
    finally:
        eng.close()
