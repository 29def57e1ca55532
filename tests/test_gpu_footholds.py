"""GPU (-m gpu): the foothold pass (shc_engine_set_footholds / _get_footholds, shc_fleet_set_footholds_device / _get_footholds_device;
BatchEngine.set_footholds / footholds, MixedFleet.set_footholds / footholds) against its definition, the three host calls
shc_engine_set_external_target / _set_external_transform / _get_external_target.  Always twins: two engines built from the same parameters and
driven identically; A takes the new call with one tensor, B the host calls with ExternalTarget rows built from tensor.double().  Then the state
records and auxiliary blobs, the three records as the host getter returns them and the counts of dropped rows are equal, and so are the bit
patterns of the joints 40 cycles later.  The pass converts and moves values: every comparison is equality of bytes."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (FH_FIELD_NAMES, SHC_ERR_BUSY, SHC_ERR_INVALID_ARG, SHC_ERR_UNSUPPORTED, SHC_OK, BatchEngine, ShcError,
                                                     device_count, foothold_columns, foothold_spec, generate_tables)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from syropod_highlevel_controller_amd.params import ExternalTarget
from test_gpu_fleet_device_io import MORPH, N, ML, LEGS, morphologies, robot_records, views
from test_gpu_resident import state_bytes

pytestmark = pytest.mark.gpu

ALL = tuple(FH_FIELD_NAMES)
PERMUTED = ("defined", "transform", "position", "frame_is_odom_ideal", "rotation", "swing_clearance")
TARGET, DEFAULT, PLANNER = 0, 1, 2
SENTINEL = 1e30
SENTINEL_BYTES = (np.float64(SENTINEL).tobytes(), np.float64(np.float32(SENTINEL)).tobytes())   # as a double, given as float64 or as float32
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
ET = np.dtype({"names": [k for k, _ in ExternalTarget._fields_], "formats": [(np.float64, 7), (np.float64, 7), np.float64, np.int32, np.int32],
               "offsets": [getattr(ExternalTarget, k).offset for k, _ in ExternalTarget._fields_], "itemsize": C.sizeof(ExternalTarget)})


def need_gpu():
    if device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")


def walking(p, n, seed, count=2, stopped=5):
    """`count` engines of n robots driven alike, the recipe of the rough-terrain case of test_gpu_checkpoint.py: velocities U(-0.4, 0.4), 50
    cycles, z tip forces U(5, 25), 15 cycles - with the velocities of the first `stopped` robots zero, so that they are STOPPED.  Returns the
    engines and the walker tips (n, L, 3)."""
    need_gpu()
    L = p.leg_count
    t = generate_tables(p)
    engines = [BatchEngine(p, n, tables=t) for _ in range(count)]
    rng = np.random.default_rng(seed)
    lin, ang = rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.4, 0.4, n)
    lin[:stopped], ang[:stopped] = 0.0, 0.0
    force = np.zeros((n, L, 3))
    force[:, :, 2] = rng.uniform(5.0, 25.0, (n, L))
    for e in engines:
        e.set_velocity(lin, ang)
        e.step(50)
        e.set_tip_force(force)
        e.step(15)
        e.synchronize()
    assert len({state_bytes(e) for e in engines}) == 1
    tips = engines[0].leg_state()["walker_tip"].reshape(n, L, 3)
    for e in engines[1:]:   # (leg_state() refreshes the derived tips, which the auxiliary blob carries)
        e.leg_state()
    return engines, tips


def rough(p):
    p.rough_terrain_mode = 1
    return p


def requests(tips, fields, legs, seed=0, rotation=None, defined=None):
    """A float64 (n, F) row set for `fields` in the row geometry `legs`: targets = walker tip + (0.02, -0.01, 0), rotation 1 0 0 0 (or the
    (n, L, 4) given), a transform near the identity, clearance 0.02, every third leg in the odom_ideal frame, and SENTINEL in every column of
    a leg >= L.  defined: the (n, L) column to use instead of ones."""
    n, L = tips.shape[:2]
    rng = np.random.default_rng(1000 + seed)
    cols, width = foothold_columns(fields, legs)
    rows = np.full((n, width), SENTINEL)
    transform = np.tile(np.array(IDENTITY), (n, L, 1))
    transform[..., :3] = rng.normal(0, 0.002, (n, L, 3)) * (seed > 0)
    frame = np.zeros((n, L, 1))
    frame[:, ::3] = 2.5 * (seed > 0)   # (any non-zero value says odom_ideal)
    values = {"position": tips + np.array([0.02, -0.01, 0.0]) + rng.normal(0, 0.001, (n, L, 3)) * (seed > 0),
              "rotation": np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, L, 1)) if rotation is None else rotation, "transform": transform,
              "swing_clearance": np.full((n, L, 1), 0.02), "frame_is_odom_ideal": frame,
              "defined": np.ones((n, L, 1)) if defined is None else np.asarray(defined, dtype=np.float64).reshape(n, L, 1)}
    for name in fields:
        block = np.full((n, legs, values[name].shape[2]), SENTINEL)
        block[:, :L] = values[name]
        rows[:, cols[name]] = block.reshape(n, -1)
    return rows


def device_tensor(rows, dtype, wide):
    """(the tensor that owns the memory, the (n, F) view set_footholds gets): dense, or columns [5, 5 + F) of a wider tensor full of SENTINEL"""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    n, width = rows.shape
    big = torch.full((n, width + (16 if wide else 0)), SENTINEL, dtype=tdt, device="cuda")
    view = big[:, 5:5 + width] if wide else big
    view.copy_(torch.from_numpy(rows).to(tdt))
    torch.cuda.synchronize()   # the engines run on streams of their own: the tensor is complete before a call
    return big, view


def device_counter():
    import torch
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return c


def host_rows(values, fields, legs, L):
    """The definition's rows: ((n, L) ExternalTarget records, the (n, L) `defined` column) from float64 values (n, >= F)."""
    cols, _ = foothold_columns(fields, legs)
    n = len(values)
    get = lambda name: values[:, cols[name]].reshape(n, legs, -1)[:, :L]
    r = np.zeros((n, L), dtype=ET)
    if "position" in cols:
        r["pose"][..., :3] = get("position")
    if "rotation" in cols:
        r["pose"][..., 3:] = get("rotation")
    r["transform"] = get("transform") if "transform" in cols else np.array(IDENTITY)
    if "swing_clearance" in cols:
        r["swing_clearance"] = get("swing_clearance")[..., 0]
    if "frame_is_odom_ideal" in cols:
        r["frame_is_odom_ideal"] = get("frame_is_odom_ideal")[..., 0] != 0
    d = get("defined")[..., 0] if "defined" in cols else np.ones((n, L))
    r["defined"] = d > 0
    return r, d


def host_calls(eng, values, fields, legs, which=TARGET, mode="request"):
    """The host calls on the twin: one call for every leg when no leg is skipped, else one call per leg that is not.  Returns the dropped rows."""
    lib, n, L = eng.L, eng.n, eng.legs
    r, d = host_rows(values, fields, legs, L)
    total, one = 0, C.c_int64(0)
    todo = [(0, n, -1, r)] if (d >= 0).all() else [(i, 1, l, r[i, l:l + 1]) for i in range(n) for l in range(L) if d[i, l] >= 0]
    for first, count, leg, part in todo:
        part = np.ascontiguousarray(part)
        if mode == "request":
            assert lib.shc_engine_set_external_target(eng.h, which, first, count, leg, part.ctypes.data_as(C.c_void_p), C.byref(one)) == SHC_OK
            total += one.value
        else:
            tr = np.ascontiguousarray(part["transform"])
            assert lib.shc_engine_set_external_transform(eng.h, which, first, count, leg, tr.ctypes.data_as(C.c_void_p)) == SHC_OK
    return total


def records(eng, which):
    """(n, L) ExternalTarget records as the host getter returns them"""
    return np.frombuffer(bytes(memoryview(eng.get_external_target(which)).cast("B")), dtype=ET).reshape(eng.n, eng.legs)


def joint_bits(eng):
    q, qd = eng.joints()
    return q.tobytes() + qd.tobytes()


def assert_twins(a, b, what, cycles=0):
    a.synchronize(), b.synchronize()
    assert state_bytes(a) == state_bytes(b), f"{what}: the state records differ"
    assert bytes(a.get_aux_state()) == bytes(b.get_aux_state()), f"{what}: the auxiliary blobs differ"
    for which in (TARGET, DEFAULT, PLANNER) if a.params.rough_terrain_mode else (TARGET, PLANNER):
        assert records(a, which).tobytes() == records(b, which).tobytes(), f"{what}: record {which} differs"
    for sentinel in SENTINEL_BYTES:
        assert sentinel not in state_bytes(a) and sentinel not in bytes(a.get_aux_state()), f"{what}: a surplus column reached the state"
    if cycles:
        a.step(cycles), b.step(cycles)
        assert joint_bits(a) == joint_bits(b), f"{what}: the joints differ {cycles} cycles later"
        assert_twins(a, b, f"{what}, {cycles} cycles later")


def both(a, b, rows, fields, legs, dtype, wide, what, which=TARGET, mode="request", cycles=0, host=False):
    """A takes the new call, B the host calls on tensor.double(); the counts of dropped rows are equal and are returned."""
    import torch
    big, view = device_tensor(rows, dtype, wide)
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)   # (a mask holds NaN: compare the bytes)
    before = big.clone()
    if host:
        ignored = a.set_footholds(view.cpu().numpy(), fields, which, mode, legs=legs)
    else:
        counter = device_counter()
        assert a.set_footholds(view, fields, which, mode, ignored=counter, legs=legs) is None
        a.synchronize()
        ignored = int(counter.item())
    want = host_calls(b, view.double().cpu().numpy(), fields, legs, which, mode)
    assert ignored == want, f"{what}: {ignored} rows counted as dropped, the host calls dropped {want}"
    assert_twins(a, b, what, cycles)
    assert torch.equal(bits(big), bits(before)), f"{what}: the tensor was written"
    return ignored


def defined_count(eng, which):
    return int(records(eng, which)["defined"].sum())


# ------------------------------------------------------------------------------------------------------------ 1. the base scenario
def test_base_scenario_target_default_planner_target():
    """37 hexapods in rough terrain mode (10 robots per wavefront: three full robot groups and one of 7), robots 0 .. 4 STOPPED.  The figures are
    the CPU oracle's for this scenario."""
    (a, b, c), tips = walking(rough(default_hexapod_params("tripod")), 37, 8, count=3)
    try:
        rows = requests(tips, ALL, 6)
        assert rows.shape == (37, 102)
        assert both(a, b, rows, ALL, 6, "float64", False, "TARGET") == 0
        assert defined_count(a, TARGET) == 192 and defined_count(a, PLANNER) == 30 and defined_count(a, DEFAULT) == 0
        assert not records(a, TARGET)["defined"][:5].any() and records(a, PLANNER)["defined"][:5].all()
        a.step(40), b.step(40), c.step(40)
        assert joint_bits(a) == joint_bits(b)
        assert_twins(a, b, "TARGET, 40 cycles later")
        assert defined_count(a, TARGET) == 96, "96 of the 192 targets are consumed by the swings of 40 cycles"
        qa, qc = a.joints()[0], c.joints()[0]
        assert np.abs(qa - qc).max() > 1e-3, "the requests changed nothing: the comparisons above show nothing"
        assert both(a, b, requests(tips, ALL, 6, seed=1), ALL, 6, "float64", False, "DEFAULT", which=DEFAULT) == 30
        assert defined_count(a, DEFAULT) == 192
        assert both(a, b, requests(tips, ALL, 6, seed=2), ALL, 6, "float64", False, "PLANNER_TARGET", which=PLANNER, cycles=40) == 0
        assert defined_count(a, PLANNER) == 222
    finally:
        a.close(), b.close(), c.close()


@pytest.fixture(scope="module")
def hexapods():
    (a, b), tips = walking(rough(default_hexapod_params("tripod")), 37, 8)
    yield a, b, tips
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ 2. float32, a wider tensor, 8-leg rows
@pytest.mark.parametrize("which", [TARGET, DEFAULT, PLANNER])
def test_float32_columns_of_a_wider_tensor_with_surplus_legs(hexapods, which):
    a, b, tips = hexapods
    rows = requests(tips, ALL, 8, seed=3 + which)
    assert rows.shape[1] == 136 and (rows == SENTINEL).sum() == 37 * 2 * 17
    both(a, b, rows, ALL, 8, "float32", True, f"float32, record {which}", which=which, cycles=40 if which == PLANNER else 0)


# ------------------------------------------------------------------------------------------------------------ 3. defaults, the mask, another order
def mixed_mask(n, L, seed):
    rng = np.random.default_rng(seed)
    mask = rng.choice([1.0, 0.0, -1.0, np.nan, 3.5, -0.0], size=(n, L))
    mask[0, :min(L, 4)] = [1.0, 0.0, -1.0, np.nan][:L]
    return mask


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_position_alone_then_a_mask(hexapods, dtype):
    """A spec of the position alone: every other member takes the callback's value.  Then position + defined with a mask that mixes 1, 0, -1
    and NaN (and 3.5 and -0.0) per leg: 0 withdraws, negative and NaN leave alone."""
    a, b, tips = hexapods
    for which in (TARGET, DEFAULT, PLANNER):
        both(a, b, requests(tips, ("position",), 6, seed=10 + which), ("position",), 6, dtype, False, f"position alone, record {which}", which=which)
        rec = records(a, which)[5:]
        assert rec["defined"].all() and (rec["transform"] == np.array(IDENTITY)).all() and not rec["pose"][..., 3:].any() and not rec["swing_clearance"].any()
        mask = mixed_mask(37, 6, 20 + which)
        fields = ("position", "defined")
        before = records(a, which)
        both(a, b, requests(tips, fields, 6, seed=30 + which, defined=mask), fields, 6, dtype, True, f"mask, record {which}", which=which)
        after = records(a, which)
        alone = ~(mask >= 0)
        assert alone.sum() > 20 and after[alone].tobytes() == before[alone].tobytes(), "a leg to leave alone changed"
        withdrawn = (mask == 0)[5:]
        assert withdrawn.sum() > 20 and not after[5:][withdrawn]["defined"].any(), "a withdrawn request is still defined"
        assert (after[5:][withdrawn]["pose"] == before[5:][withdrawn]["pose"]).all(), "a withdrawn request lost the rest of its record"
    assert_twins(a, b, "after the masks", cycles=40)


def test_every_field_in_another_order_and_from_the_host(hexapods):
    a, b, tips = hexapods
    mask = mixed_mask(37, 6, 41)
    both(a, b, requests(tips, PERMUTED, 6, seed=42, defined=mask), PERMUTED, 6, "float32", True, "another order")
    both(a, b, requests(tips, PERMUTED, 7, seed=43, defined=mask), PERMUTED, 7, "float64", False, "another order, 7-leg rows", which=DEFAULT)
    # 8. the host form equals the device form (and so the host calls)
    for dtype in ("float32", "float64"):
        both(a, b, requests(tips, PERMUTED, 6, seed=44, defined=mixed_mask(37, 6, 45)), PERMUTED, 6, dtype, False, f"host rows {dtype}", host=True)
        both(a, b, requests(tips, ALL, 6, seed=46), ALL, 6, dtype, False, f"host rows {dtype}, DEFAULT", which=DEFAULT, host=True)
    strided = np.full((37, 120), SENTINEL)
    strided[:, :102] = requests(tips, ALL, 6, seed=47)
    assert a.set_footholds(strided[:, :102], ALL) == host_calls(b, strided, ALL, 6)      # a host view with a row stride
    assert_twins(a, b, "host rows", cycles=40)


# ------------------------------------------------------------------------------------------------------------ 4. the transform refresh
def unit_transforms(seed, n, L):
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, (n, L, 4))
    return np.concatenate([rng.normal(0, 0.3, (n, L, 3)), q / np.linalg.norm(q, axis=2, keepdims=True)], axis=2)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_refresh_transform(hexapods, dtype):
    a, b, tips = hexapods
    n, L = 37, 6
    for which in (TARGET, DEFAULT, PLANNER):
        some = (np.random.default_rng(50 + which).uniform(size=(n, L)) < 0.5).astype(np.float64)     # 1 requests, 0 withdraws
        both(a, b, requests(tips, ALL, 6, seed=51 + which, defined=some), ALL, 6, "float64", False, f"some defined, record {which}", which=which)
        live = records(a, which)["defined"] != 0
        assert 0 < live[5:].sum() < live[5:].size
        before = records(a, which)
        cols, width = foothold_columns(("transform",), 6)
        rows = unit_transforms(60 + which, n, L).reshape(n, -1)
        both(a, b, rows, ("transform",), 6, dtype, True, f"refresh, record {which}", which=which, mode="refresh_transform")
        after = records(a, which)
        assert (after["transform"][live] != before["transform"][live]).any(axis=1).all(), "a defined record kept its transform"
        assert after[~live].tobytes() == before[~live].tobytes(), "a record that is not defined took a transform"
        # with a `defined` column: the skip rule alone (0 does not withdraw here)
        fields = ("defined", "transform")
        cols, width = foothold_columns(fields, 8)
        rows = np.full((n, width), SENTINEL)
        mask = mixed_mask(n, L, 70 + which)
        rows[:, cols["defined"]] = np.concatenate([mask, np.full((n, 2), SENTINEL)], axis=1)
        rows[:, cols["transform"]] = np.concatenate([unit_transforms(71 + which, n, L), np.full((n, 2, 7), SENTINEL)], axis=1).reshape(n, -1)
        both(a, b, rows, fields, 8, dtype, False, f"masked refresh, record {which}", which=which, mode="refresh_transform")
        assert (records(a, which)["defined"] != 0).tobytes() == live.tobytes()
    assert_twins(a, b, "after the refreshes", cycles=40)


# ------------------------------------------------------------------------------------------------------------ 5. morphologies
MORPHS = {"8x5, two full groups + 1": (lambda: synthetic_octopod_params("ripple", 5, 8), 17),          # 8 robots per wavefront
          "5 legs, four idle lanes": (lambda: synthetic_octopod_params("ripple", 3, 5), 25),         # 12 per wavefront (5 x 3: the build's 5-leg morphology)
          "3 legs": (lambda: synthetic_octopod_params("wave", 3, 3), 22),                             # 21 per wavefront
          "mixed DOF": (lambda: synthetic_mixed_dof_params("ripple"), 11),
          "one hexapod": (lambda: default_hexapod_params("tripod"), 1)}


@pytest.mark.parametrize("case", list(MORPHS))
def test_morphologies(case):
    make, n = MORPHS[case]
    p = rough(make())
    stopped = 0 if n == 1 else 3
    (a, b), tips = walking(p, n, 12, stopped=stopped)
    try:
        L = p.leg_count
        rng = np.random.default_rng(80)
        q = rng.normal(0, 1, (n, L, 4))
        rotation = q / np.linalg.norm(q, axis=2, keepdims=True)                                       # (legs of > 3 joints steer towards it)
        assert both(a, b, requests(tips, ALL, L, seed=81, rotation=rotation), ALL, L, "float32", False, f"{case} TARGET") == 0
        assert defined_count(a, TARGET) == (n - stopped) * L and defined_count(a, PLANNER) == stopped * L
        assert both(a, b, requests(tips, ALL, 8, seed=82, rotation=rotation), ALL, 8, "float64", True, f"{case} DEFAULT", which=DEFAULT) == stopped * L
        both(a, b, requests(tips, PERMUTED, 8, seed=83, defined=mixed_mask(n, L, 84)), PERMUTED, 8, "float32", True, f"{case} mask", cycles=40)
        # read-back in the 8-leg geometry
        got = a.footholds(fields=PERMUTED, which=TARGET, pad=-3.0, legs=8)
        want, _ = host_rows(got, PERMUTED, 8, L)
        assert want.tobytes() == records(b, TARGET).tobytes()
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ 6. without rough terrain mode
def test_without_rough_terrain_mode():
    p = default_hexapod_params("tripod")
    assert not p.rough_terrain_mode
    (a, b), tips = walking(p, 37, 8)
    try:
        assert both(a, b, requests(tips, ALL, 6, seed=90), ALL, 6, "float32", False, "no rough terrain, TARGET") == 192   # no stepper reads them
        assert defined_count(a, TARGET) == 0 and defined_count(a, PLANNER) == 30                          # the STOPPED robots' rows went to the poser
        assert both(a, b, requests(tips, ALL, 6, seed=91), ALL, 6, "float64", False, "no rough terrain, PLANNER", which=PLANNER) == 0
        import torch
        big, view = device_tensor(requests(tips, ALL, 6, seed=92), "float32", False)
        before, aux = state_bytes(a), bytes(a.get_aux_state())
        host_view = view.cpu().numpy()
        for on_device, ptr in ((1, view.data_ptr()), (0, host_view.ctypes.data)):
            spec = foothold_spec(ALL, 6, "float32", DEFAULT)
            assert a.L.shc_engine_set_footholds(a.h, C.byref(spec), C.c_void_p(ptr), on_device, None) == SHC_ERR_UNSUPPORTED
            assert a.L.shc_engine_get_footholds(a.h, C.byref(spec), C.c_void_p(ptr), on_device) == SHC_ERR_UNSUPPORTED
        a.synchronize()
        assert state_bytes(a) == before and bytes(a.get_aux_state()) == aux
        assert_twins(a, b, "no rough terrain", cycles=40)
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ 7. read-back
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_read_back(hexapods, dtype):
    import torch
    a, b, tips = hexapods
    n, L = 37, 6
    both(a, b, requests(tips, ALL, 6, seed=100, defined=(np.arange(n * L).reshape(n, L) % 3 != 0)), ALL, 6, "float64", False, "before the read-back")
    both(a, b, requests(tips, ALL, 6, seed=101), ALL, 6, "float64", False, "before the read-back", which=DEFAULT)
    a.step(7), b.step(7)      # (some targets are consumed)
    before, aux = state_bytes(a), bytes(a.get_aux_state())
    tdt, ndt = (torch.float32, np.float32) if dtype == "float32" else (torch.float64, np.float64)
    for which in (TARGET, DEFAULT, PLANNER):
        rec = records(b, which)
        assert rec["defined"].any()
        for fields, legs in ((ALL, 6), (PERMUTED, 8), (("defined",), 6), (("transform", "swing_clearance"), 7)):
            cols, width = foothold_columns(fields, legs)
            big = torch.full((n, width + 16), SENTINEL, dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            assert a.footholds(big[:, 5:5 + width], fields, which, pad=-2.5, legs=legs) is None
            a.synchronize()
            got = big.cpu().numpy()
            assert (got[:, :5] == ndt(SENTINEL)).all() and (got[:, 5 + width:] == ndt(SENTINEL)).all(), "the sentinel around the columns is gone"
            got = got[:, 5:5 + width]
            want = {"position": rec["pose"][..., :3], "rotation": rec["pose"][..., 3:], "transform": rec["transform"],
                    "swing_clearance": rec["swing_clearance"][..., None], "frame_is_odom_ideal": rec["frame_is_odom_ideal"][..., None].astype(np.float64),
                    "defined": rec["defined"][..., None].astype(np.float64)}
            for name in fields:
                block = got[:, cols[name]].reshape(n, legs, -1)
                assert block[:, :L].tobytes() == want[name].astype(ndt).tobytes(), (which, name)
                assert (block[:, L:] == ndt(-2.5)).all(), "pad is missing in a surplus leg"
            host = a.footholds(fields=fields, which=which, pad=-2.5, dtype=dtype, legs=legs)          # the host form
            assert host.dtype == ndt and host.tobytes() == got.tobytes()
    a.synchronize()
    assert state_bytes(a) == before and bytes(a.get_aux_state()) == aux, "the read-back wrote into the engine"
    assert_twins(a, b, "after the read-back")


def test_round_trip(hexapods):
    """set -> get of a float64 tensor is bit-exact for the legs whose request was accepted."""
    import torch
    a, b, tips = hexapods
    rows = requests(tips, PERMUTED, 6, seed=110)
    cols, width = foothold_columns(PERMUTED, 6)
    rows[:, cols["frame_is_odom_ideal"]] = (rows[:, cols["frame_is_odom_ideal"]] != 0)   # (0 / 1 come back)
    assert both(a, b, rows, PERMUTED, 6, "float64", False, "round trip") == 0
    out = torch.zeros((37, width), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a.footholds(out, PERMUTED, TARGET)
    a.synchronize()
    got = out.cpu().numpy()
    assert got[5:].tobytes() == rows[5:].tobytes()
    assert got[:5].tobytes() != rows[:5].tobytes()       # (the rows of the STOPPED robots went to their posers)


# ------------------------------------------------------------------------------------------------------------ 9. the device count
def test_device_ignored_adds_up_and_may_be_null(hexapods):
    a, b, tips = hexapods
    _, view = device_tensor(requests(tips, ALL, 6, seed=120), "float32", False)
    counter = device_counter()
    a.set_footholds(view, ALL, DEFAULT, ignored=counter)
    a.set_footholds(view, ALL, DEFAULT, ignored=counter)
    a.set_footholds(view, ALL, TARGET, ignored=counter)
    a.set_footholds(view, ALL, DEFAULT)                    # NULL
    a.synchronize()
    assert int(counter.item()) == 60
    values = view.double().cpu().numpy()
    assert [host_calls(b, values, ALL, 6, w) for w in (DEFAULT, DEFAULT, TARGET, DEFAULT)] == [30, 30, 0, 30]
    assert_twins(a, b, "after the counted calls")
    spec = foothold_spec(ALL, 6, "float32", DEFAULT)
    host, host_view = C.c_int64(5), view.cpu().numpy()
    assert a.L.shc_engine_set_footholds(a.h, C.byref(spec), C.c_void_p(host_view.ctypes.data), 0, C.byref(host)) == SHC_OK
    assert host.value == 35, "the host word is added to"
    assert a.L.shc_engine_set_footholds(a.h, C.byref(spec), C.c_void_p(host_view.ctypes.data), 0, None) == SHC_OK
    for _ in range(2):
        host_calls(b, values, ALL, 6, DEFAULT)
    assert_twins(a, b, "after the host forms")


# ------------------------------------------------------------------------------------------------------------ 10. split steps
def test_between_split_steps():
    """40 970 hexapods = 4 097 wavefronts, the smallest batch whose steps run as two halves on two streams: the pass joins them, as the host
    call does."""
    need_gpu()
    p = rough(default_hexapod_params("tripod"))
    n = 40970
    t = generate_tables(p)
    a, b = BatchEngine(p, n, tables=t), BatchEngine(p, n, tables=t)
    try:
        rng = np.random.default_rng(13)
        lin, ang = rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.4, 0.4, n)
        lin[:5], ang[:5] = 0.0, 0.0
        tips = np.zeros((n, 6, 3))
        for e in (a, b):
            e.set_velocity(lin, ang)
            e.step(30)
            tips = e.leg_state()["walker_tip"].reshape(n, 6, 3)
        _, view = device_tensor(requests(tips, ALL, 6, seed=130), "float32", True)
        counter = device_counter()
        a.step(2)
        a.set_footholds(view, ALL, ignored=counter)
        a.step(2)
        b.step(2)
        want = host_calls(b, view.double().cpu().numpy(), ALL, 6)
        b.step(2)
        assert joint_bits(a) == joint_bits(b)
        assert state_bytes(a) == state_bytes(b)
        assert bytes(a.get_aux_state()) == bytes(b.get_aux_state())
        assert int(counter.item()) == want == 0
        assert defined_count(a, PLANNER) == 30
    finally:
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------ 11. refusals
def test_engine_refusals():
    import torch
    (eng,), tips = walking(default_hexapod_params("tripod"), 23, 17, count=1)
    lib, n = eng.L, eng.n
    fields = ("position", "defined")
    width = foothold_columns(fields, 6)[1]
    tens = torch.full((n, width + 4), 0.25, dtype=torch.float32, device="cuda")
    t64 = torch.full((n, width + 4), 0.25, dtype=torch.float64, device="cuda")
    counter = device_counter()
    before, aux_before = state_bytes(eng), bytes(eng.get_aux_state())
    good = lambda **kw: foothold_spec(fields, 6, "float32", **kw)

    def call(spec, p=None, h=None, ignored=None):
        return lib.shc_engine_set_footholds(eng.h if h is None else h, None if spec is None else C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p), 1,
                                            ignored)

    def get(spec, p=None):
        return lib.shc_engine_get_footholds(eng.h, None if spec is None else C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p), 1)
    cases = {}
    s = good()
    s.n_fields = 0
    cases["no field"] = s
    s = good()
    s.n_fields = 7
    cases["seven fields"] = s
    cases["an unknown field"] = foothold_spec((0, 6), 6)
    cases["a negative field"] = foothold_spec((0, -1), 6)
    cases["a repeated field"] = foothold_spec(("position", "defined", "position"), 6)
    s = good()
    s.dtype = 2
    cases["an unknown dtype"] = s
    cases["an unknown record"] = good(which=3)
    cases["an unknown mode"] = good(mode=2)
    s = good()
    s.reserved = 1
    cases["reserved != 0"] = s
    cases["legs below the engine's"] = foothold_spec(fields, 5)
    cases["legs above SHC_MAX_LEGS"] = foothold_spec(fields, 9)
    cases["a row stride below the width"] = good(row_stride=width - 1)
    for what, spec in cases.items():
        assert call(spec) == SHC_ERR_INVALID_ARG, what
        assert lib.shc_last_error(), what
        assert get(spec) == SHC_ERR_INVALID_ARG, what
    # what a mode asks of the fields (set only)
    assert call(foothold_spec(("rotation", "defined"), 6)) == SHC_ERR_INVALID_ARG                      # a request without the position
    assert call(foothold_spec(("defined",), 6, mode="refresh_transform")) == SHC_ERR_INVALID_ARG       # a refresh without the transform
    assert call(foothold_spec(("transform", "position"), 6, mode="refresh_transform")) == SHC_ERR_INVALID_ARG
    assert get(foothold_spec(("transform",), 6, mode="refresh_transform")) == SHC_ERR_INVALID_ARG      # mode is 0 for get
    assert lib.shc_engine_set_footholds(None, C.byref(good()), C.c_void_p(tens.data_ptr()), 1, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_get_footholds(None, C.byref(good()), C.c_void_p(tens.data_ptr()), 1) == SHC_ERR_INVALID_ARG
    assert call(None) == SHC_ERR_INVALID_ARG and get(None) == SHC_ERR_INVALID_ARG
    for on_device in (0, 1):
        assert lib.shc_engine_set_footholds(eng.h, C.byref(good()), None, on_device, None) == SHC_ERR_INVALID_ARG
        assert lib.shc_engine_get_footholds(eng.h, C.byref(good()), None, on_device) == SHC_ERR_INVALID_ARG
    assert call(good(), p=tens.data_ptr() + 2) == SHC_ERR_INVALID_ARG and get(good(), p=tens.data_ptr() + 2) == SHC_ERR_INVALID_ARG   # not aligned to a float
    s64 = foothold_spec(fields, 6, "float64")
    assert lib.shc_engine_set_footholds(eng.h, C.byref(s64), C.c_void_p(t64.data_ptr() + 4), 1, None) == SHC_ERR_INVALID_ARG
    assert call(good(), ignored=C.c_void_p(counter.data_ptr() + 4)) == SHC_ERR_INVALID_ARG           # the count is not aligned
    # what the Python layer refuses itself
    with pytest.raises(ValueError):
        eng.set_footholds(tens[:-1], fields)                                                          # a row short
    with pytest.raises(ValueError):
        eng.set_footholds(tens[:, :width - 1], fields)                                                # a column short
    with pytest.raises(ValueError):
        eng.set_footholds(tens.to(torch.float16), fields)
    with pytest.raises(ValueError):
        eng.set_footholds(tens.T, fields)                                                             # the elements of a row are not contiguous
    with pytest.raises(ValueError):
        eng.set_footholds(tens, fields, ignored=np.zeros(1, dtype=np.int64))                          # a host count with device rows
    with pytest.raises(ValueError):
        eng.footholds(tens[:, :width - 1], fields)
    with pytest.raises(ShcError):
        eng.set_footholds(tens, ("position", "position"))
    eng.synchronize()
    assert state_bytes(eng) == before and bytes(eng.get_aux_state()) == aux_before, "a refused call changed the state"
    assert int(counter.item()) == 0
    eng.resident_begin(ring_depth=4, max_cycles=100)
    eng.resident_end()         # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
    before = state_bytes(eng)
    eng.resident_begin(ring_depth=4, max_cycles=100)
    try:
        assert call(good()) == SHC_ERR_BUSY and get(good()) == SHC_ERR_BUSY
        assert lib.shc_engine_set_footholds(eng.h, C.byref(good()), C.c_void_p(tens.cpu().numpy().ctypes.data), 0, None) == SHC_ERR_BUSY
    finally:
        eng.resident_end()
    eng.synchronize()
    assert state_bytes(eng) == before, "a call refused in resident mode changed the state"
    assert call(good(row_stride=width + 4), ignored=C.c_void_p(counter.data_ptr())) == SHC_OK        # ... and the handle still works
    eng.synchronize()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 12. fleet
def fleet_tips(fleet):
    tips = np.zeros((N, ML, 3))
    for view, ids in views(fleet):
        tips[ids, :view.legs] = view.leg_state()["walker_tip"].reshape(len(ids), view.legs, 3)
    return tips


def fleet_requests(tips, fields, seed, defined=None):
    """requests() in the fleet's 8-leg geometry: SENTINEL in the legs a hexapod lacks"""
    rows = requests(tips, fields, ML, seed=seed, defined=defined)
    cols, _ = foothold_columns(fields, ML)
    for name in fields:
        block = rows[:, cols[name]].reshape(N, ML, -1)
        for i in range(N):
            block[i, LEGS[int(MORPH[i])]:] = SENTINEL
        rows[:, cols[name]] = block.reshape(N, -1)
    return rows


def assert_fleets(a, b, what):
    a.synchronize(), b.synchronize()
    ra, rb = robot_records(a), robot_records(b)
    for i in range(N):
        assert ra[i] == rb[i], f"{what}: robot {i} (bin {MORPH[i]}) holds other records than its twin"
    assert not any(sentinel in part for rec in ra for part in rec for sentinel in SENTINEL_BYTES), f"{what}: a padded column reached the state"


def fleet_host_calls(fleet, values, fields, which=TARGET, mode="request"):
    """The definition: the host calls per part on rows[ids]"""
    return sum(host_calls(view, values[ids], fields, ML, which, mode) for view, ids in views(fleet))


def test_fleet():
    need_gpu()
    import torch
    a, b = (MixedFleet(morphologies(rough=True), MORPH, (0,)) for _ in range(2))
    try:
        rng = np.random.default_rng(14)
        lin, ang = rng.uniform(-0.4, 0.4, (N, 2)), rng.uniform(-0.4, 0.4, N)
        lin[:6], ang[:6] = 0.0, 0.0               # the first six robots are STOPPED
        for f in (a, b):
            f.set_velocity(lin, ang)
            f.step(40)
            f.synchronize()
        tips = fleet_tips(a)
        fleet_tips(b)
        assert_fleets(a, b, "before the requests")
        stopped_legs = int(sum(LEGS[int(m)] for m in MORPH[:6]))
        held = None
        for round_, (fields, which, dtype, want) in enumerate(((ALL, TARGET, "float32", 0), (ALL, DEFAULT, "float64", stopped_legs),
                                                              (PERMUTED, TARGET, "float32", None), (ALL, PLANNER, "float32", 0))):
            mask = None if want is not None else np.random.default_rng(15).choice([1.0, 0.0, -1.0, np.nan], size=(N, ML))
            rows = fleet_requests(tips, fields, 140 + round_, defined=mask)
            big, view = device_tensor(rows, dtype, True)
            before = big.cpu().numpy().tobytes()
            counter = device_counter()
            assert a.set_footholds(view, fields, which, ignored=counter) is None
            if held is None:
                held = a.io_nbytes      # (the fleet's first device I/O call: ids and staging are in place from here on)
                assert held > 0
            a.synchronize()
            ignored = fleet_host_calls(b, view.double().cpu().numpy(), fields, which)
            assert int(counter.item()) == ignored, "all parts add to the same word"
            assert want is None or ignored == want
            assert_fleets(a, b, f"fleet, round {round_}")
            assert big.cpu().numpy().tobytes() == before, "the tensor was written"
        # the refresh
        cols, width = foothold_columns(("transform",), ML)
        rows = np.full((N, ML, 7), SENTINEL)
        for i in range(N):
            rows[i, :LEGS[int(MORPH[i])]] = unit_transforms(150 + i, 1, LEGS[int(MORPH[i])])[0]
        _, view = device_tensor(rows.reshape(N, -1), "float64", False)
        a.set_footholds(view, ("transform",), TARGET, mode="refresh_transform")
        fleet_host_calls(b, view.cpu().numpy(), ("transform",), TARGET, "refresh_transform")
        assert_fleets(a, b, "fleet, refresh")
        # the read-back: pad in the legs a hexapod lacks
        for which in (TARGET, DEFAULT, PLANNER):
            for dtype, tdt in (("float32", torch.float32), ("float64", torch.float64)):
                cols, width = foothold_columns(PERMUTED, ML)
                big = torch.full((N, width + 7), SENTINEL, dtype=tdt, device="cuda")
                torch.cuda.synchronize()
                a.footholds(big[:, 3:3 + width], PERMUTED, which, pad=-2.5)
                a.synchronize()
                got = big.cpu().numpy()
                assert (got[:, :3] == np.dtype(dtype).type(SENTINEL)).all() and (got[:, 3 + width:] == np.dtype(dtype).type(SENTINEL)).all()
                got = got[:, 3:3 + width]
                for view_, ids in views(b):
                    rec = records(view_, which)
                    want_rows, _ = host_rows(got[ids].astype(np.float64), PERMUTED, ML, view_.legs)
                    if dtype == "float64":
                        assert want_rows.tobytes() == rec.tobytes()
                    else:
                        assert want_rows["pose"].tobytes() == rec["pose"].astype(np.float32).astype(np.float64).tobytes()
                        assert want_rows["defined"].tobytes() == rec["defined"].tobytes()
                    for name in PERMUTED:
                        assert (got[ids][:, cols[name]].reshape(len(ids), ML, -1)[:, view_.legs:] == -2.5).all(), "pad is missing"
                host = np.full((N, width), SENTINEL, dtype=dtype)
                a.footholds(host, PERMUTED, which, pad=-2.5)                                           # host arrays go part by part
                assert host.tobytes() == got.tobytes()
        assert a.io_nbytes == held, "the foothold pass allocated staging"
        assert_fleets(a, b, "after the read-back")
        # host rows: every part through its engine's host form
        rows = fleet_requests(tips, ALL, 160)
        assert a.set_footholds(rows, ALL, DEFAULT) == fleet_host_calls(b, rows, ALL, DEFAULT) == stopped_legs
        assert_fleets(a, b, "fleet, host rows")
        for _ in range(4):
            a.step(10), b.step(10)
            qa, qb = a.joints(), b.joints()
            assert qa[0].tobytes() == qb[0].tobytes() and qa[1].tobytes() == qb[1].tobytes()
        assert_fleets(a, b, "fleet, 40 cycles later")
    finally:
        a.close(), b.close()


def test_fleet_refusals():
    need_gpu()
    import torch
    a = MixedFleet(morphologies(), MORPH, (0,))      # (no rough terrain mode)
    try:
        lib = a.L
        fields = ("position", "defined")
        width = foothold_columns(fields, ML)[1]
        tens = torch.full((N, width), 0.25, dtype=torch.float32, device="cuda")
        counter = device_counter()
        before = robot_records(a)
        good = foothold_spec(fields, ML, "float32")

        def call(spec, p=None, ignored=None):
            return lib.shc_fleet_set_footholds_device(a.h, None if spec is None else C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p), ignored)

        def get(spec, p=None):
            return lib.shc_fleet_get_footholds_device(a.h, None if spec is None else C.byref(spec), C.c_void_p(tens.data_ptr() if p is None else p))
        assert lib.shc_fleet_set_footholds_device(None, C.byref(good), C.c_void_p(tens.data_ptr()), None) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_get_footholds_device(None, C.byref(good), C.c_void_p(tens.data_ptr())) == SHC_ERR_INVALID_ARG
        assert call(None) == SHC_ERR_INVALID_ARG and get(None) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_set_footholds_device(a.h, C.byref(good), None, None) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_get_footholds_device(a.h, C.byref(good), None) == SHC_ERR_INVALID_ARG
        for spec in (foothold_spec(fields, ML - 1, "float32"), foothold_spec(fields, ML + 1, "float32"), foothold_spec(fields, ML, 2),
                     foothold_spec(fields, ML, "float32", row_stride=width - 1), foothold_spec(("defined", "defined"), ML), foothold_spec((6,), ML),
                     foothold_spec(fields, ML, which=3), foothold_spec(fields, ML, mode=2)):
            assert call(spec) == SHC_ERR_INVALID_ARG and get(spec) == SHC_ERR_INVALID_ARG
        s = foothold_spec(fields, ML, "float32")
        s.reserved = 1
        assert call(s) == SHC_ERR_INVALID_ARG
        assert call(foothold_spec(("defined",), ML)) == SHC_ERR_INVALID_ARG                          # a request without the position
        assert call(good, p=tens.data_ptr() + 2) == SHC_ERR_INVALID_ARG
        assert call(good, ignored=C.c_void_p(counter.data_ptr() + 4)) == SHC_ERR_INVALID_ARG
        assert call(foothold_spec(fields, ML, "float32", DEFAULT)) == SHC_ERR_UNSUPPORTED             # no part reads defaults
        assert get(foothold_spec(fields, ML, "float32", DEFAULT)) == SHC_ERR_UNSUPPORTED
        assert a.io_nbytes == 0                                                                      # nobody got as far as preparing device I/O
        with pytest.raises(ValueError):
            a.set_footholds(tens[:-1], fields)
        with pytest.raises(ValueError):
            a.set_footholds(tens[:, :width - 1], fields)
        assert robot_records(a) == before
        hexapods = views(a)[0][0]
        hexapods.resident_begin(ring_depth=4, max_cycles=100)
        hexapods.resident_end()    # (whatever entering and leaving resident mode itself leaves in the records is in `before`)
        before = robot_records(a)
        hexapods.resident_begin(ring_depth=4, max_cycles=100)
        try:
            assert call(good) == SHC_ERR_BUSY and get(good) == SHC_ERR_BUSY
        finally:
            hexapods.resident_end()
        assert robot_records(a) == before, "a call refused for one part changed another"
        assert call(good, ignored=C.c_void_p(counter.data_ptr())) == SHC_OK
        a.synchronize()
        assert a.io_nbytes > 0
    finally:
        a.close()


def test_a_fleet_on_two_devices_is_refused():
    need_gpu()
    if device_count() < 2:
        pytest.skip("one device")
    import torch
    a = MixedFleet(morphologies(rough=True), MORPH, (0, 1))
    try:
        width = foothold_columns(ALL, ML)[1]
        tens = torch.zeros((N, width), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        spec = foothold_spec(ALL, ML, "float32")
        assert a.L.shc_fleet_set_footholds_device(a.h, C.byref(spec), C.c_void_p(tens.data_ptr()), None) == SHC_ERR_UNSUPPORTED
        assert a.L.shc_fleet_get_footholds_device(a.h, C.byref(spec), C.c_void_p(tens.data_ptr())) == SHC_ERR_UNSUPPORTED
    finally:
        a.close()
