"""GPU (-m gpu): shc_engine_scan_health - every robot's IK warnings (the reference's "IK Clamping Event/s" and "Inverse kinematics deviation!"
lines, model.cpp:811-853, :914-929) as one record per robot, the restore map and the ascending list of the robots that meet a caller's criteria.

The records are held to the numpy restatement of the reference lines (tests/health_numpy.py) fed from the engine's own getters - flags, masks,
list and count equal; the two ratios within 2 ulp and the tip deviation within 1e-15 m (the bars of health_numpy.assert_records_match) - and the
IK bit to the oracle's, teacher-forced."""
import ctypes as C

import numpy as np
import pytest

import health_numpy as hn
from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import (HEALTH_IK_DEVIATION, HEALTH_POSITION_LIMIT, HEALTH_SPEED_LIMIT, ROBOT_HEALTH_DTYPE, SHC_ERR_BUSY,
                                                     SHC_ERR_INVALID_ARG, SHC_OK, BatchEngine, HealthCriteria)
from syropod_highlevel_controller_amd.fleet import MixedFleet
from test_gpu_parity import apply, make_inputs
from test_gpu_resident import state_bytes
from test_gpu_teacher_forced import as_np, config3_params

pytestmark = pytest.mark.gpu
SENTINEL = -7


def numpy_health(eng, first=0, count=None, **kw):
    """The restatement on the engine's own getters: (records, selection mask) of instances [first, first + count)."""
    count = eng.n - first if count is None else count
    q, qd = eng.joints()
    ls = eng.leg_state()
    pose, _, _ = eng.body_state()
    s = slice(first, first + count)
    return hn.robot_health(eng.params, q[s], qd[s], ls["poser_tip"][s], ls["model_tip"][s], ls["admittance"][s], ls["leg_status"][s], pose[s],
                           walker_tip=ls["walker_tip"][s], **kw)


def scan_host(eng, first, count, select=0, near_limit_proximity=None, tip_deviation=None, expect=SHC_OK):
    """The host form with all four outputs: (records, restore_map, selected (sentinel-filled), n_selected)."""
    crit = HealthCriteria(select, 0, -np.inf if near_limit_proximity is None else near_limit_proximity, np.inf if tip_deviation is None else tip_deviation)
    health = np.zeros(count, dtype=ROBOT_HEALTH_DTYPE)
    rmap, sel, nsel = np.full(eng.n, SENTINEL, dtype=np.int64), np.full(count, SENTINEL, dtype=np.int64), np.full(1, SENTINEL, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = eng.L.shc_engine_scan_health(eng.h, first, count, C.byref(crit), ptr(health), ptr(rmap), ptr(sel), ptr(nsel), 0)
    assert rc == expect, eng.L.shc_last_error()
    return health, rmap, sel, int(nsel[0])


def scan_device(eng, first, count, select=0, near_limit_proximity=None, tip_deviation=None):
    """The device form into torch tensors on the engine's (the default) stream: the same four outputs, copied back."""
    import torch
    health = torch.zeros(count * 4, dtype=torch.float64, device="cuda")
    rmap, sel = (torch.full((k,), SENTINEL, dtype=torch.int64, device="cuda") for k in (eng.n, count))
    nsel = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    assert eng.scan_health(select, -np.inf if near_limit_proximity is None else near_limit_proximity, np.inf if tip_deviation is None else tip_deviation, first, count,
                           out_health=health, out_restore_map=rmap, out_selected=sel, out_n_selected=nsel) is None
    return health.cpu().numpy().view(ROBOT_HEALTH_DTYPE), rmap.cpu().numpy(), sel.cpu().numpy(), int(nsel.cpu()[0])


def check_scan(eng, first, count, what, **kw):
    """Host form == device form byte for byte; records, map, list and count against the numpy restatement."""
    h, rmap, sel, nsel = scan_host(eng, first, count, **kw)
    hd, rmapd, seld, nseld = scan_device(eng, first, count, **kw)
    assert h.tobytes() == hd.tobytes() and rmap.tobytes() == rmapd.tobytes() and sel.tobytes() == seld.tobytes() and nsel == nseld, f"{what}: host form != device form"
    want, chosen = numpy_health(eng, first, count, **kw)
    hn.assert_records_match(h, want, what)
    ids = first + np.flatnonzero(chosen)
    assert nsel == len(ids) and np.array_equal(sel[:nsel], ids), (what, nsel, sel.tolist(), ids.tolist())
    assert (sel[nsel:] == SENTINEL).all(), f"{what}: entries past the count were written"
    expect_map = np.full(eng.n, -1, dtype=np.int64)
    expect_map[ids] = ids
    assert np.array_equal(rmap, expect_map), (what, rmap.tolist())
    return h


MORPHS = {"6x3": (lambda: default_hexapod_params("tripod"), 23, [(0, 23), (3, 17)]),
          "8x5": (lambda: synthetic_octopod_params("ripple", 5, 8), 19, [(0, 19), (5, 9)]),
          "mixed DOF": (lambda: synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4)), 11, [(0, 11), (2, 8)])}


@pytest.mark.parametrize("morph", list(MORPHS))
def test_injected_states(morph):
    """The cases of tests/test_health_layout.py planted through set_state, one robot each, into a walking batch: 6x3 with n = 23 (ten robots per
    wavefront, a partial last group, and a range (3, 17) that cuts two groups), 8x5 with n = 19, the mixed-DOF robot with n = 11.  The zero-range
    joint is a joint of the engine's parameters locked at its default position (it belongs to every robot)."""
    make, n, ranges = MORPHS[morph]
    p = make()
    L = p.leg_count
    D = max(p.leg_dof[l] for l in range(L))
    lock_leg, lock_j = 2, p.leg_dof[2] - 1
    from syropod_highlevel_controller_amd.engine import generate_tables
    p.joint[lock_leg][lock_j].min = p.joint[lock_leg][lock_j].max = generate_tables(p).default_joint_position[lock_leg][lock_j]
    eng = BatchEngine(p, n)
    rng = np.random.default_rng(n)
    robots = {case: 1 + 2 * k if n >= 21 else 1 + k for k, case in enumerate(hn.CASES)}   # one robot per case, inside and outside the cut ranges
    lin, ang = rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-0.4, 0.4, n)
    for case, r in robots.items():   # the robots of the deviation cases stand (a walking 3-joint leg with a locked joint cannot track its tip: only the
        if case.startswith("deviation"):   # planted deviation is to decide their flag)
            lin[r], ang[r] = 0.0, 0.0
    eng.set_velocity(lin, ang)
    eng.step(45)
    eng.synchronize()
    ls = eng.leg_state()
    states = eng.get_state()
    s = as_np(states)
    where = {}
    for case, r in robots.items():
        leg = int(rng.integers(0, L))
        j = int(rng.integers(0, p.leg_dof[leg] - (1 if leg == lock_leg else 0)))
        where[case] = (r, leg, j)
        rec = s["leg"][r, leg]
        if case == "joint exactly on min":
            rec["joint_position"][j] = p.joint[leg][j].min
        elif case == "joint exactly on max":
            rec["joint_position"][j] = p.joint[leg][j].max
        elif case == "rate exactly at max_angular_speed":
            rec["joint_velocity"][j] = p.joint[leg][j].max_vel
        elif case.startswith("deviation"):   # model tip and poser tip are derived from the joints / walker tip: the admittance delta carries the offset
            target = {"deviation just below 5 mm": hn.IK_TOLERANCE - 1e-9, "deviation just above 5 mm": hn.IK_TOLERANCE + 1e-9,
                      "deviation above a caller threshold": 0.002}[case]
            s["leg"]["admittance_delta"][r, :L] = 0.0
            rec["admittance_delta"][j % 3] = ls["model_tip"][r, leg, j % 3] - ls["poser_tip"][r, leg, j % 3] - target
        elif case == "leg_status bit 2 on two legs":
            s["leg"]["ik_failed"][r, [1, L - 1]] = 1
        elif case == "one NaN angle":
            rec["joint_position"][j] = np.nan
        elif case == "one Inf pose component":
            s["current_pose"][r, j] = np.inf
    eng.set_state(states)
    for first, count in ranges:
        for kw in (dict(select=63, near_limit_proximity=0.05, tip_deviation=hn.IK_TOLERANCE), dict(select=hn.POSITION_LIMIT | hn.TIP_DEVIATION, tip_deviation=0.0015),
                   dict(select=0)):
            h = check_scan(eng, first, count, f"{morph} range ({first}, {count}) {kw}", **kw)
            for case, (r, leg, j) in where.items():
                if not first <= r < first + count:
                    continue
                flags, masks = int(h["flags"][r - first]), int(h["leg_masks"][r - first])
                must_set, _ = hn.CASES[case]
                if case.startswith("deviation"):
                    raised = (kw.get("tip_deviation") is not None) and {"deviation just below 5 mm": 0.005 - 1e-9, "deviation just above 5 mm": 0.005 + 1e-9,
                                                                        "deviation above a caller threshold": 0.002}[case] > kw["tip_deviation"]
                    if case != "deviation just below 5 mm" or kw.get("tip_deviation") == hn.IK_TOLERANCE:   # (the only deviation of that robot is the planted one: it
                        assert bool(flags & hn.TIP_DEVIATION) == raised, (case, kw, flags, h["max_tip_deviation"][r - first])   # stands, its other legs track within 1e-4 m)
                elif case != "zero-range joint":
                    assert flags & must_set == must_set, (case, flags)
                if case in ("joint exactly on min", "joint exactly on max"):
                    assert masks >> (8 + leg) & 1 and h["min_limit_proximity"][r - first] == 0.0
                if case == "rate exactly at max_angular_speed":
                    assert masks >> (16 + leg) & 1 and h["max_speed_ratio"][r - first] >= 1.0
                if case == "leg_status bit 2 on two legs":
                    assert masks >> 1 & 1 and masks >> (L - 1) & 1   # (the leg with the locked joint may carry the bit of its own accord)
                if case == "one NaN angle":
                    assert masks >> (24 + leg) & 1
    # the zero-range joint: locked on both of its limits at once, and on no limit for the scan (model.cpp:848) - a robot nothing was planted in
    h, _, _, _ = scan_host(eng, 0, n)
    q = eng.joints()[0].reshape(n, L, D)
    lo, hi, _, own = hn.joint_limits(p)
    free = own.copy()
    free[lock_leg, lock_j] = False
    r = 0
    assert q[r, lock_leg, lock_j] == lo[lock_leg, lock_j] == hi[lock_leg, lock_j]
    on_other = ((q[r] <= lo) | (q[r] >= hi))[lock_leg][free[lock_leg]].any()
    assert bool(h["leg_masks"][r] >> (8 + lock_leg) & 1) == bool(on_other)
    eng.close()


def test_against_the_oracle_teacher_forced():
    """64 hexapods with config 3's feature set under tip forces U(0, 20) N - the inputs under which the teacher-forced config 3 test saturates the
    clamps: at five points of a 120-cycle oracle run the oracle's records are injected and scanned.  The IK byte of leg_masks is the oracle's
    ik_failed bit for bit; proximity and speed ratio are the restatement on the oracle's q / qd; the run raises POSITION_LIMIT and SPEED_LIMIT
    (checked on the oracle alone first: these inputs raise both at every one of the five points, no larger force range was needed)."""
    p = config3_params()
    n, L = 64, 6
    inp = make_inputs(p, n, 5, imu=True, force=20.0)
    rng = np.random.default_rng(0xADD1)
    eng, ob = BatchEngine(p, n), OracleBatch(p, n)
    apply(eng, inp)
    apply(ob, inp)
    raised_oracle = raised = 0
    for c in range(120):
        if c and c % 10 == 0:
            f = np.stack([rng.normal(0, 1, (n, 6)), rng.normal(0, 1, (n, 6)), rng.uniform(0, 20, (n, 6))], axis=2)
            ob.set_tip_force(f)
        ob.step(1, 8)
        if c + 1 not in (24, 48, 72, 96, 120):
            continue
        q, qd = ob.joints()
        lo = ob.leg_state()
        want, _ = hn.robot_health(p, q, qd, lo["poser_tip"], lo["model_tip"], lo["admittance"], lo["leg_status"], ob.body_state()[0])
        raised_oracle |= int(np.bitwise_or.reduce(want["flags"]))
        eng.set_state(ob.get_state())
        h, _ = eng.scan_health()
        ik = (((lo["leg_status"] & 4) != 0) * (1 << np.arange(L))).sum(axis=1)
        assert np.array_equal(h["leg_masks"] & 0xff, ik), f"cycle {c + 1}: IK byte != the oracle's ik_failed"
        assert np.array_equal(h["leg_masks"] >> 8 & 0xffff, want["leg_masks"] >> 8 & 0xffff), f"cycle {c + 1}: limit bytes"
        for k in ("min_limit_proximity", "max_speed_ratio"):
            d = np.abs(h[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
            print(f"cycle {c + 1}: {k} max difference {d.max():.3e}")
            assert d.max() <= 2.3e-16, (c + 1, k, float(d.max()))
        raised |= int(np.bitwise_or.reduce(h["flags"]))
    assert raised_oracle & (hn.POSITION_LIMIT | hn.SPEED_LIMIT), "the oracle alone must raise a limit flag under these inputs"
    assert raised & (hn.POSITION_LIMIT | hn.SPEED_LIMIT)
    eng.close()


def test_ik_bit_against_the_deviation():
    """Position-only IK (3-joint legs, no tip rotation): after a cycle, a leg carries the IK deviation bit exactly when its deviation - the
    getters' model tip against poser tip + admittance delta - exceeds 5 mm.  The getters re-derive the two tips (a rounding away from what the
    cycle compared), so legs within 1e-9 m of the threshold are left out; they are fewer than 1 % of the legs compared."""
    p = default_hexapod_params("tripod")
    p.admittance_control = 1
    n, L = 256, 6
    rng = np.random.default_rng(11)
    eng = BatchEngine(p, n)
    eng.set_velocity(rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(-0.8, 0.8, n))
    seen_set = seen_clear = excluded = compared = 0
    for burst in range(4):
        eng.set_tip_force(np.stack([rng.normal(0, 1, (n, L)), rng.normal(0, 1, (n, L)), rng.uniform(0, 20, (n, L))], axis=2))
        eng.step(12)
        h, _ = eng.scan_health()
        ls = eng.leg_state()
        dev = np.abs(ls["model_tip"] - (ls["poser_tip"] + ls["admittance"])).max(axis=2)
        bit = (h["leg_masks"][:, None] >> np.arange(L) & 1).astype(bool)
        assert np.array_equal(bit, (ls["leg_status"] & 4) != 0)
        clear = np.abs(dev - hn.IK_TOLERANCE) > 1e-9
        assert np.array_equal(bit[clear], (dev > hn.IK_TOLERANCE)[clear]), f"burst {burst}"
        excluded, compared = excluded + int((~clear).sum()), compared + clear.size
        seen_set, seen_clear = seen_set + int(bit.sum()), seen_clear + int((~bit).sum())
    assert excluded < 0.01 * compared, (excluded, compared)
    assert seen_set > 0 and seen_clear > 0, "both sides of the threshold are visited"
    eng.close()


def test_compaction_across_passes():
    """n = 5 003 hexapods are 501 wavefronts of ten: the count scan works on tiles of 256 wavefronts (kHealthTile, csrc/shc_health.hpp), so the
    counts fill two tiles (the second partly) and a second level adds the tiles' totals - a robot's place in the list is the sum of two levels'
    prefixes.  A pseudo-random third of the robots is selected through an injected IK flag."""
    p = default_hexapod_params("tripod")
    n = 5003
    eng = BatchEngine(p, n)
    rng = np.random.default_rng(5003)
    pick = rng.random(n) < 1.0 / 3.0
    states = eng.get_state()
    s = as_np(states)
    s["leg"]["ik_failed"][pick, 3] = 1
    eng.set_state(states)
    for first, count in ((0, n), (2557, 2446)):   # ... and a range that starts inside the second tile's first wavefronts
        h, rmap, sel, nsel = scan_device(eng, first, count, select=HEALTH_IK_DEVIATION)
        ids = first + np.flatnonzero(pick[first:first + count])
        assert nsel == len(ids)
        assert (np.diff(sel[:nsel]) > 0).all() and np.array_equal(sel[:nsel], ids)
        assert (sel[nsel:] == SENTINEL).all()
        assert np.array_equal(np.flatnonzero(rmap >= 0), ids) and np.array_equal(rmap[ids], ids) and (rmap[rmap < 0] == -1).all()
        assert np.array_equal(h["flags"] != 0, pick[first:first + count])
    eng.close()


def test_closed_loop_on_the_device():
    """step -> scan -> restore without a host round trip: 40 hexapods with admittance control, the odd ones under 20 N on every tip.  After 60
    cycles the scan selects the robots that show an IK deviation or stand on a position / speed limit into a device map, and restore(ck, map)
    resets exactly those to the checkpoint.  (The oracle on the CPU gives flags 7 for every odd robot and 0 for every even one under these inputs.)"""
    import torch
    p = default_hexapod_params("tripod")
    p.admittance_control = 1
    n = 40
    eng = BatchEngine(p, n)
    rng = np.random.default_rng(40)
    eng.set_velocity(rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(-0.5, 0.5, n))
    f = np.zeros((n, 6, 3))
    eng.set_tip_force(f)   # the first tip-force message switches touchdown detection on for the engine (a fact get_state reports per robot): before the capture
    ck = eng.checkpoint()
    at_checkpoint = state_bytes(eng)
    f[1::2, :, 2] = 20.0
    eng.set_tip_force(f)
    eng.step(60)
    before = state_bytes(eng)
    rmap = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    nsel = torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.scan_health(HEALTH_IK_DEVIATION | HEALTH_POSITION_LIMIT | HEALTH_SPEED_LIMIT, out_restore_map=rmap, out_n_selected=nsel)
    eng.restore(ck, rmap)
    after = state_bytes(eng)
    m, k = rmap.cpu().numpy(), int(nsel.cpu()[0])
    assert 0 < k < n and k == int((m >= 0).sum())
    per = len(after) // n
    for i in range(n):
        assert after[i * per:(i + 1) * per] == (at_checkpoint if m[i] >= 0 else before)[i * per:(i + 1) * per], (i, int(m[i]))
    assert np.array_equal(np.flatnonzero(m >= 0), np.arange(1, n, 2)), m.tolist()
    ck.close()
    eng.close()


def test_refusals():
    import torch
    p = default_hexapod_params("tripod")
    n = 12
    eng = BatchEngine(p, n)
    fn = eng.L.shc_engine_scan_health
    health = np.zeros(n, dtype=ROBOT_HEALTH_DTYPE)
    hp = health.ctypes.data_as(C.c_void_p)
    for first, count in ((-1, 2), (0, n + 1), (n + 1, 0), (5, n - 4), (3, -1)):
        assert fn(eng.h, first, count, None, hp, None, None, None, 0) == SHC_ERR_INVALID_ARG, (first, count)
    assert fn(eng.h, 0, n, None, None, None, None, None, 0) == SHC_ERR_INVALID_ARG
    assert fn(eng.h, 0, n, C.byref(HealthCriteria(64, 0, 0.0, 0.0)), hp, None, None, None, 0) == SHC_ERR_INVALID_ARG
    assert fn(eng.h, 0, n, C.byref(HealthCriteria(1, 1, 0.0, 0.0)), hp, None, None, None, 0) == SHC_ERR_INVALID_ARG
    dev = torch.zeros(4 * n + 2, dtype=torch.float64, device="cuda")
    assert dev.data_ptr() % 16 == 0
    assert fn(eng.h, 0, n, None, C.c_void_p(dev.data_ptr() + 8), None, None, None, 1) == SHC_ERR_INVALID_ARG
    assert fn(eng.h, 0, n, None, None, C.c_void_p(dev.data_ptr() + 4), None, None, 1) == SHC_ERR_INVALID_ARG
    assert fn(eng.h, 0, n, None, C.c_void_p(dev.data_ptr()), None, None, None, 1) == SHC_OK
    # count = 0 writes a zero count and a map of -1, in both forms
    _, rmap, sel, nsel = scan_host(eng, 4, 0, select=63)
    assert nsel == 0 and (rmap == -1).all()
    _, rmap, sel, nsel = scan_device(eng, n, 0, select=63)
    assert nsel == 0 and (rmap == -1).all()
    with pytest.raises(ValueError):
        eng.scan_health(out_restore_map=torch.zeros(n - 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.scan_health(out_selected=torch.zeros(n, dtype=torch.int32, device="cuda"))
    eng.resident_begin(ring_depth=4, max_cycles=50)
    assert fn(eng.h, 0, n, None, hp, None, None, None, 0) == SHC_ERR_BUSY
    eng.resident_end()
    assert fn(eng.h, 0, n, None, hp, None, None, None, 0) == SHC_OK
    eng.close()


def test_a_scan_changes_no_state():
    p = config3_params()
    n = 33
    inp = make_inputs(p, n, 9, imu=True, force=12.0)
    a, b = BatchEngine(p, n), BatchEngine(p, n)
    for e in (a, b):
        apply(e, inp)
        e.step(30)
    before = state_bytes(a)
    check_scan(a, 0, n, "config 3", select=63, near_limit_proximity=0.1, tip_deviation=0.001)
    check_scan(a, 7, 19, "config 3 range", select=7)
    assert state_bytes(a) == before
    for e in (a, b):
        e.step(20)
    assert state_bytes(a) == state_bytes(b), "twenty further cycles differ from the twin that never scanned"
    a.close()
    b.close()


def test_fleet_records_in_the_callers_order():
    pa, pb = default_hexapod_params("tripod"), synthetic_octopod_params("ripple", 5, 8)
    pa.admittance_control = 1
    morph = np.array([0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1], dtype=np.int32)
    n = len(morph)
    fleet = MixedFleet([pa, pb], morph)
    rng = np.random.default_rng(13)
    fleet.set_velocity(rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.6, 0.6, n))
    f = np.zeros((n, fleet.max_legs, 3))
    f[::3, :, 2] = 20.0
    a = np.ascontiguousarray(f)
    from syropod_highlevel_controller_amd import engine as _e
    _e._check(fleet.L.shc_fleet_set_tip_force(fleet.h, a.ctypes.data_as(C.c_void_p)), "shc_fleet_set_tip_force")
    fleet.step(50)
    kw = dict(select=63, near_limit_proximity=0.2, tip_deviation=0.002)
    got = fleet.scan_health(**kw)
    assert got.shape == (n,) and got["flags"].any()
    seen = np.zeros(n, dtype=bool)
    for handle, m, _, ids in fleet.parts():
        view = BatchEngine.view(handle, fleet.params[m], len(ids))
        h, _ = view.scan_health(**kw)
        assert got[ids].tobytes() == h.tobytes(), f"part of morphology {m}"
        want, _ = numpy_health(view, **kw)
        hn.assert_records_match(h, want, f"fleet part of morphology {m}")
        seen[ids] = True
    assert seen.all()
    fleet.close()
