"""Health scan (shc_engine_scan_health), the part that needs no GPU: the exported symbols, the record and criteria layouts against the ctypes /
numpy mirrors, and the arithmetic of one robot - shc_debug_robot_health runs the two functions the scan kernel runs (leg_health, robot_health of
csrc/shc_health.hpp) on the host - against the numpy restatement of the reference lines (tests/health_numpy.py), case by case."""
import ctypes as C

import numpy as np
import pytest

import health_numpy as hn
from syropod_highlevel_controller_amd import default_hexapod_params, engine, synthetic_mixed_dof_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, SHC_OK, HealthCriteria, RobotHealth

SYMBOLS = ["shc_engine_scan_health", "shc_fleet_scan_health", "shc_debug_robot_health"]
ROBOTS = {"hexapod 6x3": lambda: default_hexapod_params("tripod"), "octopod 8x5": lambda: synthetic_octopod_params("ripple", 5, 8),
          "mixed DOF 353 454": lambda: synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4))}


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert hasattr(engine.BatchEngine, "scan_health")   # the fourth: the Python entry point
    assert lib.shc_abi_version() == 6


def test_record_and_criteria_layouts():
    assert C.sizeof(RobotHealth) == 32 and C.sizeof(HealthCriteria) == 24
    dt = engine.ROBOT_HEALTH_DTYPE
    assert dt.itemsize == 32
    want = {"min_limit_proximity": (0, np.float64), "max_tip_deviation": (8, np.float64), "max_speed_ratio": (16, np.float64), "flags": (24, np.uint32),
            "leg_masks": (28, np.uint32)}
    assert set(dt.names) == set(want)
    for name, (offset, typ) in want.items():
        assert dt.fields[name][1] == offset == getattr(RobotHealth, name).offset and dt.fields[name][0] == np.dtype(typ), name
    assert [getattr(HealthCriteria, k).offset for k in ("select", "reserved", "near_limit_proximity", "tip_deviation")] == [0, 4, 8, 16]
    assert (engine.HEALTH_IK_DEVIATION, engine.HEALTH_POSITION_LIMIT, engine.HEALTH_SPEED_LIMIT, engine.HEALTH_NEAR_LIMIT, engine.HEALTH_TIP_DEVIATION,
            engine.HEALTH_NONFINITE) == (1, 2, 4, 8, 16, 32) == (hn.IK_DEVIATION, hn.POSITION_LIMIT, hn.SPEED_LIMIT, hn.NEAR_LIMIT, hn.TIP_DEVIATION, hn.NONFINITE)
    # the library writes the record the mirror describes: one robot with every field distinct
    p = default_hexapod_params("tripod")
    a = healthy(p)
    a["q"][2, 1] = p.joint[2][1].max
    a["qd"][4, 0] = -2.0 * p.joint[4][0].max_vel
    a["leg_status"][5] |= 4
    rec = debug_health(p, a, select=0)
    assert rec["flags"][0] == 7 and rec["leg_masks"][0] == (1 << 5) | (1 << (8 + 2)) | (1 << (16 + 4))
    assert rec["min_limit_proximity"][0] == 0.0 and rec["max_speed_ratio"][0] == 2.0 and 0.0 < rec["max_tip_deviation"][0] < 1e-3


def healthy(p, seed=3):
    """One robot well inside every limit: joints a little off mid-range, rates at 10 .. 30 % of the motors', model tip within 0.2 mm of the
    poser tip + admittance delta, no IK flag, a finite body pose."""
    L = p.leg_count
    lo, hi, vmax, own = hn.joint_limits(p)
    rng = np.random.default_rng(seed)
    q = np.where(own, lo + (hi - lo) * rng.uniform(0.35, 0.65, lo.shape), 0.0)
    qd = np.where(own, vmax * rng.uniform(0.1, 0.3, lo.shape) * rng.choice([-1.0, 1.0], lo.shape), 0.0)
    poser = rng.uniform(-0.3, 0.3, (L, 3))
    adm = rng.uniform(-0.01, 0.01, (L, 3))
    model = poser + adm + rng.uniform(-2e-4, 2e-4, (L, 3))
    return dict(q=q, qd=qd, poser_tip=poser, model_tip=model, admittance=adm, leg_status=np.zeros(L, dtype=np.int32) + 1 + (37 << 8),
                pose7=np.array([0.01, -0.02, 0.0, 1.0, 0.0, 0.0, 0.0]))


def debug_health(p, a, select=0, near_limit_proximity=None, tip_deviation=None, expect=SHC_OK):
    """shc_debug_robot_health on one robot's arrays -> a one-element ROBOT_HEALTH_DTYPE array."""
    crit = None
    if select or near_limit_proximity is not None or tip_deviation is not None:
        crit = C.byref(HealthCriteria(select, 0, -np.inf if near_limit_proximity is None else near_limit_proximity,
                                      np.inf if tip_deviation is None else tip_deviation))
    out = RobotHealth()
    arrs = [np.ascontiguousarray(a[k], dtype=np.float64) for k in ("q", "qd", "poser_tip", "model_tip", "admittance")]
    st, pose = np.ascontiguousarray(a["leg_status"], dtype=np.int32), np.ascontiguousarray(a["pose7"], dtype=np.float64)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = engine.lib().shc_debug_robot_health(C.byref(p), crit, *[ptr(x) for x in arrs], ptr(st), ptr(pose), C.byref(out))
    assert rc == expect, engine.lib().shc_last_error()
    return np.frombuffer(bytes(out), dtype=engine.ROBOT_HEALTH_DTYPE)


def plant(case, p, a, rng):
    """Plants one of health_numpy.CASES into the healthy robot `a` (and, for the zero-range joint, into the parameters).  Returns the criteria
    thresholds the case is judged under and (leg, mask byte) pairs that must be set in leg_masks."""
    L = p.leg_count
    leg = int(rng.integers(0, L))
    j = int(rng.integers(0, p.leg_dof[leg]))
    kw, bits = {}, []
    if case == "joint exactly on min":
        a["q"][leg, j] = p.joint[leg][j].min
        bits = [(leg, 1)]
    elif case == "joint exactly on max":
        a["q"][leg, j] = p.joint[leg][j].max
        bits = [(leg, 1)]
    elif case == "zero-range joint":   # locked where it stands: contributes 1.0 (model.cpp:848) and is on no limit
        p.joint[leg][j].min = p.joint[leg][j].max = a["q"][leg, j]
        kw = dict(near_limit_proximity=0.3)   # every other joint stands in the middle 30 % of its range: proximity >= 0.7
    elif case == "rate exactly at max_angular_speed":
        a["qd"][leg, j] = -p.joint[leg][j].max_vel
        bits = [(leg, 2)]
    elif case.startswith("deviation"):
        axis = int(rng.integers(0, 3))
        target, thr = {"deviation just below 5 mm": (hn.IK_TOLERANCE - 1e-9, hn.IK_TOLERANCE), "deviation just above 5 mm": (hn.IK_TOLERANCE + 1e-9, hn.IK_TOLERANCE),
                       "deviation above a caller threshold": (0.002, 0.0015)}[case]
        a["model_tip"][leg, axis] = a["poser_tip"][leg, axis] + a["admittance"][leg, axis] - target
        kw = dict(tip_deviation=thr)
    elif case == "leg_status bit 2 on two legs":
        a["leg_status"][[1, L - 1]] |= 4
        bits = [(1, 0), (L - 1, 0)]
    elif case == "one NaN angle":
        a["q"][leg, j] = np.nan
        bits = [(leg, 3)]
    elif case == "one Inf pose component":
        a["pose7"][int(rng.integers(0, 7))] = -np.inf
    else:
        raise KeyError(case)
    return kw, bits


@pytest.mark.parametrize("case", list(hn.CASES))
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_one_robot_against_the_numpy_restatement(robot, case):
    p = ROBOTS[robot]()
    rng = np.random.default_rng(sum(map(ord, robot + case)))
    a = healthy(p)
    base = debug_health(p, a)
    assert base["flags"][0] == 0 and base["leg_masks"][0] == 0 and base["min_limit_proximity"][0] >= 0.7, "the healthy robot raises nothing"
    kw, bits = plant(case, p, a, rng)
    select = hn.CASES[case][0] or hn.NEAR_LIMIT
    got = debug_health(p, a, select=select, **kw)
    want, chosen = hn.robot_health(p, a["q"][None], a["qd"][None], a["poser_tip"][None], a["model_tip"][None], a["admittance"][None], a["leg_status"][None],
                                   a["pose7"][None], select=select, **kw)
    hn.assert_records_match(got, want, what=f"{robot}: {case}")
    must_set, must_clear = hn.CASES[case]
    assert got["flags"][0] & must_set == must_set and got["flags"][0] & must_clear == 0, (case, int(got["flags"][0]))
    for leg, byte in bits:
        assert got["leg_masks"][0] >> (8 * byte + leg) & 1, (case, leg, byte, hex(got["leg_masks"][0]))
    assert bool(chosen[0]) == bool(must_set), "selected exactly when the case raises the flag it selects on"
    if case == "zero-range joint":
        assert got["min_limit_proximity"][0] >= 0.7


def test_null_criteria_and_refusals():
    p = default_hexapod_params("tripod")
    a = healthy(p)
    a["model_tip"][0, 0] += 0.02
    a["q"][1, 1] = p.joint[1][1].min + 1e-6
    rec = debug_health(p, a)   # NULL criteria: the two thresholds are unused
    assert rec["flags"][0] == 0 and rec["max_tip_deviation"][0] > 0.019 and rec["min_limit_proximity"][0] < 1e-5
    rec = debug_health(p, a, select=24, near_limit_proximity=0.01, tip_deviation=0.005)
    assert rec["flags"][0] == hn.NEAR_LIMIT | hn.TIP_DEVIATION
    debug_health(p, a, select=64, expect=SHC_ERR_INVALID_ARG)
    lib = engine.lib()
    assert lib.shc_debug_robot_health(C.byref(p), None, None, None, None, None, None, None, None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_scan_health(None, 0, 0, None, None, None, None, None, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_scan_health(None, None, None) == SHC_ERR_INVALID_ARG
