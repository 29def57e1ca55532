"""numpy restatement of the health scan's record (shc_robot_health, include/shc_batch.h), written from the reference lines it cites -
not from csrc/shc_health.hpp - for tests/test_health_layout.py (CPU) and tests/test_gpu_health.py.

  Leg::updateJointPositions (src/model.cpp:799-857)
      :803       min_limit_proximity starts at 1.0
      :812-821   velocity clamp: |desired_velocity_| > max_angular_speed_ -> clamped to it (the state it leaves: |qd| / max >= 1)
      :827-841   position clamp: desired_position_ < min -> min, > max -> max (the state it leaves: q <= min or q >= max)
      :845-849   min_diff = |min - q|, max_diff = |max - q|, half_joint_range = (max - min) / 2,
                 limit_proximity = half_joint_range != 0 ? min(min_diff, max_diff) / half_joint_range : 1.0; the minimum is kept
  Leg::setDesiredTipPose (:653-663)   desired_tip_pose_ = poser tip (+ admittance_delta_ unless the leg is MANUAL / WALKING_TO_MANUAL)
  Leg::applyIK (:916-929)             position_error = current_tip_pose_ - desired_tip_pose_; |error[i]| > IK_TOLERANCE (0.005) is the warning

Minima / maxima ignore NaN operands (np.fmin / np.fmax, like C's fmin / fmax), so the flags of a non-finite robot are defined; its three
doubles are unspecified by the ABI and not compared.
"""
import numpy as np

IK_DEVIATION, POSITION_LIMIT, SPEED_LIMIT, NEAR_LIMIT, TIP_DEVIATION, NONFINITE = 1, 2, 4, 8, 16, 32
IK_TOLERANCE = 0.005  # model.h:17

DTYPE = np.dtype([("min_limit_proximity", "<f8"), ("max_tip_deviation", "<f8"), ("max_speed_ratio", "<f8"), ("flags", "<u4"), ("leg_masks", "<u4")])


def joint_limits(p):
    """(min, max, max_vel, own) as [legs][longest DOF] arrays; own = the joint belongs to the leg (legs may differ in DOF)."""
    L = p.leg_count
    D = max(p.leg_dof[l] for l in range(L))
    lo, hi, vmax, own = np.zeros((L, D)), np.zeros((L, D)), np.ones((L, D)), np.zeros((L, D), dtype=bool)
    for l in range(L):
        for j in range(p.leg_dof[l]):
            lo[l, j], hi[l, j], vmax[l, j], own[l, j] = p.joint[l][j].min, p.joint[l][j].max, p.joint[l][j].max_vel, True
    return lo, hi, vmax, own


def robot_health(p, q, qd, poser_tip, model_tip, admittance, leg_status, pose7, select=0, near_limit_proximity=None, tip_deviation=None,
                 walker_tip=None, apply_delta=None):
    """Records (DTYPE, shape (n,)) and the selection mask for n robots.  q, qd: (n, legs * D) or (n, legs, D); tips / admittance (n, legs, 3);
    leg_status (n, legs) with bit 2 = IK deviation; pose7 (n, 7).  near_limit_proximity / tip_deviation None = the threshold is unused (NULL
    criteria).  apply_delta (n, legs) bool: False for MANUAL / WALKING_TO_MANUAL legs (default: every leg applies it)."""
    L = p.leg_count
    lo, hi, vmax, own = joint_limits(p)
    D = lo.shape[1]
    q, qd = np.asarray(q, dtype=np.float64).reshape(-1, L, D), np.asarray(qd, dtype=np.float64).reshape(-1, L, D)
    n = q.shape[0]
    poser_tip, model_tip, admittance = (np.asarray(a, dtype=np.float64).reshape(n, L, 3) for a in (poser_tip, model_tip, admittance))
    leg_status, pose7 = np.asarray(leg_status).reshape(n, L), np.asarray(pose7, dtype=np.float64).reshape(n, 7)
    walker_tip = np.zeros((n, L, 3)) if walker_tip is None else np.asarray(walker_tip, dtype=np.float64).reshape(n, L, 3)
    apply_delta = np.ones((n, L), dtype=bool) if apply_delta is None else np.asarray(apply_delta, dtype=bool).reshape(n, L)

    with np.errstate(invalid="ignore", divide="ignore"):
        half = (hi - lo) / 2.0                                                       # :847
        prox = np.fmin(np.abs(lo - q), np.abs(hi - q)) / np.where(half != 0, half, 1.0)  # :845-848
        prox = np.where(own & (half != 0), prox, 1.0)
        min_prox = np.fmin(1.0, np.fmin.reduce(prox.reshape(n, -1), axis=1))         # :803, :849
        on_limit = (own & (half != 0) & ((q <= lo) | (q >= hi))).any(axis=2)         # :827-841
        ratio = np.where(own, np.abs(qd) / vmax, 0.0)                                # :814
        max_ratio = np.fmax(0.0, np.fmax.reduce(ratio.reshape(n, -1), axis=1))
        on_speed = (own & (ratio >= 1.0)).any(axis=2)                                # :812-821
        desired = poser_tip + np.where(apply_delta[..., None], admittance, 0.0)      # :656-661
        err = np.abs(model_tip - desired)                                            # :918
        max_dev = np.fmax(0.0, np.fmax.reduce(err.reshape(n, -1), axis=1))
    ik = (leg_status & 4) != 0                                                       # :916-929, leg_status bit 2
    bad_leg = ~(np.isfinite(np.where(own, q, 0.0)).all(axis=2) & np.isfinite(np.where(own, qd, 0.0)).all(axis=2) & np.isfinite(walker_tip).all(axis=2)
                & np.isfinite(poser_tip).all(axis=2) & np.isfinite(model_tip).all(axis=2) & np.isfinite(admittance).all(axis=2))
    bit = (1 << np.arange(L)).astype(np.uint32)
    masks = ((ik * bit).sum(axis=1) | ((on_limit * bit).sum(axis=1) << 8) | ((on_speed * bit).sum(axis=1) << 16) | ((bad_leg * bit).sum(axis=1) << 24)).astype(np.uint32)
    flags = np.zeros(n, dtype=np.uint32)
    flags |= np.where(ik.any(axis=1), IK_DEVIATION, 0).astype(np.uint32)
    flags |= np.where(on_limit.any(axis=1), POSITION_LIMIT, 0).astype(np.uint32)
    flags |= np.where(on_speed.any(axis=1), SPEED_LIMIT, 0).astype(np.uint32)
    flags |= np.where(bad_leg.any(axis=1) | ~np.isfinite(pose7).all(axis=1), NONFINITE, 0).astype(np.uint32)
    if near_limit_proximity is not None:
        flags |= np.where(min_prox < near_limit_proximity, NEAR_LIMIT, 0).astype(np.uint32)
    if tip_deviation is not None:
        flags |= np.where(max_dev > tip_deviation, TIP_DEVIATION, 0).astype(np.uint32)
    out = np.zeros(n, dtype=DTYPE)
    out["min_limit_proximity"], out["max_tip_deviation"], out["max_speed_ratio"], out["flags"], out["leg_masks"] = min_prox, max_dev, max_ratio, flags, masks
    return out, (flags & np.uint32(select)) != 0


# The cases both test files plant, one at a time, into an otherwise healthy robot: name -> (flags that must be raised, flags that must stay clear)
CASES = {
    "joint exactly on min": (POSITION_LIMIT, SPEED_LIMIT | IK_DEVIATION | NONFINITE),
    "joint exactly on max": (POSITION_LIMIT, SPEED_LIMIT | IK_DEVIATION | NONFINITE),
    "zero-range joint": (0, POSITION_LIMIT | SPEED_LIMIT | IK_DEVIATION | NONFINITE | NEAR_LIMIT),
    "rate exactly at max_angular_speed": (SPEED_LIMIT, POSITION_LIMIT | IK_DEVIATION | NONFINITE),
    "deviation just below 5 mm": (0, TIP_DEVIATION | NONFINITE),
    "deviation just above 5 mm": (TIP_DEVIATION, NONFINITE),
    "deviation above a caller threshold": (TIP_DEVIATION, NONFINITE),
    "leg_status bit 2 on two legs": (IK_DEVIATION, POSITION_LIMIT | SPEED_LIMIT | NONFINITE),
    "one NaN angle": (NONFINITE, IK_DEVIATION),
    "one Inf pose component": (NONFINITE, IK_DEVIATION | POSITION_LIMIT | SPEED_LIMIT),
}


def assert_records_match(got, want, what=""):
    """Flags and masks equal; for finite robots the two ratios within 2 ulp (2.3e-16 relative to 1.0: the same correctly rounded operations run
    on both sides, with at most a reciprocal-multiply in place of the division) and the tip deviation within 1e-15 m (one add, one subtract,
    on values below 1 m)."""
    assert np.array_equal(got["flags"], want["flags"]), (what, "flags", got["flags"].tolist(), want["flags"].tolist())
    assert np.array_equal(got["leg_masks"], want["leg_masks"]), (what, "leg_masks", [hex(v) for v in got["leg_masks"]], [hex(v) for v in want["leg_masks"]])
    ok = (want["flags"] & NONFINITE) == 0
    for f in ("min_limit_proximity", "max_speed_ratio"):
        d = np.abs(got[f][ok] - want[f][ok]) / np.maximum(1.0, np.abs(want[f][ok]))
        assert d.size == 0 or d.max() <= 2.3e-16, (what, f, float(d.max()))
    d = np.abs(got["max_tip_deviation"][ok] - want["max_tip_deviation"][ok])
    assert d.size == 0 or d.max() <= 1e-15, (what, "max_tip_deviation", float(d.max()))
