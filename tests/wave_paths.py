"""The wave-uniform shortcuts of the cycle kernels as a table, a classifier that says which side of each a run was on, and the scenarios that reach both.

Every `__all(` / `__any(` / `__ballot(` in csrc/shc_cycle.hpp, csrc/shc_walk_front_body.hpp and csrc/shc_cycle_kernel.hpp makes what the code does for one robot
depend on the other robots of its wavefront.  GUARDS has one entry per site: where it is (file, enclosing function, the guard's text), what a configuration must
have for the site to be compiled in and reached (`needs`), and a per-robot predicate - a numpy function of the oracle's state record before the cycle, the
inputs in force and the parameters (Ctx) - that says how each robot votes: YES, NO, UNSURE (the host cannot know the exact floating-point outcome: never
counted) or ABSENT (the robot's lanes do not take part in the vote: the site sits in a branch they did not enter).  Where the record after the cycle is the only
exact witness of a decision made in the middle of the cycle (the walk state machine's leg bookkeeping, the manual pose a reset drives) the predicate reads
Ctx.after as well, and says so.  EXEMPT lists the sites that are plumbing or cannot be steered from outside.

Which robots share a wavefront (wave_of).  cycle_wave (shc_cycle_kernel.hpp) puts robots rob0 = wave * RPW .. rob0 + RPW - 1, RPW = 64 / L, on wavefront
`wave`: `const int64_t rob0 = wave * RPW`, lane -> group `grp = lane / L`, and the resident forms address `rob = wave * RPW + r` (resident_take_inputs).  The
engine stores instance i at robot i: slot_of(rob, leg, L) = (rob / rpw) * 64 + (rob % rpw) * L + leg and rob_index(r, ...) with r / rpw, r % rpw (shc_engine.hip),
n_waves = ceil(n / rpw).  shc_cycle_half_kernel - the two launches of the rotation-constrained cycle - calls the same cycle_wave with the same wave index for
both halves, so the 8 x 5 cycle groups robots in the same way.  Lanes without a robot (64 % L tail lanes, groups past the end of the batch in the last wave)
mirror the LAST live robot of the wave (`if (grp >= robots_here) grp = robots_here - 1`): they vote as that robot does and never change a vote's outcome.

In divergent code the builtins vote over the lanes that are active, which is why a predicate can be ABSENT for a robot.
"""
import os
import re

import numpy as np

from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.params import FEAT_DEFAULT, InstanceState
from test_gpu_teacher_forced import Schedule

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "syropod_highlevel_controller_amd", "csrc")
FILES = ("shc_cycle.hpp", "shc_walk_front_body.hpp", "shc_cycle_kernel.hpp")
INCLUDED = "(included text)"   # shc_walk_front_body.hpp is a run of statements, no function

YES, NO, UNSURE, ABSENT = 1, 0, -1, -2
WS_STARTING, WS_MOVING, WS_STOPPING, WS_STOPPED = 0, 1, 2, 3
SS_FORCE_STOP = 3
K_MIN = 3   # wave-cycles of every required class, per guard

UNIFORM_TAKEN, UNIFORM_NOT_TAKEN, MIXED, UNDECIDED, NOT_REACHED = "UNIFORM_TAKEN", "UNIFORM_NOT_TAKEN", "MIXED", "UNDECIDED", "NOT_REACHED"
LONE_FIRST, LONE_INNER, LONE_LAST, LONE_PARTIAL = "LONE_DISSENT(first)", "LONE_DISSENT(inner)", "LONE_DISSENT(last)", "LONE_DISSENT(partial wave)"
REQUIRED = (UNIFORM_TAKEN, UNIFORM_NOT_TAKEN, LONE_FIRST, LONE_LAST, LONE_PARTIAL)
LONE = (LONE_FIRST, LONE_LAST, LONE_PARTIAL)


def wave_of(robot, L):
    return np.asarray(robot) // (64 // L)


def as_np(states):
    return np.frombuffer(states, dtype=np.dtype(InstanceState)).copy()


def tri(yes, no):
    """YES where `yes`, NO where `no`, UNSURE elsewhere."""
    return np.where(yes, YES, np.where(no, NO, UNSURE)).astype(np.int8)


def both(v):
    return tri(v, ~v)


def bearing_bracket(y, x):
    """bearing_bracket of shc_cycle.hpp; second result: the point lies so close to a sector edge that the host cannot know the bracket."""
    kc, ks = 0.99996192306417128874, 0.0087265354983739347
    xr, yr = kc * x - ks * y, ks * x + kc * y
    ax, ay = np.abs(xr), np.abs(yr)
    upper = (yr > 0.0) | ((yr == 0.0) & (xr > 0.0))
    up = np.where(xr > 0.0, np.where(ay < ax, 0, 1), np.where(ay > ax, 2, 3))
    lo = np.where(xr < 0.0, np.where(ay < ax, 4, 5), np.where(ay > ax, 6, 7))
    zero = (x == 0.0) & (y == 0.0)
    scale = ax + ay
    edgy = ~zero & ((np.abs(ay - ax) <= 1e-9 * scale) | (ax <= 1e-9 * scale) | (ay <= 1e-9 * scale))
    return np.where(zero, 0, np.where(upper, up, lo)), edgy


class Ctx:
    """What a predicate may read: one cycle of one run.  before / after: the state records around the cycle (structured arrays, one row per robot)."""

    def __init__(self, p, tables, features, before, after, inforce, loop_memo=None):
        self.p, self.tables, self.features, self.before, self.after, self.inp = p, tables, features, before, after, inforce
        self.L = p.leg_count
        self.n = len(before)
        self.wave = wave_of(np.arange(self.n), self.L)
        self.memo = loop_memo   # None in a launch form: every launch starts with fresh memos
        b = before
        self.ws = b["walk_state"]
        self.lin, self.ang = np.asarray(inforce["lin"], dtype=float), np.asarray(inforce["ang"], dtype=float)
        self.lin_n2 = self.lin[:, 0] * self.lin[:, 0] + self.lin[:, 1] * self.lin[:, 1]
        self.has_cmd = (self.lin_n2 != 0.0) | (self.ang != 0.0)
        self.steady = (self.ws == WS_MOVING) & self.has_cmd          # (no manual legs in these runs: no robot is frozen)
        self.early_return = (self.ws == WS_STOPPED) & self.has_cmd   # STOPPED -> STARTING: updateWalk returns before the steppers (:545)
        self.may_stop = (self.ws == WS_STOPPING) | ((self.ws == WS_MOVING) & ~((self.ang != 0.0) | (np.abs(self.lin) > 1e-100).any(axis=1)))
        leg_b, leg_a = b["leg"][:, :self.L], after["leg"][:, :self.L]
        self.stepping_leg = leg_a["step_state"] != SS_FORCE_STOP      # (after: what the state machine of this cycle left)
        self.any_stepping = self.stepping_leg.any(axis=1)
        # the walk state the leg bookkeeping of this cycle runs under
        lacp, lcfs = b["legs_at_correct_phase"], b["legs_completed_first_step"]
        self.moving_now = ((self.ws == WS_STARTING) & (lacp == self.L) & (lcfs == self.L)) | ((self.ws == WS_MOVING) & self.has_cmd)
        # LegStepper::updateDefaultTipPosition on the STOPPING -> FORCE_STOP edge (after: the leg's step state says that the edge was taken)
        self.update_default_leg = (leg_a["step_state"] == SS_FORCE_STOP) & (leg_b["step_state"] != SS_FORCE_STOP) & (after["walk_state"] == WS_STOPPING)[:, None]
        # scaled swing progress of the legs as the previous iteratePhase left it (pose_controller.cpp:1100-1108): the LAST leg within [0, 1] drives the pose
        scaler = max(1.0, float(p.swing_phase) / p.phase_offset)
        sp = leg_b["swing_progress"] * scaler
        ok = (leg_b["swing_progress"] >= 0.0) & (sp >= 0.0) & (sp <= 1.0)
        self.sel = ok.any(axis=1)
        last = self.L - 1 - np.argmax(ok[:, ::-1], axis=1)
        self.c_one = self.sel & (sp[np.arange(self.n), last] == 1.0)   # (it + 1) / swing iterations == 1: smoothStep(1) = 1 exactly
        uz = np.array([0.0, 0.0, 1.0])
        self.pnorm_prev_flat = (b["stepper_walk_plane_normal"] == uz).all(axis=1)
        self.pnorm_flat = (b["walk_plane_normal"] == uz).all(axis=1)
        ident = np.array([1.0, 0.0, 0.0, 0.0])
        self.owpp_upright = (b["origin_walk_plane_pose"][:, 3:] == ident).all(axis=1)
        self.flat = (~self.sel | self.pnorm_prev_flat) & self.owpp_upright
        self.planes_same = (b["walk_plane"] == b["stepper_walk_plane"]).all(axis=1) & (b["walk_plane_normal"] == b["stepper_walk_plane_normal"]).all(axis=1)
        # manual pose
        reset = np.asarray(inforce.get("reset", np.zeros(self.n, dtype=np.int32)))
        self.idle = (reset == 0) & (b["translation_velocity_input"] == 0.0).all(axis=1) & (b["rotation_velocity_input"] == 0.0).all(axis=1)
        ident7 = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        m = after["manual_pose"]                                      # (after: the pose this cycle's updateManualPose leaves)
        exact = (m == ident7).all(axis=1) & (self.idle | (reset == 5))   # held, or IMMEDIATE_ALL_RESET: the identity by assignment, no arithmetic
        self.unposed = tri(exact, np.abs(m - ident7).max(axis=1) > 1e-9)
        self.rot_identity = tri(exact, np.abs(m[:, 3:] - ident).max(axis=1) > 1e-9)
        self._front()

    def _front(self):
        """The velocity front (shc_walk_front_body.hpp) on the host, with the oracle's limit tables (they agree with the engine's to 1e-9 relative)."""
        b, t = self.before, self.tables
        tip = b["leg"]["walker_tip"][:, :self.L]
        sx = self.lin[:, 0, None] - self.ang[:, None] * tip[:, :, 1]
        sy = self.lin[:, 1, None] + self.ang[:, None] * tip[:, :, 0]
        self.bracket, edgy = bearing_bracket(sy, sx)
        self.bracket_unsure = edgy.any(axis=1)
        tab = np.stack([np.array(t.max_linear_speed[:8]), np.array(t.max_angular_speed[:8]), np.array(t.max_linear_acceleration[:8]),
                        np.array(t.max_angular_acceleration[:8])], axis=1)
        lim = tab[self.bracket].min(axis=1)          # [n, 4]
        n2 = self.lin_n2
        self.n2_le1 = tri(n2 <= 1.0 - 1e-12, n2 >= 1.0 + 1e-12)
        norm = np.sqrt(n2)
        k = np.where(norm > 1.0, 1.0 / np.maximum(norm, 1e-300), 1.0)
        sc = 1.0 - np.abs(self.ang)
        nv = self.lin * k[:, None] * lim[:, 0, None] * sc[:, None]
        nv[self.ws == WS_STOPPING] = 0.0
        v = b["desired_linear_velocity"]
        a = nv - v
        an = np.sqrt((a * a).sum(axis=1))
        cap = lim[:, 2] * self.p.time_delta
        at_rest = (nv == 0.0).all(axis=1) & (v == 0.0).all(axis=1)   # 0 - 0: exact on any table
        self.an2_zero = tri(at_rest, an > 1e-7)                      # (a robot AT its non-zero target is 1e-9 relative off it on the engine's own table)
        self.an_lt_cap = tri(an < cap * (1.0 - 1e-6), an > cap * (1.0 + 1e-6))
        self.an_lt_cap[self.bracket_unsure] = UNSURE
        ha = 0.5 * self.after["desired_angular_velocity"] * self.p.time_delta
        self.small_yaw = tri(np.abs(ha) <= 0.4, np.abs(ha) >= 0.6)

    def wave_any(self, v):
        out = np.zeros(self.wave.max() + 1, dtype=bool)
        np.logical_or.at(out, self.wave, v)
        return out[self.wave]

    def absent(self, vote, where):
        return np.where(where, ABSENT, vote).astype(np.int8)


# ------------------------------------------------------------------------------------------------ predicates
def p_bracket_memo(x):
    if x.memo is None:      # a launch form: fb is fresh, limit_bracket = -1 matches no bracket
        return np.full(x.n, NO, dtype=np.int8)
    held = x.memo.setdefault("bracket", np.full((x.n, x.L), -1))
    vote = tri((x.bracket == held).all(axis=1) & ~x.bracket_unsure, (x.bracket != held).any(axis=1) & ~x.bracket_unsure)
    miss = np.zeros(x.wave.max() + 1, dtype=bool)
    np.logical_or.at(miss, x.wave, vote != YES)
    held[miss[x.wave]] = x.bracket[miss[x.wave]]   # a wave that misses (or may have) keeps the brackets of this cycle
    return vote


def p_odom_cache(x):
    """OdomCache: each lane keeps the half yaw step of the wave's last miss.  Exact on the records of the engine that runs the same cycles (the twin)."""
    if x.memo is None:      # no launch form passes a cache
        return np.full(x.n, ABSENT, dtype=np.int8)
    ha = 0.5 * (x.after["desired_angular_velocity"] * x.p.time_delta)
    held = x.memo.setdefault("odom_ha", np.full(x.n, np.nan))
    vote = x.absent(both(ha == held), x.early_return)
    miss = np.zeros(x.wave.max() + 1, dtype=bool)
    np.logical_or.at(miss, x.wave, vote == NO)
    store = miss[x.wave] & ~x.early_return
    held[store] = ha[store]
    return vote


def in_loop(fn):
    """A site that only the resident 6 x 3 loop runs: no robot takes part in a launch form."""
    def pred(x):
        return np.full(x.n, ABSENT, dtype=np.int8) if x.memo is None else fn(x)
    return pred


def p_planes_in_sync(x):
    """fb.planes_in_sync: while it holds the comparison (and this vote) is skipped; a default tip that moves clears it (`__any(default_changed)`)."""
    nw = x.wave.max() + 1
    in_sync = x.memo.setdefault("planes_in_sync", np.zeros(nw, dtype=bool))
    reach = ~x.early_return
    vote = x.absent(both(x.planes_same | x.any_stepping), ~reach | in_sync[x.wave])
    new = np.ones(nw, dtype=bool)
    np.logical_and.at(new, x.wave, (vote == YES) | (vote == ABSENT))
    voted = np.zeros(nw, dtype=bool)
    np.logical_or.at(voted, x.wave, vote != ABSENT)
    in_sync[voted] = new[voted]
    changed = np.zeros(nw, dtype=bool)
    np.logical_or.at(changed, x.wave, reach & x.update_default_leg.any(axis=1))
    in_sync[changed] = False
    return vote


def p_walker_dirty(x):
    """DIRTY_SWING_ORG / DIRTY_STANCE_ORG: a leg in the first iteration of a swing or stance period (after: the origins are the witness)."""
    b, a = x.before["leg"][:, :x.L], x.after["leg"][:, :x.L]
    return both(((a["stance_origin_tip"] != b["stance_origin_tip"]).any(axis=2) | (a["swing_origin_tip"] != b["swing_origin_tip"]).any(axis=2)).any(axis=1))


def p_lin_norm_gt1(x):
    # (while every robot of the wave is inside the disc lin_norm is the stand-in 0.5 / 0: not above 1 either)
    return np.where(x.n2_le1 == UNSURE, UNSURE, 1 - x.n2_le1).astype(np.int8)


def p_pnp_flat(x):
    return x.absent(both(x.pnorm_prev_flat), ~x.wave_any(x.may_stop))


def p_owpp_changed(x):
    """`!same` behind `c == 1.0`: the walk-plane pose reached at the end of a swing differs from the origin it started from."""
    b = x.before
    owpp, owpp_after = b["origin_walk_plane_pose"], x.after["origin_walk_plane_pose"]
    wave_flat = ~x.wave_any(~x.flat)
    npp = np.zeros((x.n, 7))
    npp[:, 2] = x.p.body_clearance + b["stepper_walk_plane"][:, 2]
    npp[:, 3] = 1.0
    same_flat = (owpp == npp).all(axis=1)      # flat path with c = 1: npp * 1 + owpp.p * 0, identity rotation
    # The general path (after: the store of OWPP is the witness).  A robot that is flat itself takes it with the identity rotation and c = 1: products with
    # 0 and 1 only, exact on both sides; for a tilted robot only a change well above rounding is certain.
    d = np.abs(owpp_after - owpp).max(axis=1)
    vote = np.where(wave_flat, both(~same_flat), tri(d > 1e-9, x.flat & (d == 0.0)))
    return x.absent(vote, ~x.c_one)


def p_all_moving(x):
    steady_wave = ~x.wave_any(~x.steady)
    return x.absent(both(x.moving_now), steady_wave | x.early_return)


def p_update_default(x):
    return x.absent(both(x.update_default_leg.any(axis=1)), x.early_return)


def p_flat_n_straight(x):
    rough_form = bool(x.p.rough_terrain_mode) or bool(x.p.force_normal_touchdown)
    return x.absent(both(x.pnorm_flat), x.early_return | rough_form)


def p_flat_n_branching(x):
    rough_form = bool(x.p.rough_terrain_mode) or bool(x.p.force_normal_touchdown)
    return x.absent(both(x.pnorm_flat), x.early_return | ~x.any_stepping | (not rough_form))


def p_planes_differ(x):
    return x.absent(both(~x.planes_same), x.early_return | ~x.any_stepping)


def p_default_changed(x):
    if x.p.rough_terrain_mode:   # + the defaults re-derived at every swing / stance start
        return np.full(x.n, UNSURE, dtype=np.int8)
    return x.absent(both(x.update_default_leg.any(axis=1)), x.early_return)


def p_rough_update_default(x):
    """A stepping leg in the first iteration of a swing or stance period: the only place that writes the swing / stance origin (after: the origins are the
    witness; a leg whose tip rests on its old origin would rewrite the same value: unknowable)."""
    b, a = x.before["leg"][:, :x.L], x.after["leg"][:, :x.L]
    changed = (a["stance_origin_tip"] != b["stance_origin_tip"]).any(axis=2) | (a["swing_origin_tip"] != b["swing_origin_tip"]).any(axis=2)
    rests = (b["walker_tip"] == b["stance_origin_tip"]).all(axis=2) | (b["walker_tip"] == b["swing_origin_tip"]).all(axis=2)
    yes = (changed & x.stepping_leg).any(axis=1)
    unsure = (rests & ~changed & x.stepping_leg).any(axis=1)
    return x.absent(tri(yes, ~yes & ~unsure), x.early_return | ~x.any_stepping)


def p_small_yaw(x):
    return x.absent(x.small_yaw, x.early_return)


def p_tgt_unit(x):
    # identity: |q|^2 = 1 exactly.  A posed target is a product of three half-angle rotations, a few ulp from unit norm: unknowable on the host
    return tri(x.rot_identity == YES, np.zeros(x.n, dtype=bool))


def p_tgt_posed(x):
    return np.where(x.rot_identity == UNSURE, UNSURE, 1 - x.rot_identity).astype(np.int8)


def p_not_unposed(x):
    return x.unposed


class Guard:
    def __init__(self, gid, file, function, text, kind, needs, predicate, occurrence=1, waived=None, note="", per_launch=False):
        self.per_launch = per_launch   # one vote at the end of a resident launch, over what the launch's cycles left: a robot votes YES if it did in any cycle
        self.id, self.file, self.function, self.text, self.kind, self.needs, self.predicate = gid, file, function, text, kind, frozenset(needs), predicate
        self.occurrence, self.waived, self.note = occurrence, dict(waived or {}), note
        assert kind in ("all", "any")

    def required(self):
        return [c for c in REQUIRED if c not in self.waived]


ONLY_FLAT = "without rough terrain no default tip ever leaves the plane z = 0: the walk-plane normal is (0, 0, 1) in every robot"
FLAT_WAIVER = {UNIFORM_NOT_TAKEN: ONLY_FLAT, LONE_FIRST: ONLY_FLAT, LONE_LAST: ONLY_FLAT, LONE_PARTIAL: ONLY_FLAT}
NO_TILT_IN_LOOP = "the resident 6 x 3 loop has no rough-terrain form: default tips stay on z = 0, every plane fit returns the plane it replaces, no robot ever votes NO"
CY, FB, CK = FILES

GUARDS = [
    # ---- velocity front
    Guard("front.bracket_memo", FB, INCLUDED, "if (__all(idx == fb.limit_bracket)) {", "all", {"loop"}, p_bracket_memo,
          note="a memo: lives across the cycles of the resident 6 x 3 loop only; every other form - single launches, step_k's batch kernel - starts each "
               "cycle with limit_bracket = -1 (cycle(), shc_cycle.hpp)"),
    Guard("front.inside_disc", FB, INCLUDED, "if (velocity_input_mode == 0 && __all(lin_n2 <= 1.0)) lin_norm = lin_n2 != 0.0 ? 0.5 : 0.0;", "all", {"throttle"},
          lambda x: x.n2_le1),
    Guard("front.outside_disc", FB, INCLUDED, "if (__any(lin_norm > 1.0)) k = lin_norm > 1.0 ? 1.0 / lin_norm : 1.0;", "any", {"throttle"}, p_lin_norm_gt1),
    Guard("front.at_target", FB, INCLUDED, "const double an = __all(an2 == 0.0) ? 0.0 : sqrt(an2);", "all", {"throttle"}, lambda x: x.an2_zero,
          note="decidable on the host only where target and velocity are both exactly zero (a robot at a non-zero target differs from it by the 1e-9 "
               "relative difference of the two sides' limit tables)"),
    Guard("front.below_cap", FB, INCLUDED, "if (__all(an < cap)) {", "all", {"throttle"}, lambda x: x.an_lt_cap),
    # ---- odometry
    Guard("odom.cache", CY, "odometry_advance", "if (cache != nullptr && cache->valid && __all(ha == cache->ha)) {", "all", {"loop", "odometry"}, p_odom_cache,
          note="a memo of the resident 6 x 3 loop (the only caller that passes a cache)"),
    Guard("odom.small_yaw", CY, "odometry_advance", "if (__all(fabs(ha) <= 0.5)) sincos_joint<false>(ha, &sh, &ch);", "all", {"odometry"}, p_small_yaw,
          waived={c: "half a cycle's yaw is bounded by max_angular_speed * time_delta / 2 (milliradians): no input reaches 0.5 rad" for c in (UNIFORM_NOT_TAKEN,) + LONE}),
    # ---- cycle_pose
    Guard("pose.swing_table", CY, "cycle_pose", "if (__any(sel)) c = sel ? C.swing_c[it_sel] : 0.0;", "any", set(), lambda x: both(x.sel)),
    Guard("pose.flat", CY, "cycle_pose", "if (__builtin_expect(__all(flat), 1)) {", "all", {"rough"}, lambda x: both(x.flat)),
    Guard("pose.owpp_store", CY, "cycle_pose", "if (__any(!same)) {", "any", {"rough"}, p_owpp_changed),
    Guard("pose.manual_active", CY, "cycle_pose", "if (__any(!idle)) {", "any", {"manual"}, lambda x: both(~x.idle)),
    Guard("pose.manual_unposed", CY, "cycle_pose", "if (!__all(unposed)) cp = add_pose(cp, mpose);", "all", {"manual"}, p_not_unposed),
    Guard("pose.imu_unit_target", CY, "cycle_pose", "Quat err = normalized(cur * (__all(tgt_n2 == 1.0) ? conj(tgt) : inverse(tgt)));", "all", {"manual", "imu"},
          p_tgt_unit, waived={c: "the host cannot know whether a posed target's |q|^2 rounds to 1.0 (it is within a few ulp): only the identity is certain; "
                                 "the posed side runs wherever pose.imu_posed_target is taken" for c in (UNIFORM_NOT_TAKEN,) + LONE}),
    Guard("pose.imu_posed_target", CY, "cycle_pose", "if (__any(!tgt_identity)) {", "any", {"manual", "imu"}, p_tgt_posed),
    # ---- cycle_front
    Guard("walk.may_stop", CY, "cycle_front", "if (!(SHC_DBG(P) & 128) && __any(may_stop)) {", "any", set(), lambda x: both(x.may_stop)),
    Guard("walk.stop_plane_flat", CY, "cycle_front", "if (__all(pnp.x == 0.0 && pnp.y == 0.0 && pnp.z == 1.0)) err.z = 0.0;", "all", {"rough"}, p_pnp_flat),
    Guard("walk.steady", CY, "cycle_front", "const bool steady = __all(!frozen && walk_state == WS_MOVING && has_cmd) && !(SHC_DBG(P) & 16384);", "all", set(),
          lambda x: both(x.steady)),
    Guard("walk.all_moving", CY, "cycle_front", "if (__all(walk_state == WS_MOVING)) {", "all", set(), p_all_moving),
    Guard("walk.update_default", CY, "cycle_front", "if (__any(my_update_default)) {", "any", set(), p_update_default),
    Guard("walk.flat_normal_straight", CY, "cycle_front", "if (!__all(flat_n)) pn = normalized(pn);", "all", set(), p_flat_n_straight, occurrence=1, waived=FLAT_WAIVER,
          note="the straight form of the stepper runs without rough terrain only"),
    Guard("walk.flat_normal_branching", CY, "cycle_front", "if (!__all(flat_n)) pn = normalized(pn);", "all", {"rough"}, p_flat_n_branching, occurrence=3),
    Guard("walk.rough_update_default", CY, "cycle_front", "if (rough && __any(rough_update_default)) {", "any", {"rough"}, p_rough_update_default),
    Guard("walk.planes_differ", CY, "cycle_front", "if (__any(!same)) {", "any", {"rough"}, p_planes_differ),
    Guard("walk.default_changed", CY, "cycle_front", "if (__any(default_changed)) {", "any", set(), p_default_changed),
    # ---- sites that only the resident 6 x 3 loop runs (shc_resident2_kernel and the forms of cycle_pose / cycle_front it instantiates)
    Guard("loop.pose_swing_table", CY, "walk_plane_control_input", "if (__any(sel)) c = sel ? C.swing_c[it_sel] : 0.0;", "any", {"loop"}, in_loop(lambda x: both(x.sel)),
          note="the OWN_WORD pose; the vote is on the leg words the previous updateWalk left, as pose.swing_table's"),
    Guard("loop.flat_normal_behind_front", CY, "cycle_front", "if (!__all(flat_n)) pn = normalized(pn);", "all", {"loop"}, in_loop(p_flat_n_straight), occurrence=2,
          waived=FLAT_WAIVER, note="the straight form behind the front's flag (FRONT_HERE = false)"),
    Guard("loop.planes_in_sync", CY, "cycle_front", "fb.planes_in_sync = __all(same || any_stepping);", "all", {"loop"}, in_loop(p_planes_in_sync),
          waived={c: NO_TILT_IN_LOOP for c in (UNIFORM_NOT_TAKEN,) + LONE}, note="a memo: the vote runs only while the memo does not hold (after a default tip moved)"),
    Guard("loop.odom_mailbox", CK, "shc_resident2_kernel", "if (__any(mb[384] != 0.0)) {", "any", {"loop", "odometry"}, in_loop(lambda x: both(~x.early_return))),
    Guard("loop.odom_run", CK, "shc_resident2_kernel", "if (FT::odom(P) && __any(fb.odom_run)) {", "any", {"loop", "odometry"}, in_loop(lambda x: both(~x.early_return)),
          note="this site or loop.odom_mailbox runs, by the role that owns the accumulator in the form launched: the same vote"),
    Guard("loop.dirty_pose_role", CK, "shc_resident2_kernel", "if (__any((dirty & b) != 0)) d |= b;", "any", {"loop", "manual"}, in_loop(lambda x: both(~x.idle)),
          occurrence=1, per_launch=True, note="classified on DIRTY_MANUAL, the bit the role that runs the pose can own"),
    Guard("loop.dirty_front_role", CK, "shc_resident2_kernel", "if (__any((dirty & b) != 0)) d |= b;", "any", {"loop", "manual"}, in_loop(lambda x: both(~x.idle)),
          occurrence=2, per_launch=True, note="classified on DIRTY_MANUAL (the fourth role runs the pose in the four-role form)"),
    Guard("loop.dirty_walker", CK, "shc_resident2_kernel", "if (__any((dirty & b) != 0)) d |= b;", "any", {"loop"}, in_loop(p_walker_dirty),
          occurrence=3, per_launch=True, note="the other roles' bits arrive merged, the same in every lane: classified on the walker's own DIRTY_SWING_ORG / DIRTY_STANCE_ORG"),
    # ---- the launch's tail
    Guard("store.dirty", CK, "cycle_wave", "if (__any((dirty & b) != 0)) d |= b;", "any", {"manual"}, lambda x: both(~x.idle),
          note="one site for five dirty bits; classified on DIRTY_MANUAL (the store of the manual-pose group is elided unless some robot's pose ran)"),
]

# Sites that are plumbing, or that no input steers.  (file, function, text, occurrence): reason
EXEMPT = [
    (CK, "resident_relay", "if (__all(word_ok)) {", 1, "ring header: the relay's lanes read the words of ONE record, there is no robot behind a lane"),
    (CY, "quat_to_euler_zyx_grouped", "if (__builtin_expect(__any((r0 < 0.0) != neg), 0)) r1 = atan2(-m20, r0 < 0.0 ? -c2 : c2);", 1,
     "the atan2 sign-prediction fallback, never observed to run: tests/test_math_primitives.py holds the prediction itself"),
    (CY, "walk_plane_control_input", "const unsigned legs_ok = unsigned((__ballot(ok_own) >> g.base) & ((1ull << L) - 1));", 1,
     "a gather: each robot reads the bits of its own group only"),
    (CY, "cycle_front", "any_stepping = ((__ballot((s.word & 3) != SS_FORCE_STOP) >> g.base) & ((1ull << L) - 1)) != 0;", 1,
     "a gather: each robot reads the bits of its own group only"),
    (CY, "cycle_front", "any_stepping = ((__ballot((s.word & 3) != SS_FORCE_STOP) >> g.base) & ((1ull << L) - 1)) != 0;", 2,
     "a gather: each robot reads the bits of its own group only"),
]

# ------------------------------------------------------------------------------------------------ source scan
_FUNC = re.compile(r"(\w+)\s*\(")


def scan_sources(csrc=CSRC):
    """Every line with a wave vote: (file, enclosing function, stripped line, occurrence of that line in that function, line number)."""
    found = []
    for f in FILES:
        function, seen = INCLUDED, {}
        with open(os.path.join(csrc, f)) as fh:
            for no, line in enumerate(fh, 1):
                if line.startswith(("__device__", "__global__")):
                    names = [m.group(1) for m in _FUNC.finditer(line) if m.group(1) not in ("__launch_bounds__", "__attribute__")]
                    function, seen = names[0], {}
                code = line.split("//")[0]
                if re.search(r"__(all|any|ballot)\(", code):
                    text = code.strip()
                    seen[text] = seen.get(text, 0) + 1
                    found.append((f, function, text, seen[text], no))
    return found


def match_sources(found, guards=None, exempt=None):
    """Problems (strings) of the table against the sources: a vote no entry names, one that two do, an entry that names no line."""
    guards, exempt = GUARDS if guards is None else guards, EXEMPT if exempt is None else exempt
    entries = [(g.file, g.function, g.text, g.occurrence, g.id) for g in guards] + [e[:4] + ("exempt",) for e in exempt]
    problems, used = [], [0] * len(entries)
    for f, function, text, occ, no in found:
        hits = [i for i, e in enumerate(entries) if e[0] == f and e[1] == function and e[3] == occ and e[2] in text]
        for i in hits:
            used[i] += 1
        if len(hits) != 1:
            problems.append(f"{f}:{no} in {function} (occurrence {occ}): `{text}` matches {len(hits)} entries {[entries[i][4] for i in hits]}")
    problems += [f"entry {e[4]} ({e[0]}, {e[1]}, occurrence {e[3]}: `{e[2]}`) matches {u} lines" for e, u in zip(entries, used) if u != 1]
    return problems


# ------------------------------------------------------------------------------------------------ classifier
def classify_wave(kind, votes):
    """One wave's class from the votes of its live robots (in robot order), and whether the wave is a partial one (said by the caller)."""
    v = votes[votes != ABSENT]
    if v.size == 0:
        return NOT_REACHED, None
    if (v == UNSURE).any():
        return UNDECIDED, None
    yes = int((v == YES).sum())
    common, lone = (YES, NO) if kind == "all" else (NO, YES)   # the side a lone robot takes the wave away from / the side it takes it to
    if yes == v.size:
        return UNIFORM_TAKEN, None
    if yes == 0:
        return UNIFORM_NOT_TAKEN, None
    if int((v == lone).sum()) == 1 and v.size > 1:
        return "LONE", int(np.flatnonzero(votes == lone)[0])
    return MIXED, None


def classify(guard, x):
    """Per wave: the class of this cycle."""
    votes = guard.predicate(x)
    rpw = 64 // x.L
    out = []
    for w in range((x.n + rpw - 1) // rpw):
        mine = votes[w * rpw:(w + 1) * rpw]
        cls, at = classify_wave(guard.kind, mine)
        if cls == "LONE":
            partial = len(mine) < rpw
            cls = LONE_PARTIAL if partial else (LONE_FIRST if at == 0 else (LONE_LAST if at == len(mine) - 1 else LONE_INNER))
        out.append(cls)
    return out


class Tally:
    """Wave-cycles per guard and class."""

    def __init__(self):
        self.counts = {}

    def add(self, gid, cls, k=1):
        self.counts.setdefault(gid, {}).setdefault(cls, 0)
        self.counts[gid][cls] += k

    def merge(self, other):
        for gid, d in other.counts.items():
            for cls, k in d.items():
                self.add(gid, cls, k)
        return self

    def missing(self, guards, k_min=K_MIN):
        """(guard id, class, count) of every required class that has fewer than k_min wave-cycles."""
        return [(g.id, c, self.counts.get(g.id, {}).get(c, 0)) for g in guards for c in g.required() if self.counts.get(g.id, {}).get(c, 0) < k_min]

    def line(self, gid):
        d = self.counts.get(gid, {})
        return f"{gid}: " + ", ".join(f"{c} {d[c]}" for c in REQUIRED + (LONE_INNER, MIXED, UNDECIDED, NOT_REACHED) if d.get(c))


# ------------------------------------------------------------------------------------------------ scenarios
class WaveSchedule(Schedule):
    """A Schedule that also keeps what the classifier needs: the inputs in force and the oracle's state record at the start of every cycle (teacher_forced
    hands the oracle to fire() once per cycle, after the previous cycle and before this one)."""

    def __init__(self, initial):
        super().__init__()
        self.inforce = {k: np.array(v, copy=True) for k, v in initial.items()}
        self.records, self.inputs = {}, {}
        self.recorder = None   # the object whose state is recorded; None: the oracle among those fire() is given
        self.prestep = 0       # cycles the oracle runs alone before cycle 0 (the start-up of a long gait: teacher forcing takes the engine there)
        self.cuts = ()         # loop runs: the cycles at which the loop is ended and begun again

    def fire(self, cycle, objs):
        if cycle == 0 and self.prestep:
            for o in objs:
                if isinstance(o, OracleBatch):
                    o.step(self.prestep, 8)
        super().fire(cycle, objs)
        for k, v in self.events.get(cycle, {}).items():
            self.inforce[k] = np.array(v, copy=True)
        for o in objs:
            if o is self.recorder or (self.recorder is None and isinstance(o, OracleBatch)):
                self.records[cycle] = as_np(o.get_state())
                self.inputs[cycle] = dict(self.inforce)


def designated(n, L, position):
    """One robot per wave: the first / an inner / the last group of each full wave; the LAST robot of the partial wave whatever the position."""
    rpw = 64 // L
    at = {"first": 0, "inner": rpw // 2, "last": rpw - 1}[position]
    robots = []
    for w in range((n + rpw - 1) // rpw):
        size = min(rpw, n - w * rpw)
        robots.append(w * rpw + (at if size == rpw else size - 1))
    return np.array(robots)


def batch_size(L):
    rpw = 64 // L
    return 2 * rpw + (rpw + 1) // 2   # two full waves and a partial one


MORPHS = {}
KINDS = ("front_pose_stop", "stop_restart")
POSITIONS = ("first", "inner", "last")
ROUGH_RUNS = tuple((k, pos) for k in ("lone_tilt_stop", "late_start") for pos in POSITIONS) + (("all_tilt_stop", "first"), ("flat_stop", "first"))


def morph(name, provides, moving_at, stopped_after, runs=None, only=None, prestep=0):
    """moving_at: the cycle by which every robot is MOVING under the base command; stopped_after: cycles from a zero command to STOPPED (both measured on the
    oracle); runs: the (kind, position) pairs of the morphology's scenarios; only: the feature whose guards this morphology is there for (None: every guard
    its features reach)."""
    def deco(fn):
        MORPHS[name] = (fn, frozenset(provides), (moving_at, stopped_after), runs or tuple((k, pos) for k in KINDS for pos in POSITIONS), only, prestep)
        return fn
    return deco


def _fast(p):
    p.step_frequency = 4.0   # a step cycle of 24 (tripod) / 36 (ripple) iterations: start-up, a stop and a restart fit 150 cycles
    return p


@morph("6x3", {"throttle", "odometry", "manual", "imu"}, 5, 104, prestep=78)
def _m63():
    # config 3 (wave gait, admittance, IMU posing) + manual posing.  The wave gait's shortest step cycle is 72 iterations, its start-up takes 80 cycles and a
    # stop 99: the oracle walks through the start-up alone before cycle 0 (WaveSchedule.prestep), the 150 compared cycles begin with every robot MOVING
    p = _fast(default_hexapod_params("wave"))
    p.admittance_control, p.imu_posing, p.manual_posing = 1, 1, 1
    p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    return p


@morph("8x5", {"throttle", "odometry", "manual"}, 46, 54)
def _m85():
    p = _fast(synthetic_octopod_params("ripple", 5, 8))
    p.gravity_aligned_tips = 1   # the two-launch cycle; L = 8 fills the wavefront exactly
    return p


def _imu_width(gait, dof, legs):
    def make():   # the parameter sets of test_imu_posing_on_every_group_width: idle lanes (L = 5, 7) and the mirror lane (L = 3)
        p = _fast(synthetic_octopod_params(gait, dof, legs))
        p.admittance_control, p.imu_posing = 1, 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
        return p
    return make


for _legs, _dof, _gait in ((3, 3, "tripod"), (5, 3, "ripple"), (7, 3, "ripple")):
    morph(f"{_legs}x{_dof}", {"throttle", "odometry", "manual", "imu"}, 34 if _legs == 3 else 46, 30 if _legs == 3 else 54)(_imu_width(_gait, _dof, _legs))


@morph("6x3-rough", {"throttle", "odometry", "manual", "rough"}, 34, 30, runs=ROUGH_RUNS, only="rough")
def _m63_rough():
    p = _fast(default_hexapod_params("tripod"))
    # step_depth 0: a swing that meets no ground ends on the plane it aimed at, so a robot without tip forces keeps its default tips - and its walk
    # plane - exactly flat, and only a robot whose legs touch down early (a tip force during the swing) tilts
    p.rough_terrain_mode, p.step_depth = 1, 0.0
    return p


LOOP_RUNS = tuple((k, pos) for k in ("front_pose_stop", "stop_restart_posed", "cold_restart") for pos in POSITIONS)


@morph("6x3-loop", {"throttle", "odometry", "manual"}, 34, 30, runs=LOOP_RUNS)
def loop_params():
    return _fast(default_hexapod_params("tripod"))   # the configuration the resident 6 x 3 loop keeps its memos for (and bench.py's headline runs)


def build_scenario(name, kind, position, cycles=150):
    """(params, n, initial inputs, WaveSchedule).  The base command keeps every robot on the common side of every guard: MOVING with a command of its own inside
    the unit disc, no pose input, the identity manual pose, flat ground.  At chosen cycles the designated robot of every wave gets the spoiling input; in other
    stretches every robot does.  The cycle numbers below were chosen on the CPU oracle (tests/test_wave_paths_table.py runs exactly this) so that every guard
    reaches K_MIN wave-cycles of every class it can have, as tests/test_gpu_resident_front.py chooses its SEED."""
    make, provides, (T, stop_len), runs, _, prestep = MORPHS[name]
    assert (kind, position) in runs
    p = make()
    L = p.leg_count
    n = batch_size(L)
    rng = np.random.default_rng(1000 * L + 10 * len(kind) + POSITIONS.index(position))
    d = designated(n, L, position)
    th, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.3, 0.6, n)
    if kind == "front_pose_stop":
        # the designated robots walk close to the rim of the unit disc: a command outside it moves their target by less than three cycles of the acceleration
        # cap, so they REACH the clamped target while the command lasts and the clamp's value is compared, not only the capped approach to it
        r[d] = rng.uniform(0.93, 0.97, len(d))
    lin = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    ang = rng.uniform(0.05, 0.2, n) * rng.choice([-1.0, 1.0], n)
    inp = {"lin": lin, "ang": ang, "effort": rng.normal(0, 0.5, (n, L * p.leg_dof[0]))}
    if p.rough_terrain_mode:
        inp["force"] = np.zeros((n, L, 3))
    if p.imu_posing:
        from test_gpu_parity import make_inputs
        im = make_inputs(p, n, 77 + L, imu=True, force=6.0)
        inp.update(imu_q=im["imu_q"], gyro=im["gyro"], force=im["force"])
    zero3 = np.zeros((n, 3))
    inp.update(tv=zero3.copy(), rv=zero3.copy(), reset=np.zeros(n, dtype=np.int32))
    s = WaveSchedule(inp)
    s.prestep = prestep

    def only(base, value):      # the designated robots get `value`, the others keep `base`
        out = np.array(base, copy=True)
        out[d] = value
        return out

    def vel(c, lin_, ang_):
        s.at(c, lin=lin_, ang=ang_)

    def pose(c, tv, rv, reset):
        s.at(c, tv=tv, rv=rv, reset=reset)

    none, all5 = np.zeros(n, dtype=np.int32), np.full(n, 5, dtype=np.int32)
    push = np.tile([0.6, -0.4, 0.5], (n, 1))
    big = lin / np.linalg.norm(lin, axis=1, keepdims=True) * 1.7
    if kind == "front_pose_stop":
        vel(T, only(lin, big[d]), ang)                 # one robot outside the unit disc: its clamp, and a jump beyond the acceleration cap
        vel(T + 9, lin, ang)                           # ... at its clamped target after three cycles, and back (capped again for a few cycles)
        vel(T + 16, big, ang)                          # every robot outside
        vel(T + 21, lin, ang)
        pose(T + 2, only(zero3, push[d]), only(zero3, -push[d]), none)   # one robot posed by the joystick ...
        pose(T + 8, zero3, zero3, only(none, 5))                          # ... reset at once to the identity
        pose(T + 11, zero3, zero3, none)
        pose(T + 24, push, -push, none)                # every robot posed
        pose(T + 30, zero3, zero3, all5)
        pose(T + 33, zero3, zero3, none)
        pose(T + 36, only(zero3, push[d]), only(zero3, push[d]), none)   # once more, held to the end: one posed robot among unposed ones
        vel(T + 40, only(lin, 0.0), only(ang, 0.0))    # one robot without a command: STOPPING, then STOPPED, to the end
        s.cuts = (75,)
    elif kind.endswith("tilt_stop") or kind == "flat_stop":
        hit = d if kind == "lone_tilt_stop" else (np.arange(n) if kind == "all_tilt_stop" else np.array([], dtype=int))
        for c in range(T + 2, cycles, 6):              # tip-state messages: contact forces that come and go, for the robots that are to meet ground early
            f = np.zeros((n, L, 3))
            g = rng.normal(0, 0.25, (n, L, 3))
            g[..., 2] += rng.choice([0.0, 0.05, 0.6, 1.5], size=(n, L), p=[0.3, 0.2, 0.2, 0.3])
            f[hit] = g[hit]
            s.at(c, force=f)
        vel(T + 50, 0.0 * lin, 0.0 * ang)              # every robot stops: the stop predicates on tilted and on flat planes
    elif kind == "late_start":
        # one robot gets its command seven cycles after the others: its legs begin their swing and stance periods in other cycles than its wave-mates' do
        inp["lin"], inp["ang"] = only(lin, 0.0), only(ang, 0.0)
        s.inforce.update(lin=inp["lin"].copy(), ang=inp["ang"].copy())
        vel(7, lin, ang)
    elif kind == "cold_restart":
        # every robot but one starts from STOPPED in cycle 0 (updateWalk returns early for all of them: no odometry step), the one follows; every robot stops;
        # and once more every robot but one starts.  The loop is cut while every robot rests: a launch in which no leg begins a swing or a stance period.
        inp["lin"], inp["ang"] = only(lin, 0.0), only(ang, 0.0)
        s.inforce.update(lin=inp["lin"].copy(), ang=inp["ang"].copy())
        vel(3, lin, ang)
        vel(T + 6, 0.0 * lin, 0.0 * ang)
        vel(T + stop_len + 26, only(lin, 0.0), only(ang, 0.0))
        s.cuts = (T + stop_len + 19, T + stop_len + 24)
    else:
        assert kind in ("stop_restart", "stop_restart_posed")
        if kind == "stop_restart_posed":   # one robot posed in each half of the run, which a loop run cuts in two: a launch in which one robot's pose ran
            for c in (5, 80):
                pose(c, only(zero3, push[d]), only(zero3, -push[d]), none)
                pose(c + 3, zero3, zero3, only(none, 5))
                pose(c + 5, zero3, zero3, none)
            s.cuts = (75, 110)   # (two launches in which the one robot that started again is the only one whose legs begin swing / stance periods)
        vel(T, 0.0 * lin, 0.0 * ang)                   # every robot stops: STOPPING together, the defaults re-derived together, STOPPED, at rest
        vel(T + stop_len, only(0.0 * lin, lin[d]), only(0.0 * ang, ang[d]))   # one robot starts again among robots at rest
    assert max(s.events) < cycles
    return p, n, inp, s


def oracle_run(p, n, inp, sched, cycles):
    """The scenario on the oracle alone: fills the schedule's records as a teacher-forced run does."""
    from test_gpu_parity import apply
    ob = OracleBatch(p, n)
    apply(ob, inp)
    for c in range(cycles):
        sched.fire(c, (ob,))
        ob.step(1, 8)
    return ob


def guards_of(name):
    provides, only = MORPHS[name][1], MORPHS[name][4]
    return [g for g in GUARDS if g.needs <= provides and "loop" not in g.needs and (only is None or only in g.needs)]


def tally_run(p, sched, final_record, cycles, guards, features=FEAT_DEFAULT):
    """Classifies every cycle of a run from the records the schedule kept (+ the record after the last cycle)."""
    tables = OracleBatch(p, 1).tables()
    t = Tally()
    for c in range(cycles):
        after = sched.records[c + 1] if c + 1 < cycles else final_record
        x = Ctx(p, tables, features, sched.records[c], after, sched.inputs[c])
        for g in guards:
            for cls in classify(g, x):
                t.add(g.id, cls)
    return t


# ------------------------------------------------------------------------------------------------ memo guards (loop forms)
HIT_AFTER_MISS = "HIT_AFTER_MISS"
LOOP_CYCLES, LOOP_HISTORY = 64, 40


def loop_guards():
    return [g for g in GUARDS if "loop" in g.needs]


def loop_plan(n, L=6, cycles=LOOP_CYCLES):
    """(lin, ang) of every cycle of the loop.  Every robot holds a command of its own; every sixth cycle the designated robot of each wave - first, inner, last
    group in turn, and the last robot of the partial wave - gets a command turned by 50 degrees with another angular part, so that the stride bearings of its
    legs cross 45-degree sector edges (the bracket memo of its wave misses because of one robot) and its desired angular velocity moves for a few cycles (so does
    the odometry cache); in between the memos hit.  Twice every robot turns.  Seed and cycles chosen on the CPU oracle (tests/test_wave_paths_table.py)."""
    rng = np.random.default_rng(64)
    th, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(0.3, 0.6, n)
    ang = rng.uniform(0.05, 0.2, n) * rng.choice([-1.0, 1.0], n)
    out, event = [], 0
    for c in range(cycles):
        if c % 6 == 4:
            who = np.arange(n) if c in (28, 52) else designated(n, L, POSITIONS[event % 3])
            th[who] += np.deg2rad(50.0)
            ang[who] = -ang[who] * 0.9
            event += 1
        out.append((np.stack([r * np.cos(th), r * np.sin(th)], axis=1), ang.copy()))
    return out


def tally_loop(p, records, plan, guards=None, features=FEAT_DEFAULT):
    """records[c]: the state record before cycle c of the loop (records[len(plan)]: after the last).  Memos start empty with the loop."""
    guards = loop_guards() if guards is None else guards
    tables = OracleBatch(p, 1).tables()
    t, memo, last = Tally(), {}, {}
    for c, (lin, ang) in enumerate(plan):
        x = Ctx(p, tables, features, records[c], records[c + 1], {"lin": lin, "ang": ang}, loop_memo=memo)
        for g in guards:
            now = classify(g, x)
            for w, cls in enumerate(now):
                t.add(g.id, cls)
                before = last.get((g.id, w))
                if cls == UNIFORM_TAKEN and before is not None and before not in (UNIFORM_TAKEN, UNDECIDED, NOT_REACHED):
                    t.add(g.id, HIT_AFTER_MISS)
            last.update({(g.id, w): cls for w, cls in enumerate(now)})
    return t


def tally_loop_run(p, sched, final_record, cycles, guards=None, features=FEAT_DEFAULT):
    """A scenario run as a loop (cut at sched.cuts into resident launches, each starting with empty memos), classified from the records the schedule kept."""
    guards = loop_guards() if guards is None else guards
    tables = OracleBatch(p, 1).tables()
    t, last = Tally(), {}
    bounds = [0] + list(sched.cuts) + [cycles]
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        memo, launch_votes = {}, {}
        for c in range(c0, c1):
            after = sched.records[c + 1] if c + 1 < cycles else final_record
            x = Ctx(p, tables, features, sched.records[c], after, sched.inputs[c], loop_memo=memo)
            for g in guards:
                if g.per_launch:
                    v = g.predicate(x)
                    launch_votes[g.id] = v if g.id not in launch_votes else np.where((launch_votes[g.id] == YES) | (v == YES), YES, np.minimum(launch_votes[g.id], v))
                    continue
                now = classify(g, x)
                for w, cls in enumerate(now):
                    t.add(g.id, cls)
                    before = last.get((g.id, w)) if c > c0 else None
                    if cls == UNIFORM_TAKEN and before is not None and before not in (UNIFORM_TAKEN, UNDECIDED, NOT_REACHED):
                        t.add(g.id, HIT_AFTER_MISS)
                last.update({(g.id, w): cls for w, cls in enumerate(now)})
        for g in guards:
            if g.per_launch:
                x.votes_override = launch_votes[g.id]
                for cls in classify(Guard(g.id, g.file, g.function, g.text, g.kind, g.needs, lambda y: y.votes_override), x):
                    t.add(g.id, cls)
    return t


MEMO_GUARDS = ("front.bracket_memo", "odom.cache")


def memo_guards():
    return [g for g in GUARDS if g.id in MEMO_GUARDS]


def loop_missing(t, guards=None):
    guards = loop_guards() if guards is None else guards
    return t.missing(guards) + [(g.id, HIT_AFTER_MISS, t.counts.get(g.id, {}).get(HIT_AFTER_MISS, 0)) for g in guards
                                if g.id in MEMO_GUARDS and t.counts.get(g.id, {}).get(HIT_AFTER_MISS, 0) < K_MIN]
