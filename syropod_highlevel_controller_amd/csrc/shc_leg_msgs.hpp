// shc_leg_msgs.hpp — StateController::publishLegState (state_controller.cpp:809-893) for a range of instances in one device pass:
// shc_engine_get_leg_state_msgs, and for one robot through the same pass: shc_engine_read_leg_state_msg.  Included by shc_engine.hip (uses its
// slot_of / rob_index / derive_tips and entry-point macros).
//
// The derived fields of the payload (swing / stance progress, time_to_swing_end, pose_delta, LegPoser::auto_pose_) are functions of the
// stored state and of a few launch-uniform parameters; LegMsgArgs carries those parameters, and the device functions below are the ONE
// implementation of that arithmetic - leg_state_msgs_kernel and the observation rows (shc_observe.hpp) call them; nothing is recomputed on the host.
#pragma once

#include <cstddef>

// Launch-uniform inputs of the derived LegState fields: a kernel argument of leg_state_msgs_kernel and observe_kernel.
struct LegMsgArgs {
  double swing_time, stance_time; // (swing / stance period / period) / frequency (state_controller.cpp:863-864)
  double force_gain;
  int32_t period, swing_start, swing_end, stance_start, stance_end;
  int32_t admittance_control;
  int32_t auto_live;         // auto posing runs (only where IMU posing does not, pose_controller.cpp:836-846)
  int32_t pose_clock_ahead;  // the pose phase counter has advanced past the cycle the poses belong to (pose_frequency != -1)
  int32_t pose_phase_length, n_auto_posers;
  int32_t ap_start[kMaxAutoPosers], ap_end[kMaxAutoPosers]; // pose phase starts / ends * normaliser
  double ap_amp[kMaxAutoPosers][7];                          // x y z gravity roll pitch yaw
  int32_t neg_start[SHC_MAX_LEGS], neg_end[SHC_MAX_LEGS];    // pose negation phase starts / ends * normaliser
  double neg_ratio[SHC_MAX_LEGS];
};

static LegMsgArgs leg_msg_args(const shc_params &p, const shc_tables &t) {
  LegMsgArgs a;
  memset(&a, 0, sizeof a);
  const shc_step_cycle &step = t.step;
  a.swing_time = (double(step.swing_period) / step.period) / step.frequency;
  a.stance_time = (double(step.stance_period) / step.period) / step.frequency;
  a.force_gain = p.force_gain;
  a.period = step.period, a.swing_start = step.swing_start, a.swing_end = step.swing_end;
  a.stance_start = step.stance_start, a.stance_end = step.stance_end;
  a.admittance_control = p.admittance_control;
  a.auto_live = p.auto_posing && !p.imu_posing && t.pose_phase_length > 0;
  a.pose_clock_ahead = p.pose_frequency != -1.0;
  a.pose_phase_length = t.pose_phase_length;
  a.n_auto_posers = p.n_auto_posers < kMaxAutoPosers ? p.n_auto_posers : kMaxAutoPosers;
  const int nrm = t.pose_normaliser;
  for (int i = 0; i < a.n_auto_posers; ++i) {
    a.ap_start[i] = p.pose_phase_starts[i] * nrm, a.ap_end[i] = p.pose_phase_ends[i] * nrm;
    const double amp[7] = {p.x_amplitudes[i],    p.y_amplitudes[i],     p.z_amplitudes[i],  p.gravity_amplitudes[i],
                           p.roll_amplitudes[i], p.pitch_amplitudes[i], p.yaw_amplitudes[i]};
    for (int k = 0; k < 7; ++k) a.ap_amp[i][k] = amp[k];
  }
  for (int l = 0; l < SHC_MAX_LEGS; ++l) {
    a.neg_start[l] = p.pose_negation_phase_starts[l] * nrm, a.neg_end[l] = p.pose_negation_phase_ends[l] * nrm;
    a.neg_ratio[l] = p.negation_transition_ratio[l];
  }
  return a;
}

// The master phase of the cycle the stored poser latches belong to
__device__ __forceinline__ int leg_msg_master_phase(const LegMsgArgs &a, int pose_phase) {
  return (a.auto_live && a.pose_clock_ahead) ? mod_i(pose_phase - 1, a.pose_phase_length) : pose_phase;
}

// PoseController::auto_pose_ of the cycle whose master phase and (post-update) poser latches are given: the sum the cycle
// kernel forms (AutoPoser::updatePose, pose_controller.cpp:1338-1439), re-derived for LegState.auto_pose.
__device__ __forceinline__ Pose leg_msg_auto_pose(const LegMsgArgs &a, int master_phase, int flags, Quat imu) {
  Pose auto_pose = pose_identity();
  const int len = a.pose_phase_length;
  for (int i = 0; i < a.n_auto_posers; ++i) {
    const bool allow = ((flags >> (4 * i)) & 8) != 0;
    int phase = master_phase, sp = a.ap_start[i], ep = a.ap_end[i];
    if (sp > ep) {
      ep += len;
      if (phase < sp) phase += len;
    }
    if (!(phase >= sp && phase < ep && allow)) continue;
    const int iteration = phase - sp + 1, num = ep - sp;
    const bool first_half = iteration <= num / 2;
    const double delta_t = 1.0 / (num / 2.0);
    const int offset = int(first_half ? 0 : num / 2.0);
    const double tt = (iteration - offset) * delta_t, u = 1.0 - tt;
    const double wgt = first_half ? (4.0 * tt * tt * tt * u + tt * tt * tt * tt) : (u * u * u * u + 4.0 * tt * u * u * u);
    V3 pos;
    if (a.ap_amp[i][3] != 0.0) { // Model::estimateGravity (model.cpp:156-165)
      const V3 e = quat_to_euler(imu, false);
      V3 gv{0, 0, kGravity};
      gv = rotate(angle_axis_y(-e.y), gv);
      gv = rotate(angle_axis_x(-e.x), gv);
      pos = normalized(gv) * (a.ap_amp[i][3] * wgt);
    } else {
      pos = V3{a.ap_amp[i][0] * wgt, a.ap_amp[i][1] * wgt, a.ap_amp[i][2] * wgt};
    }
    const V3 rot{a.ap_amp[i][4] * wgt, a.ap_amp[i][5] * wgt, a.ap_amp[i][6] * wgt};
    auto_pose = add_pose(auto_pose, Pose{pos, euler_to_quat(rot, false)});
  }
  return auto_pose;
}
// LegPoser::updateAutoPose's negation (pose_controller.cpp:1740-1776) for a leg whose negate flag is set
__device__ __forceinline__ Pose leg_msg_leg_auto_pose(const LegMsgArgs &a, int leg, int master_phase, bool negate, const Pose &auto_pose) {
  if (!negate) return auto_pose;
  const int len = a.pose_phase_length;
  int sp = a.neg_start[leg], ep = a.neg_end[leg], np = master_phase;
  if (sp == 0) sp = len;
  if (ep == 0) ep = len;
  if (sp > ep) {
    ep += len;
    if (np < sp) np += len;
  }
  const int iteration = np - sp + 1, num = ep - sp;
  const bool first_half = iteration <= num / 2;
  double ci = 1.0;
  const double ratio = a.neg_ratio[leg];
  if (ratio > 0.0) ci = first_half ? fmin(1.0, iteration / (num * ratio)) : fmin(1.0, (num - iteration) / (num * ratio));
  ci = smooth_step(ci);
  return remove_pose(auto_pose, interpolate_pose(pose_identity(), ci, auto_pose));
}

// LegStepper::swing_progress_ / stance_progress_ as iteratePhase left them (walk_controller.cpp:871-897): a function of the leg word's progress
// mode, the phase and the step cycle the phase counts in.  The ONE place this arithmetic is written: leg_msg_progress and the state records
// (shc_snapshot.hpp) call it, each with the step cycle it holds (Cycle: LegMsgArgs or CycleParams - the members read here carry the same names).
template <class Cycle>
SHC_HD void step_progress(const Cycle &c, int pm, int phase, double &swing, double &stance) {
  swing = stance = -1.0; // walk_controller.h:498-499
  if (pm == PM_SWING) {
    swing = clampd(double(phase - c.swing_start + 1) / double(c.swing_end - c.swing_start), 0.0, 1.0);
  } else if (pm == PM_STANCE) {
    stance = clampd(double(mod_i(phase + (c.period - c.stance_start), c.period) + 1) / double(mod_i(c.stance_end - c.stance_start, c.period)), 0.0, 1.0);
  } else if (pm == PM_STOP) {
    stance = 0.0;
  }
}

// ... and from them time_to_swing_end (state_controller.cpp:866-873) and WalkController::calculateOdometry(time_to_swing_end)
// (walk_controller.cpp:783-791), from the leg word and the desired velocity.  pose_delta: x, y, z, qw, qx, qy, qz.
struct LegMsgProgress {
  double stance_progress, swing_progress, time_to_swing_end, pose_delta[7];
};
__device__ __forceinline__ LegMsgProgress leg_msg_progress(const LegMsgArgs &a, int word, double vx, double vy, double vw) {
  LegMsgProgress r;
  step_progress(a, (word >> LW_PM_SHIFT) & 3, (word >> LW_PHASE_SHIFT) & LW_PHASE_MASK, r.swing_progress, r.stance_progress);
  r.time_to_swing_end = r.stance_progress >= 0.0 ? a.stance_time * (1.0 - r.stance_progress) + a.swing_time : a.swing_time * (1.0 - r.swing_progress);
  const double t = r.time_to_swing_end;
  r.pose_delta[0] = vx * t;
  r.pose_delta[1] = vy * t;
  r.pose_delta[2] = 0.0 * t;
  r.pose_delta[3] = cos(0.5 * (vw * t));
  r.pose_delta[4] = 0.0;
  r.pose_delta[5] = 0.0;
  r.pose_delta[6] = sin(0.5 * (vw * t));
  return r;
}

// LegState.tip_force: tip_force_calculated_ * force_gain (state_controller.cpp:883-885)
__device__ __forceinline__ double leg_msg_tip_force(const LegMsgArgs &a, double calculated) { return calculated * a.force_gain; }

// ---- the batched form
// Record layout in doubles (shc_leg_state_msg is 64 doubles, no padding: the kernel builds a record as double rec[64])
struct LegMsgAt {
#define SHC_MSG_AT(NAME) int(offsetof(shc_leg_state_msg, NAME) / 8)
  static constexpr int WALKER = SHC_MSG_AT(walker_tip_position), TARGET = SHC_MSG_AT(target_tip_position), POSER = SHC_MSG_AT(poser_tip_position),
                       MODEL = SHC_MSG_AT(model_tip_position), ACTUAL = SHC_MSG_AT(actual_tip_pose), JPOS = SHC_MSG_AT(joint_positions),
                       JVEL = SHC_MSG_AT(joint_velocities), JEFF = SHC_MSG_AT(joint_efforts), STANCE = SHC_MSG_AT(stance_progress),
                       SWING = SHC_MSG_AT(swing_progress), TTSE = SHC_MSG_AT(time_to_swing_end), PDELTA = SHC_MSG_AT(pose_delta),
                       AUTO = SHC_MSG_AT(auto_pose), FORCE = SHC_MSG_AT(tip_force), ADM = SHC_MSG_AT(admittance_delta),
                       STIFF = SHC_MSG_AT(virtual_stiffness);
#undef SHC_MSG_AT
};
constexpr int kMsgDoubles = 64;
static_assert(sizeof(shc_leg_state_msg) == kMsgDoubles * 8, "shc_leg_state_msg is 64 doubles without padding");
// A lane's record goes through LDS in two halves of 32 doubles.  A lane's strip is 34 doubles (272 B): 272 / 4 = 68 = 4 mod 32 banks, so
// the eight lanes a ds_write_b128 serves per LDS cycle start 4 banks apart and cover all 32 banks once - no conflict; the read side takes
// 16 consecutive lanes from one strip (256 contiguous bytes), conflict-free by construction.  17 KiB per wavefront: 9 wavefronts per CU.
constexpr int kMsgHalf = kMsgDoubles / 2, kMsgStrip = kMsgHalf + 2;

// Fields [F0, F0 + K) of one leg slot, read as whole 16-byte planes (two fields each)
template <int F0, int K>
__device__ __forceinline__ void load_leg_fields(const double2 *__restrict__ planes, int64_t n_slots, int64_t slot, double (&o)[K]) {
  constexpr int p0 = F0 >> 1, p1 = (F0 + K - 1) >> 1;
#pragma unroll
  for (int p = p0; p <= p1; ++p) {
    const double2 v = planes[int64_t(p) * n_slots + slot];
    if (2 * p >= F0 && 2 * p < F0 + K) o[2 * p - F0] = v.x;
    if (2 * p + 1 >= F0 && 2 * p + 1 < F0 + K) o[2 * p + 1 - F0] = v.y;
  }
}

// The geometry of shc_rows.hpp (RowGroup) for [first, first + count).  The records of a
// wavefront are consecutive in `out` (consecutive instances, consecutive legs), so after staging the block is written with all 64 lanes,
// 16 B per lane, contiguous within each 256-byte half record.  MODEL_TIP / POSER_TIP must have been derived (derive_tips).
template <int L, int NJ>
__global__ __launch_bounds__(64) void leg_state_msgs_kernel(double2 *__restrict__ out, DevState st, const SharedConsts<L, NJ> *__restrict__ gc,
                                                            const LegMsgArgs a, int64_t first, int64_t count) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  using At = LegMsgAt;
  constexpr int rpw = 64 / L;
  __shared__ double2 strip[64 * kMsgStrip / 2];
  const RowGroup<L> rg(first, first + count);
  const int lane = rg.lane, leg = rg.leg;
  const int64_t rob = rg.rob;
  // lanes [lane0, lane0 + n_rec) hold the records out[rec0 ..] of this block
  const int lane0 = rg.g0 * L, n_rec = rg.n_rob * L;
  const int64_t rec0 = (rg.rob_lo - first) * L;

  double rec[kMsgDoubles];
#pragma unroll
  for (int k = 0; k < kMsgDoubles; ++k) rec[k] = 0.0;
  if (rg.live) {
    const double2 *planes = reinterpret_cast<const double2 *>(st.legd);
    const int64_t slot = rg.slot;
    const int word = st.legi[slot];
    {
      double v[2 * NJ + 3]; // Q, QD, TIP are consecutive fields
      load_leg_fields<FD::Q, 2 * NJ + 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int j = 0; j < NJ; ++j) rec[At::JPOS + j] = v[j], rec[At::JVEL + j] = v[NJ + j];
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::WALKER + k] = v[2 * NJ + k];
    }
    {
      double v[3];
      load_leg_fields<FD::TARG, 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::TARGET + k] = v[k];
      load_leg_fields<FD::POSER_TIP, 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::POSER + k] = v[k];
      load_leg_fields<FD::MODEL_TIP, 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::MODEL + k] = v[k];
      load_leg_fields<FD::TF, 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::FORCE + k] = leg_msg_tip_force(a, v[k]);
    }
    if (a.admittance_control) {
      double v[4];
      load_leg_fields<FD::ADM_DELTA, 4>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) rec[At::ADM + k] = v[k];
      rec[At::STIFF] = v[3];
    }
    {
      double v[NJ];
      load_leg_fields<FD::EFFORT_IN, NJ>(planes, st.n_slots, slot, v); // desired_effort_ = current_effort_ (state_controller.cpp:1590)
#pragma unroll
      for (int j = 0; j < NJ; ++j) rec[At::JEFF + j] = v[j];
    }
    { // actual_tip_pose: Leg::applyFK(false, true) on the measured joint positions (:839)
      double qm[NJ];
      load_leg_fields<FD::MEAS_Q, NJ>(planes, st.n_slots, slot, qm);
      const Pose tp = fk_tip_pose<NJ>(gc->leg[leg], qm);
      rec[At::ACTUAL + 0] = tp.p.x, rec[At::ACTUAL + 1] = tp.p.y, rec[At::ACTUAL + 2] = tp.p.z;
      rec[At::ACTUAL + 3] = tp.r.w, rec[At::ACTUAL + 4] = tp.r.x, rec[At::ACTUAL + 5] = tp.r.y, rec[At::ACTUAL + 6] = tp.r.z;
    }
    // robot-level inputs: every lane of a robot's group reads the same words of the wavefront's robot tile
    const double vx = st.robd[rob_index(rob, R::VLIN, rpw, R::COUNT)], vy = st.robd[rob_index(rob, R::VLIN + 1, rpw, R::COUNT)];
    const double vw = st.robd[rob_index(rob, R::VANG, rpw, R::COUNT)];
    const LegMsgProgress pr = leg_msg_progress(a, word, vx, vy, vw);
    rec[At::STANCE] = pr.stance_progress, rec[At::SWING] = pr.swing_progress, rec[At::TTSE] = pr.time_to_swing_end;
#pragma unroll
    for (int k = 0; k < 7; ++k) rec[At::PDELTA + k] = pr.pose_delta[k];
    // LegPoser::auto_pose_ (:877-880).  The robot-level sum is formed by every lane of the group for itself: the lanes run the same
    // instructions whether one of them or all need the result, and sharing it would add seven cross-lane moves.
    Pose la = pose_identity();
    if (a.auto_live) {
      const int latches = st.robi[rob_index(rob, R::I_APOSER, rpw, R::I_COUNT)];
      const int master_phase = leg_msg_master_phase(a, st.robi[rob_index(rob, R::I_POSE_PHASE, rpw, R::I_COUNT)]);
      const Quat imu{st.robd[rob_index(rob, R::IMUQ, rpw, R::COUNT)], st.robd[rob_index(rob, R::IMUQ + 1, rpw, R::COUNT)],
                     st.robd[rob_index(rob, R::IMUQ + 2, rpw, R::COUNT)], st.robd[rob_index(rob, R::IMUQ + 3, rpw, R::COUNT)]};
      la = leg_msg_leg_auto_pose(a, leg, master_phase, (word & LW_NEG) != 0, leg_msg_auto_pose(a, master_phase, latches, imu));
    }
    rec[At::AUTO + 0] = la.p.x, rec[At::AUTO + 1] = la.p.y, rec[At::AUTO + 2] = la.p.z;
    rec[At::AUTO + 3] = la.r.w, rec[At::AUTO + 4] = la.r.x, rec[At::AUTO + 5] = la.r.y, rec[At::AUTO + 6] = la.r.z;
  }

  constexpr int kChunks = kMsgHalf / 2; // 16-byte chunks of a half record
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads(); // the first half has been read out of the strips
#pragma unroll
    for (int k = 0; k < kChunks; ++k) strip[lane * (kMsgStrip / 2) + k] = double2{rec[h * kMsgHalf + 2 * k], rec[h * kMsgHalf + 2 * k + 1]};
    __syncthreads();
    for (int c = lane; c < n_rec * kChunks; c += 64) {
      const int r = c / kChunks, k = c - r * kChunks;
      out[(rec0 + r) * (kMsgDoubles / 2) + h * kChunks + k] = strip[(lane0 + r) * (kMsgStrip / 2) + k];
    }
  }
}

extern "C" int shc_engine_get_leg_state_msgs(shc_engine *e, int64_t first, int64_t count, shc_leg_state_msg *msgs, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!msgs) return fail(SHC_ERR_INVALID_ARG, "msgs is NULL");
  if (first < 0 || count < 0 || first + count > e->n) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if (on_device && (reinterpret_cast<uintptr_t>(msgs) & 15)) return fail(SHC_ERR_INVALID_ARG, "a device msgs buffer must be 16-byte aligned");
  if (count == 0) return SHC_OK;
  int rc = derive_tips(e);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  shc_leg_state_msg *d = hc.out(msgs, size_t(count) * e->L, on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  const LegMsgArgs args = leg_msg_args(e->params, e->tables);
  const unsigned grid = row_grid(e->L, first, first + count);
  rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    leg_state_msgs_kernel<L, NJ><<<dim3(grid), dim3(64), 0, e->stream>>>(reinterpret_cast<double2 *>(d), e->st, (const SharedConsts<L, NJ> *)e->d_consts, args, first, count);
    return SHC_OK;
  });
  return rc != SHC_OK ? rc : hc.finish();
}
// One robot's records: the pass above for [instance, instance + 1), so the bytes of the batched call
extern "C" int shc_engine_read_leg_state_msg(shc_engine *e, int64_t instance, shc_leg_state_msg *legs) {
  SHC_ENTER_JOINED(e);
  if (!legs) return fail(SHC_ERR_INVALID_ARG, "legs is NULL");
  if (instance < 0 || instance >= e->n) return fail(SHC_ERR_INVALID_ARG, "instance out of range");
  return shc_engine_get_leg_state_msgs(e, instance, 1, legs, 0);
}
