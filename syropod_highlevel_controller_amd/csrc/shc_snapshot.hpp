// shc_snapshot.hpp — shc_engine_get_state / shc_engine_set_state: the engine's SoA planes <-> shc_instance_state records
// (include/shc_batch.h), and the auxiliary state blobs.  Checkpoint / restore and state injection; not on the per-cycle path.
//
// The record speaks the reference's member names (LegStepper / LegPoser / WalkController / PoseController members, cited in
// the header); the engine's packed words and direction vectors are converted here, by ONE walk over the record that both
// directions are instances of (state_kernel<NJ, TO_ENGINE>) - a member added to the walk is read and injected alike:
//   * swing_progress_ / stance_progress_  <->  the 2-bit "progress mode" + the phase (walk_controller.cpp:871-897 writes
//     them from the phase alone, so the pair is a function of (mode, phase): step_progress of shc_leg_msgs.hpp, which the
//     LegState payload calls too);
//   * the stepping legs' copies of the walk plane (LegStepper::walk_plane_) are one per robot in the engine.
#pragma once

#include "shc_cycle.hpp"

namespace shc {

// ---- the members that are not straight copies of plane fields: a pack (record -> engine) and an unpack (engine -> record) each

// the robot word
__device__ __forceinline__ int snap_pack_robot_word(const shc_instance_state &o) {
  return (o.walk_state & 3) | ((o.legs_at_correct_phase & 15) << RW_LACP_SHIFT) | ((o.legs_completed_first_step & 15) << RW_LCFS_SHIFT) |
         (o.return_to_default_attempted ? RW_RTDA : 0) | ((o.auto_posing_state & 3) << RW_APS_SHIFT);
}
__device__ __forceinline__ void snap_unpack_robot_word(int w, shc_instance_state &o) {
  o.walk_state = w & 3;
  o.legs_at_correct_phase = (w >> RW_LACP_SHIFT) & 15;
  o.legs_completed_first_step = (w >> RW_LCFS_SHIFT) & 15;
  o.return_to_default_attempted = (w & RW_RTDA) ? 1 : 0;
  o.auto_posing_state = (w >> RW_APS_SHIFT) & 3;
}
// odometry_ideal_ is stored as (x, y, qw, qz), pure yaw: the pack ignores slots 2, 4 and 5 of the 7-double pose, the unpack writes zeros there
__device__ __forceinline__ void snap_pack_odometry(const double (&pose)[7], double (&s)[4]) { s[0] = pose[0], s[1] = pose[1], s[2] = pose[3], s[3] = pose[6]; }
__device__ __forceinline__ void snap_unpack_odometry(const double (&s)[4], double (&pose)[7]) {
  pose[0] = s[0], pose[1] = s[1], pose[2] = 0.0, pose[3] = s[2], pose[4] = 0.0, pose[5] = 0.0, pose[6] = s[3];
}
// the leg word; pm: its progress mode (below).  The pack builds the whole word.  rotations: this leg's tip rotations are tracked - only then
// do the two rotation bits travel, in either direction
__device__ __forceinline__ int snap_pack_leg_word(const shc_leg_snapshot &g, int pm, bool rotations) {
  return (g.step_state & 3) | (g.at_correct_phase ? LW_ACP : 0) | (g.completed_first_step ? LW_CFS : 0) | (pm << LW_PM_SHIFT) |
         (g.negate_auto_pose ? LW_NEG : 0) | (g.ik_failed ? LW_IKFAIL : 0) | ((g.phase & LW_PHASE_MASK) << LW_PHASE_SHIFT) |
         (rotations && g.tip_rotation_defined ? LW_ROTDEF : 0) | (rotations && g.target_rotation_defined ? LW_TARGROT : 0);
}
__device__ __forceinline__ void snap_unpack_leg_word(int w, shc_leg_snapshot &g, bool rotations) {
  g.step_state = w & 3;
  g.phase = (w >> LW_PHASE_SHIFT) & LW_PHASE_MASK;
  g.at_correct_phase = (w & LW_ACP) ? 1 : 0;
  g.completed_first_step = (w & LW_CFS) ? 1 : 0;
  g.negate_auto_pose = (w & LW_NEG) ? 1 : 0;
  g.ik_failed = (w & LW_IKFAIL) ? 1 : 0;
  if (rotations) {
    g.tip_rotation_defined = (w & LW_ROTDEF) ? 1 : 0;
    g.target_rotation_defined = (w & LW_TARGROT) ? 1 : 0;
  }
}
// the progress mode of (swing_progress, stance_progress); its unpack is step_progress (shc_leg_msgs.hpp: LegStepper::iteratePhase)
__device__ __forceinline__ int snap_pack_progress_mode(double swing, double stance) {
  return swing >= 0.0 ? PM_SWING : stance > 0.0 ? PM_STANCE : stance == 0.0 ? PM_STOP : PM_NONE;
}
// the step plane (x, y, z, defined flag).  The pack writes position-or-zeros and the flag 1.0 / 0.0 whatever rough_terrain says; the unpack
// calls the plane defined only in rough terrain mode with a non-zero flag, and copies the position only then
__device__ __forceinline__ void snap_pack_step_plane(const shc_leg_snapshot &g, double (&s)[4]) {
  for (int k = 0; k < 3; ++k) s[k] = g.step_plane_defined ? g.step_plane_position[k] : 0.0;
  s[3] = g.step_plane_defined ? 1.0 : 0.0;
}
__device__ __forceinline__ void snap_unpack_step_plane(const double (&s)[4], bool rough_terrain, shc_leg_snapshot &g) {
  g.step_plane_defined = (rough_terrain && s[3] != 0.0) ? 1 : 0;
  if (g.step_plane_defined)
    for (int k = 0; k < 3; ++k) g.step_plane_position[k] = s[k];
}

// ---- the one walk over a record: every (record member, plane field) pair is named once; TO_ENGINE picks the direction (set_state : get_state).
// touchdown: RT_TOUCHDOWN, for the records read (the host side of state_transfer raises it from the records injected).
// long_legs: bit l = leg l has more than 3 joints (its stepper tracks a tip rotation under gravity_aligned_tips / rough terrain mode; a shorter
// leg of the same robot, padded up to the kernel's joint count, does not: its record fields stay zero, as for a robot of 3-joint legs, and an
// injected record leaves its direction planes alone, so that get_state -> set_state is the identity on every leg).
template <int NJ, bool TO_ENGINE>
__global__ void state_kernel(shc_instance_state *recs, DevState st, CycleParams P, int L, int64_t first, int64_t count, int touchdown, unsigned long_legs) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int64_t rob = first + t;
  const int rpw = 64 / L;
  shc_instance_state &o = recs[t];
  auto move = [](auto &plane, auto &member) {
    if constexpr (TO_ENGINE) plane = member;
    else member = plane;
  };
  auto rd = [&](int f) -> double & { return st.robd[rob_index(rob, f, rpw, R::COUNT)]; };
  auto ri = [&](int f) -> int32_t & { return st.robi[rob_index(rob, f, rpw, R::I_COUNT)]; };
  auto robot = [&](int f0, double *member, int n) { // n consecutive robot fields from f0
    for (int k = 0; k < n; ++k) move(rd(f0 + k), member[k]);
  };
  robot(R::VLIN, o.desired_linear_velocity, 2);
  robot(R::VANG, &o.desired_angular_velocity, 1);
  robot(R::PLANE, o.walk_plane, 3);
  robot(R::PNORM, o.walk_plane_normal, 3);
  robot(R::PLANE_PREV, o.stepper_walk_plane, 3);
  robot(R::PNORM_PREV, o.stepper_walk_plane_normal, 3);
  robot(R::TVI, o.translation_velocity_input, 3);
  robot(R::RVI, o.rotation_velocity_input, 3);
  robot(R::ABSE, o.rotation_absement_error, 3);
  robot(R::VERR, o.rotation_velocity_error, 3);
  robot(R::OWPP, o.origin_walk_plane_pose, 7);
  robot(R::MPOSE, o.manual_pose, 7);
  robot(R::CPOSE, o.current_pose, 7);
  robot(R::TALIGN, o.tip_align_pose, 7);
  robot(R::OTALIGN, o.origin_tip_align_pose, 7);
  robot(R::APREV, o.auto_pose_rotation, 4);
  move(ri(R::I_POSE_PHASE), o.pose_phase);
  {
    double s[4];
    if constexpr (TO_ENGINE) snap_pack_odometry(o.odometry, s);
    robot(R::ODOM, s, 4);
    if constexpr (!TO_ENGINE) snap_unpack_odometry(s, o.odometry);
  }
  if constexpr (TO_ENGINE) ri(R::I_WORD) = snap_pack_robot_word(o);
  else snap_unpack_robot_word(ri(R::I_WORD), o);
  int latches = TO_ENGINE ? 0 : ri(R::I_APOSER); // the poser-latch word: four bits per poser
  for (int i = 0; i < SHC_MAX_AUTO_POSERS; ++i) {
    if constexpr (TO_ENGINE) latches |= (o.auto_poser_flags[i] & 15) << (4 * i);
    else o.auto_poser_flags[i] = (latches >> (4 * i)) & 15;
  }
  if constexpr (TO_ENGINE) ri(R::I_APOSER) = latches;
  if constexpr (!TO_ENGINE) o.touchdown_detection = touchdown, o.pad_ = 0; // read only: injected, the host side has looked at touchdown_detection
  for (int l = 0; l < SHC_MAX_LEGS; ++l) {
    shc_leg_snapshot &g = o.leg[l];
    if constexpr (!TO_ENGINE) __builtin_memset(&g, 0, sizeof g); // read: what the walk does not write is zero ...
    if (l >= L) continue;                                        // ... the legs the robot lacks whole; injected, they are skipped
    const int64_t slot = slot_of(rob, l, L);
    auto leg = [&](int f0, double *member, int n) { // n consecutive leg fields from f0
      for (int k = 0; k < n; ++k) move(st.legd[leg_field_index(f0 + k, slot, st.n_slots)], member[k]);
    };
    leg(FD::Q, g.joint_position, NJ);
    leg(FD::QD, g.joint_velocity, NJ);
    leg(FD::TIP, g.walker_tip, 3);
    leg(FD::TVEL, g.walker_tip_velocity, 3);
    leg(FD::SORG, g.swing_origin_tip, 3);
    leg(FD::SVEL, g.swing_origin_tip_velocity, 3);
    leg(FD::TORG, g.stance_origin_tip, 3);
    leg(FD::DFLT, g.default_tip, 3);
    leg(FD::TARG, g.target_tip, 3);
    leg(FD::STRD, g.stride_vector, 3);
    leg(FD::ADM_DELTA, g.admittance_delta, 3);
    leg(FD::ADM_DELTA + 3, &g.virtual_stiffness, 1);
    leg(FD::TF, g.tip_force_calculated, 3);
    leg(FD::ADM, g.admittance_state, 2);
    {
      double s[4];
      if constexpr (TO_ENGINE) snap_pack_step_plane(g, s);
      leg(FD::STEP_PLANE, s, 4);
      if constexpr (!TO_ENGINE) snap_unpack_step_plane(s, P.rough_terrain, g);
    }
    // tip rotations tracked (joint_control: a MANUAL 3-joint leg holds its FK tip rotation)
    const bool rotations = (P.gravity_aligned && ((long_legs >> l) & 1u)) || P.joint_control == 2;
    int32_t &w = st.legi[slot];
    if constexpr (TO_ENGINE) {
      w = snap_pack_leg_word(g, snap_pack_progress_mode(g.swing_progress, g.stance_progress), rotations);
    } else {
      snap_unpack_leg_word(w, g, rotations);
      step_progress(P, (w >> LW_PM_SHIFT) & 3, g.phase, g.swing_progress, g.stance_progress); // (P: the step cycle the phase counts in)
    }
    if (rotations) { // an untracked leg's direction planes are never touched
      leg(FD::ORG_DIR, g.origin_tip_direction, 3);
      leg(FD::CUR_DIR, g.walker_tip_direction, 3);
      if (TO_ENGINE || (w & LW_TARGROT)) leg(FD::TARG_DIR, g.target_tip_direction, 3); // read only while the target rotation is defined, written always
    }
  }
}

} // namespace shc

// ---- host side (included by shc_engine.hip below the engine's helpers)
extern "C" int64_t shc_sizeof_instance_state(void) { return (int64_t)sizeof(shc_instance_state); }

// Snapshot records travel through a temporary device buffer (checkpoint / injection are not per-cycle operations).
// Neither direction consumes an adjustParameter that waits for its loop: a record shows the legs' phases in the period they still count in (as the
// reference's state between the two loops), an injected record's phases are mapped onto the new period inside the accepting loop.
static int state_transfer(shc_engine *e, int64_t first, int64_t count, shc_instance_state *out, const shc_instance_state *in) {
  if (first < 0 || count < 0 || first + count > e->n) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if (count == 0) return SHC_OK;
  if (in) e->rt_flags |= RT_MANUAL_LIVE; // an injected state may carry any manual pose
  if (in) // touchdown detection is one flag per engine: on as soon as any injected record has it (tip-state messages arrive for a whole robot)
    for (int64_t i = 0; i < count; ++i)
      if (in[i].touchdown_detection) e->rt_flags |= RT_TOUCHDOWN;
  if (in && !(e->rt_flags & RT_EFFORT_LIVE)) { // a non-zero tip-force filter state decays over the following cycles: evaluate it
    bool any = false;
    for (int64_t i = 0; i < count && !any; ++i)
      for (int l = 0; l < e->L; ++l)
        for (int k = 0; k < 3; ++k) any |= in[i].leg[l].tip_force_calculated[k] != 0.0;
    if (any) {
      const int rc = effort_live(e);
      if (rc != SHC_OK) return rc;
    }
  }
  const int touchdown = (e->rt_flags & RT_TOUCHDOWN) ? 1 : 0;
  CycleParams cp = e->cp; // (a record read derives swing / stance progress from the phase: in the step cycle the phase counts in)
  set_step_cycle(cp, phase_step_cycle(e));
  unsigned long_legs = 0;
  for (int l = 0; l < e->L; ++l) long_legs |= e->params.leg_dof[l] > 3 ? 1u << l : 0u;
  HIP_TRY(hipSetDevice(e->device));
  HostCall hc(e);
  shc_instance_state *d = in ? const_cast<shc_instance_state *>(hc.in(in, size_t(count), 0)) : hc.out(out, size_t(count), 0); // (in: the staged copy)
  if (const int rc = hc.status()) return rc;
  const dim3 grid((unsigned)((count + 63) / 64)), block(64);
  dispatch_nj(e->NJ, [&](auto nj) {
    constexpr int NJ_ = decltype(nj)::value;
    if (in) state_kernel<NJ_, true><<<grid, block, 0, e->stream>>>(d, e->st, cp, e->L, first, count, touchdown, long_legs);
    else state_kernel<NJ_, false><<<grid, block, 0, e->stream>>>(d, e->st, cp, e->L, first, count, touchdown, long_legs);
  });
  return hc.finish();
}
extern "C" int shc_engine_get_state(shc_engine *e, int64_t first, int64_t count, shc_instance_state *states) {
  SHC_ENTER_JOINED(e);
  if (!states) return fail(SHC_ERR_INVALID_ARG, "states is NULL");
  return state_transfer(e, first, count, states, nullptr);
}
extern "C" int shc_engine_set_state(shc_engine *e, int64_t first, int64_t count, const shc_instance_state *states) {
  SHC_ENTER_JOINED(e);
  if (!states) return fail(SHC_ERR_INVALID_ARG, "states is NULL");
  return state_transfer(e, first, count, nullptr, states);
}

// ---- auxiliary state: what only the calls AROUND the control cycle keep (shc_instance_state covers the cycle itself)
struct AuxHeader {
  uint32_t magic;   // 'SHCA'
  uint16_t version; // layout version of this blob
  uint8_t legs, dof;
  uint32_t flags;   // 1: manual-leg record live, 2: external target records live, 4: sequence / planner record live,
                    // 8: the LegPoser tips are state (plan calls under time-dependent posing since the last control cycle)
  int32_t reset_mode; // PoseController::pose_reset_mode_ (RobotFields::I_RESET_MODE: written by the toggle kernel, read by the cycle)
};
constexpr uint32_t kAuxMagic = 0x41434853u;
constexpr uint16_t kAuxVersion = 2; // 2: + the LegPoser tip positions (POSER_TIP) and flag 8
static size_t aux_leg_doubles(int NJ) { // per leg: ExtFields record + leg fields [DES_TIP, COUNT) + the LegPoser tip position
  const int tail = dispatch_nj(NJ, [](auto nj) { return Fields<decltype(nj)::value>::COUNT - Fields<decltype(nj)::value>::DES_TIP; });
  return size_t(ExtFields::COUNT) + size_t(tail) + 3;
}
static size_t aux_bytes(const shc_engine *e) {
  return sizeof(AuxHeader) + sizeof(ManualRobot) + sizeof(SeqRobotState) + size_t(e->L) * aux_leg_doubles(e->NJ) * 8;
}
__global__ void aux_state_kernel(unsigned char *blobs, size_t stride, DevState st, SeqRobotState *seq, int L, int NJ, int des_tip_field, int n_leg_fields, int64_t first,
                                 int64_t count, int to_engine, uint32_t live_flags, int poser_tip_field) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const int64_t rob = first + t;
  unsigned char *b = blobs + size_t(t) * stride;
  AuxHeader *h = reinterpret_cast<AuxHeader *>(b);
  ManualRobot *m = reinterpret_cast<ManualRobot *>(b + sizeof(AuxHeader));
  SeqRobotState *q = reinterpret_cast<SeqRobotState *>(b + sizeof(AuxHeader) + sizeof(ManualRobot));
  double *legs = reinterpret_cast<double *>(b + sizeof(AuxHeader) + sizeof(ManualRobot) + sizeof(SeqRobotState));
  const int tail = n_leg_fields - des_tip_field;
  const int per_leg = ExtFields::COUNT + tail + 3;
  int32_t &reset_mode = st.robi[rob_index(rob, RobotFields::I_RESET_MODE, 64 / L, RobotFields::I_COUNT)];
  if (!to_engine) {
    h->magic = kAuxMagic, h->version = kAuxVersion, h->legs = uint8_t(L), h->dof = uint8_t(NJ), h->flags = live_flags, h->reset_mode = reset_mode;
    if (st.manual) *m = st.manual[rob];
    else memset(m, 0, sizeof(ManualRobot));
    if (seq) *q = seq[rob];
    else memset(q, 0, sizeof(SeqRobotState));
  } else {
    reset_mode = h->reset_mode;
    if (st.manual) {
      if (h->flags & 1) st.manual[rob] = *m;
      else memset(&st.manual[rob], 0, sizeof(ManualRobot));
    }
    if (seq) {
      if (h->flags & 4) seq[rob] = *q;
      else memset(&seq[rob], 0, sizeof(SeqRobotState));
    }
  }
  for (int leg = 0; leg < L; ++leg) {
    const int64_t slot = slot_of(rob, leg, L);
    double *row = legs + size_t(leg) * per_leg;
    for (int f = 0; f < ExtFields::COUNT; ++f) {
      if (!to_engine) row[f] = st.ext ? st.ext[leg_field_index(f, slot, st.n_slots)] : 0.0;
      else if (st.ext) st.ext[leg_field_index(f, slot, st.n_slots)] = (h->flags & 2) ? row[f] : 0.0;
    }
    for (int f = 0; f < tail; ++f) {
      double &x = st.legd[leg_field_index(des_tip_field + f, slot, st.n_slots)];
      if (!to_engine) row[ExtFields::COUNT + f] = x;
      else x = row[ExtFields::COUNT + f];
    }
    for (int f = 0; f < 3; ++f) { // LegPoser::current_tip_pose_.position_ (state while flag 8 holds, an output otherwise)
      double &x = st.legd[leg_field_index(poser_tip_field + f, slot, st.n_slots)];
      if (!to_engine) row[ExtFields::COUNT + tail + f] = x;
      else if (h->flags & 8) x = row[ExtFields::COUNT + tail + f];
    }
  }
}
extern "C" int64_t shc_engine_aux_state_bytes(const shc_engine *e) { return e ? int64_t(aux_bytes(e)) : 0; }
// AuxHeader::flags of the blobs this engine writes now: the lazily allocated records it holds, and whether the LegPoser tips are state
static uint32_t aux_live_flags(const shc_engine *e) {
  return (e->st.manual && (e->rt_flags & RT_MANUAL_LEGS) ? 1u : 0u) | (e->st.ext ? 2u : 0u) | (e->d_seq ? 4u : 0u) | (e->plan_poser_tips_current ? 8u : 0u);
}
static int aux_state(shc_engine *e, int64_t first, int64_t count, void *blobs, int to_engine) {
  if (!blobs) return fail(SHC_ERR_INVALID_ARG, "blobs is NULL");
  if (first < 0 || count < 0 || first + count > e->n) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if (count == 0) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  const size_t stride = aux_bytes(e);
  uint32_t want = 0;
  if (to_engine) { // the engine grows the records the blobs carry
    for (int64_t i = 0; i < count; ++i) {
      const AuxHeader *h = reinterpret_cast<const AuxHeader *>(static_cast<const unsigned char *>(blobs) + size_t(i) * stride);
      if (h->magic != kAuxMagic || h->version != kAuxVersion || h->legs != e->L || h->dof != e->NJ)
        return fail(SHC_ERR_INVALID_ARG, "auxiliary state blob of another library version / morphology");
      want |= h->flags;
    }
    int rc = SHC_OK;
    if ((want & 1) && !e->st.manual) rc = ensure_manual(e);
    if (rc == SHC_OK && (want & 4) && !e->d_seq) rc = ensure_seq(e);
    double *ext_new = nullptr;
    if (rc == SHC_OK && (want & 2) && !e->st.ext) { // (allocated and cleared completely before the engine sees it: a failure leaves nothing half-grown)
      const size_t bytes = size_t(ExtFields::COUNT) * e->n_slots * 8;
      if (hipMalloc(&ext_new, bytes) != hipSuccess) rc = fail(SHC_ERR_HIP, "hipMalloc(external target records)");
      else if (hipMemsetAsync(ext_new, 0, bytes, e->stream) != hipSuccess) {
        (void)hipFree(ext_new);
        rc = fail(SHC_ERR_HIP, "hipMemset(external target records)");
      }
    }
    if (rc != SHC_OK) return rc;
    if (ext_new) e->st.ext = ext_new;
    if (want & 1) e->rt_flags |= RT_MANUAL_LEGS | RT_MANUAL_LIVE;
    if (want & 2) e->rt_flags |= RT_EXTERNAL;
    // "The LegPoser tips of the last plan call are still current" is a fact about the whole engine (any control cycle clears it): a restore
    // of the whole batch sets it from the blobs; a partial restore / migration of a few instances can only keep it when both sides agree -
    // it never raises it for the instances it did not touch, and the per-blob flag stays authoritative for the restored ones.
    if (first == 0 && count == e->n) e->plan_poser_tips_current = (want & 8) != 0;
    else e->plan_poser_tips_current = e->plan_poser_tips_current && (want & 8) != 0;
  }
  HostCall hc(e);
  unsigned char *const host = static_cast<unsigned char *>(blobs);
  unsigned char *d = to_engine ? const_cast<unsigned char *>(hc.in(host, stride * size_t(count), 0)) : hc.out(host, stride * size_t(count), 0);
  if (const int rc = hc.status()) return rc;
  const uint32_t live = aux_live_flags(e);
  aux_state_kernel<<<dim3((unsigned)((count + 127) / 128)), dim3(128), 0, e->stream>>>(d, stride, e->st, e->d_seq, e->L, e->NJ, LEG_FIELD(e, DES_TIP), e->n_leg_fields,
                                                                                   first, count, to_engine, live, LEG_FIELD(e, POSER_TIP));
  return hc.finish();
}
extern "C" int shc_engine_get_aux_state(shc_engine *e, int64_t first, int64_t count, void *blobs) {
  SHC_ENTER_JOINED(e);
  return aux_state(e, first, count, blobs, 0);
}
extern "C" int shc_engine_set_aux_state(shc_engine *e, int64_t first, int64_t count, const void *blobs) {
  SHC_ENTER_JOINED(e);
  return aux_state(e, first, count, const_cast<void *>(blobs), 1);
}
