// shc_loop_calls.hpp — the loop-level calls: every StateController::loop() that is not the plain control cycle.
//   direct start-up, sequence start-up / shut-down, stepToNewStance, legStateToggle, executePlan, packLegs / unpackLegs, finish_sequence_startup
// One driver (loop_call) owns the protocol they share - mark / pose pass / body / marked cycle - and one guard (RtFlagsGuard) owns every temporary change of
// e->rt_flags.  The kernels are shc_sequence.hpp's.  Included by shc_engine.hip once the per-leg entry points (LegCall, LEG_KERNEL) are defined.

// e->rt_flags with `raise` added for the lifetime of the guard; the word the guard found is put back when it leaves scope, on every way out.
struct RtFlagsGuard {
  shc_engine *e;
  const unsigned keep;
  explicit RtFlagsGuard(shc_engine *e_, unsigned raise = 0) : e(e_), keep(e_->rt_flags) { e->rt_flags |= raise; }
  RtFlagsGuard(const RtFlagsGuard &) = delete;
  ~RtFlagsGuard() { e->rt_flags = keep; }
};

// LegPoser::transitionConfiguration's progress is a function of its iteration count alone (pose_controller.cpp:1546-1566): `calls` iterations made,
// this one included, out of `iterations`.
static int transition_progress(int calls, int iterations) {
  if (calls >= iterations) return 100;
  const int p = int((double(calls - 1) / double(iterations)) * 100);
  return p < 1 ? 1 : (p > 100 ? 100 : p);
}

// One iteration of LegPoser::transitionConfiguration on every leg of every robot towards one [L][NJ] configuration shared by all instances
static int transition_every_leg(shc_engine *e, const std::vector<double> &target, double transition_time) {
  LegCall c;
  int rc = c.init(e, 0, e->n, -1);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(target.data(), target.size(), 0);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_transition_configuration_kernel, d, 0, transition_time, e->params.time_delta, (int32_t *)nullptr)) != SHC_OK) return rc;
  return hc.finish();
}

extern "C" int shc_engine_begin_direct_startup(shc_engine *e) {
  SHC_ENTER_JOINED(e);
  int rc = init_state(e);
  if (rc != SHC_OK) return rc;
  // Leg::init(true) (model.cpp:286-305): Joint::default_position_ = clamped(0, min, max) (:1038)
  const std::vector<double> q0 = leg_joint_table(e, [&](int l, int j) { return clampd(0.0, e->params.joint[l][j].min, e->params.joint[l][j].max); });
  HostCall hc(e);
  const double *d = hc.in(q0.data(), q0.size(), 0);
  if ((rc = hc.status()) != SHC_OK) return rc;
  dispatch_nj(e->NJ, [&](auto nj) { set_initial_joints_kernel<decltype(nj)::value><<<grid256(e->n * e->L), dim3(256), 0, e->stream>>>(e->st, d, e->L); });
  if ((rc = hc.finish()) != SHC_OK) return rc;
  e->startup_calls = 0;
  e->starting_up = 1;
  return SHC_OK;
}

extern "C" int shc_engine_direct_startup(shc_engine *e, int32_t *progress) {
  SHC_ENTER_JOINED(e);
  if (!e->starting_up) return fail(SHC_ERR_INVALID_ARG, "call shc_engine_begin_direct_startup first");
  HIP_TRY(hipSetDevice(e->device));
  // desired_configuration_ of every leg = the joints the simulated start-up solve ended on (pose_controller.cpp:476-510):
  // the init chain's default_joint_position, one row per leg shared by all instances
  const std::vector<double> target = leg_joint_table(e, [&](int l, int j) { return e->tables.default_joint_position[l][j]; });
  int rc = transition_every_leg(e, target, e->params.time_to_start);
  if (rc != SHC_OK) return rc;
  const int p = transition_progress(++e->startup_calls, hostinit::startup_loops(e->params)); // (every leg runs the same number of iterations)
  if (p == 100) {
    e->starting_up = 0;
    // READY reached; the loop that enters RUNNING also runs the first control cycle (state_controller.cpp:277-281, :189-192)
    if ((rc = shc_engine_step(e, 1)) != SHC_OK) return rc;
  }
  if (progress) *progress = p;
  return SHC_OK;
}

// ---- start-up / shut-down sequences (start_up_sequence: true; shc_sequence.hpp)
extern "C" int shc_engine_begin_sequence_startup(shc_engine *e, const double *joint_positions, int per_instance) {
  SHC_ENTER_JOINED(e);
  // (arguments first: an INVALID_ARG return leaves the batch as it was)
  if (per_instance && !joint_positions) return fail(SHC_ERR_INVALID_ARG, "per_instance needs joint_positions");
  const size_t rows = per_instance ? size_t(e->n) * e->L : size_t(e->L);
  // (without positions: READY, every joint at its `unpacked` position, state_controller.cpp:217, :236)
  const std::vector<double> q = joint_positions ? std::vector<double>(joint_positions, joint_positions + rows * e->NJ)
                                                : leg_joint_table(e, [&](int l, int j) { return e->params.joint[l][j].unpacked; });
  e->fresh_pose_controller = true;
  int rc = init_state(e); // StateController::init(): fresh walker / poser state
  e->fresh_pose_controller = false;
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(q.data(), q.size(), 0);
  if ((rc = hc.status()) != SHC_OK) return rc;
  set_joint_positions_kernel<<<grid256(e->n * e->L), dim3(256), 0, e->stream>>>(e->st, d, per_instance, e->L, e->NJ, LEG_FIELD(e, Q), LEG_FIELD(e, QD), LEG_FIELD(e, MEAS_Q));
  HIP_TRY(hipGetLastError());
  if (e->d_seq) HIP_TRY(hipMemsetAsync(e->d_seq, 0, sizeof(SeqRobotState) * size_t(e->n), e->stream)); // fresh PoseController
  if ((rc = hc.finish()) != SHC_OK) return rc;
  e->starting_up = 0;
  e->pack_step = e->executing_transition = e->transition_calls = 0;
  return SHC_OK;
}

static int ensure_seq(shc_engine *e) { // the per-robot PoseController records of the sequence / planner kernels, on first use
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_seq) {
    HIP_TRY(hipMalloc(&e->d_seq, sizeof(SeqRobotState) * size_t(e->n)));
    HIP_TRY(hipMemsetAsync(e->d_seq, 0, sizeof(SeqRobotState) * size_t(e->n), e->stream));
  }
  return SHC_OK;
}
static int ensure_manual_records(shc_engine *e) { // the per-robot ManualRobot records (all legs WALKING, no skip marks), on first use; no flag changes
  HIP_TRY(hipSetDevice(e->device));
  if (!e->st.manual) {
    HIP_TRY(hipMalloc(&e->st.manual, sizeof(ManualRobot) * size_t(e->n_rob_pad)));
    HIP_TRY(hipMemsetAsync(e->st.manual, 0, sizeof(ManualRobot) * size_t(e->n_rob_pad), e->stream)); // all WALKING
    const std::vector<int32_t> none(size_t(e->n), -1);
    HostCall hc(e);
    const int32_t *d = hc.in(none.data(), none.size(), 0);
    if (const int rc = hc.status()) return rc;
    set_manual_inputs_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(e->st.manual, e->n, d, nullptr, nullptr, d, nullptr, nullptr);
    return hc.finish();
  }
  return SHC_OK;
}
static int ensure_manual(shc_engine *e) {
  if (e->cp.tip_align)
    return fail(SHC_ERR_UNSUPPORTED, "manual leg manipulation / planner mode with the tip-align pose (gravity_aligned_tips on <= 3-DOF legs)");
  const int rc = ensure_manual_records(e);
  if (rc != SHC_OK) return rc;
  e->rt_flags |= RT_MANUAL_LEGS | RT_MANUAL_LIVE; // (the toggle resets the manual pose: its group of the robot tile is live from now on)
  return SHC_OK;
}

// The body pose has parts that move while a robot stands (IMU PID, auto-pose latches, inclination): the posing part of a loop-level
// call then runs in the cycle kernel (RT_POSE_MARKED), not in the loop-level kernel.
static bool posing_needs_pose_pass(const shc_engine *e) { return e->params.imu_posing || e->params.auto_posing || e->params.inclination_posing; }
static SeqParams seq_params(const shc_engine *e) {
  SeqParams P{};
  const shc_params &q = posing_params(e); // shc_adjust.hpp, row "seq_params, toggle_leg_state"
  P.step_frequency = e->params.step_frequency;
  P.swing_height = q.swing_height;
  P.dt = e->params.time_delta;
  P.force_gain = q.force_gain;
  P.clamp_vel = e->params.clamp_joint_velocities;
  P.clamp_pos = e->params.clamp_joint_positions;
  P.tip_force = e->cp.tip_force;
  P.have_adm = e->params.admittance_control;
  P.gravity_aligned = rotations_tracked(e);
  P.inclination_posing = e->params.inclination_posing;
  P.gravity_aligned_tips = e->params.gravity_aligned_tips;
  P.pose_pass = posing_needs_pose_pass(e);
  P.poser_tip_kept = e->params.auto_posing && !e->params.imu_posing;
  return P;
}
// One launch of the cycle kernel that treats the marked robots apart.  RT_POSE_MARKED: the pose pass - their PoseController::updateCurrentPose + admittance
// update, everybody else untouched.  RT_SKIP_MARKED: the marked cycle - one ordinary control cycle that they keep out of.
static int cycle_apart(shc_engine *e, unsigned how) {
  const RtFlagsGuard flags(e, how);
  return shc_engine_step(e, 1);
}
static dim3 robot_grid(const shc_engine *e) { return dim3((unsigned)((e->n + 63) / 64)); } // the loop-level kernels: one thread per robot, blocks of 64

// One loop-level call.  launch(phase) enqueues the call's kernel for one phase and returns SHC_OK or an error.
//   posed:  launch(LOOP_MARK) marks the robots whose loop this call is, the pose pass runs the posing part of their loop, then
//           launch(LOOP_AFTER_POSE) does the rest;        else: launch(LOOP_WHOLE) does both.
//   hc.finish() brings back what the kernel returned - `ordinary_cycle` with it, when given: a host word the kernel raises if the loop of some robots is the
//   ordinary control cycle: the marked cycle, waited for.  end() is the tail of the call.
template <class Launch, class End>
static int loop_call(shc_engine *e, HostCall &hc, bool posed, Launch &&launch, const int32_t *ordinary_cycle, End &&end) {
  int rc;
  if (posed) {
    if ((rc = launch(LOOP_MARK)) != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    if ((rc = cycle_apart(e, RT_POSE_MARKED)) != SHC_OK) return rc;
  }
  if ((rc = launch(posed ? LOOP_AFTER_POSE : LOOP_WHOLE)) != SHC_OK) return rc;
  if ((rc = hc.finish()) != SHC_OK) return rc;
  if (ordinary_cycle && *ordinary_cycle) {
    if ((rc = cycle_apart(e, RT_SKIP_MARKED)) != SHC_OK) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
  }
  return end();
}

// executeSequence / stepToNewStance under auto posing on its own clock: the skip marks of the robots whose sequence still runs (sequence_mark_kernel), and
// RT_MANUAL_LEGS / RT_MANUAL_LIVE - the pose-only pass runs on the manual-leg kernels (the marks live in the ManualRobot records), but no leg is toggled by a
// sequence: a later shc_engine_step keeps its kernels, shc_engine_step_k / resident mode stay available.  Neither outlives the scope, whichever way it is
// left: a marked robot would sit out every later cycle.
struct SequenceMarks {
  shc_engine *e;
  const int which;
  const RtFlagsGuard flags;
  bool set = false;
  SequenceMarks(shc_engine *e_, int which_) : e(e_), which(which_), flags(e_, RT_MANUAL_LEGS | RT_MANUAL_LIVE) {}
  void mark(bool on) {
    sequence_mark_kernel<<<robot_grid(e), dim3(64), 0, e->stream>>>(e->st.manual, e->d_seq, e->n, which, on ? 1 : 0);
    set = on;
  }
  ~SequenceMarks() { if (set) mark(false); }
};

static int sequence_launch(shc_engine *e, int which /* 0 / 1: executeSequence(START_UP / SHUT_DOWN), 2: stepToNewStance */, int32_t *progress) {
  SHC_ENTER_JOINED(e);
  int rc = ensure_seq(e);
  if (rc != SHC_OK) return rc;
  SeqParams P = seq_params(e);
  if (e->cp.gravity_target) { // identity tip rotation of gravity-aligned tips (walk_controller.cpp:37-41)
    const Quat r = from_two_vectors(V3{1, 0, 0}, V3{e->cp.target_dir[0], e->cp.target_dir[1], e->cp.target_dir[2]});
    P.target_rotation[0] = r.w, P.target_rotation[1] = r.x, P.target_rotation[2] = r.y, P.target_rotation[3] = r.z;
  }
  HostCall hc(e);
  int32_t *d_progress = hc.scratch<int32_t>(size_t(e->n));
  hc.back(progress, d_progress, size_t(e->n));
  if ((rc = hc.status()) != SHC_OK) return rc;
  // Auto posing on its own clock keeps posing through the sequence (pose_controller.cpp:1134-1187 runs in every loop, state_controller.cpp:165-167): the
  // posing part of this loop runs in the cycle kernel for the robots whose sequence is still running (a pose-only pass, as for leg toggles and plan steps)
  const bool own_clock = e->params.auto_posing && e->params.pose_frequency != -1.0;
  std::optional<SequenceMarks> marks;
  if (own_clock) {
    if (e->cp.tip_align)
      return fail(SHC_ERR_UNSUPPORTED, "executeSequence / stepToNewStance with auto posing on its own clock on robots that carry the tip-align pose "
                                       "(gravity_aligned_tips on <= 3-DOF legs): the pose-only pass has no tip-align form");
    if ((rc = ensure_manual_records(e)) != SHC_OK) return rc;
    marks.emplace(e, which);
  }
  P.posed = own_clock;
  const auto launch = [&](int phase) -> int {
    if (phase == LOOP_MARK) return marks->mark(true), SHC_OK;
    rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      if (which == 2) step_to_new_stance_kernel<L, NJ><<<robot_grid(e), dim3(64), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, e->d_seq, P, d_progress);
      else execute_sequence_kernel<L, NJ><<<robot_grid(e), dim3(64), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, e->d_seq, which, P, d_progress);
      return SHC_OK;
    });
    if (rc != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    if (marks) {
      marks->mark(false);
      marks.reset(); // (the flags as they were before the tail below reads them)
      HIP_TRY(hipGetLastError());
    }
    return SHC_OK;
  };
  // shc_adjust.hpp, rows "SHUT_DOWN" / "START_UP sequence step, step_to_new_stance"
  return loop_call(e, hc, own_clock, launch, nullptr, [&] { return which == SHC_SEQUENCE_SHUT_DOWN ? adjust_served_by_loop(e) : SHC_OK; });
}

extern "C" int shc_engine_execute_sequence(shc_engine *e, int sequence, int32_t *progress) {
  SHC_ENTER_JOINED(e);
  if (sequence != SHC_SEQUENCE_START_UP && sequence != SHC_SEQUENCE_SHUT_DOWN) return fail(SHC_ERR_INVALID_ARG, "sequence must be SHC_SEQUENCE_START_UP or SHC_SEQUENCE_SHUT_DOWN");
  return sequence_launch(e, sequence, progress);
}

extern "C" int shc_engine_step_to_new_stance(shc_engine *e, int32_t *progress) { return sequence_launch(e, 2, progress); }

// ---- manual leg manipulation (shc_sequence.hpp)
extern "C" int shc_engine_toggle_leg_state(shc_engine *e, const int32_t *leg_selection, int32_t *result) {
  SHC_ENTER_JOINED(e);
  int rc = ensure_manual(e);
  if (rc != SHC_OK) return rc;
  if (!leg_selection) return fail(SHC_ERR_INVALID_ARG, "leg_selection is NULL");
  int32_t cycle = 0; // robots without a request, or asked to stop first: their loop is one ordinary control cycle; the others keep out of it
  HostCall hc(e);
  const int32_t *d_sel = hc.in(leg_selection, size_t(e->n), 0);
  int32_t *d_res = hc.scratch<int32_t>(size_t(e->n)), *d_cycle = hc.out(&cycle, 1, 0);
  hc.back(result, d_res, size_t(e->n));
  if ((rc = hc.status()) != SHC_OK) return rc;
  HIP_TRY(hipMemsetAsync(d_cycle, 0, 4, e->stream));
  const SeqParams P = seq_params(e);
  const double virtual_stiffness = posing_params(e).virtual_stiffness; // (as seq_params)
  const auto toggle = [&](int phase) {
    return dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      leg_state_toggle_kernel<L, NJ><<<robot_grid(e), dim3(64), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, d_sel, P, virtual_stiffness,
                                                                               e->params.swing_stiffness_scaler, e->params.load_stiffness_scaler,
                                                                               e->params.admittance_control && e->params.dynamic_stiffness, d_res, d_cycle, phase);
      return SHC_OK;
    });
  };
  return loop_call(e, hc, P.pose_pass, toggle, &cycle, [&] { return adjust_served_by_loop(e); }); // shc_adjust.hpp, row "toggle_leg_state, execute_plan"
}

extern "C" int shc_engine_set_manual_inputs(shc_engine *e, const int32_t *primary_leg, const double *primary_tip_velocity, const double *primary_tip_position,
                                            const int32_t *secondary_leg, const double *secondary_tip_velocity, const double *secondary_tip_position) {
  SHC_ENTER_JOINED(e);
  int rc = ensure_manual(e);
  if (rc != SHC_OK) return rc;
  const size_t n = size_t(e->n);
  HostCall hc(e);
  const int32_t *d_p = hc.in(primary_leg, n, 0), *d_s = hc.in(secondary_leg, n, 0);
  const double *src[4] = {primary_tip_velocity, primary_tip_position, secondary_tip_velocity, secondary_tip_position}, *d_v[4];
  for (int k = 0; k < 4; ++k) d_v[k] = hc.in(src[k], n * 3, 0);
  if ((rc = hc.status()) != SHC_OK) return rc;
  set_manual_inputs_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(e->st.manual, e->n, d_p, d_v[0], d_v[1], d_s, d_v[2], d_v[3]);
  hc.wait_at_finish(); // (also when every array is NULL)
  return hc.finish();
}

extern "C" int shc_engine_get_leg_manipulation_state(shc_engine *e, int32_t *states) {
  SHC_ENTER_JOINED(e);
  if (!states) return fail(SHC_ERR_INVALID_ARG, "states is NULL");
  const int64_t rows = e->n * e->L;
  return gather_output(e, states, size_t(rows), 0, [&](int32_t *d) {
    get_leg_manipulation_state_kernel<<<grid256(rows), dim3(256), 0, e->stream>>>(e->st.manual, e->n, e->L, d);
  });
}

// ---- planner mode (shc_sequence.hpp: execute_plan_kernel)
static int ensure_planner(shc_engine *e) {
  int rc = ensure_manual(e); // the ManualRobot records carry the skip marks of the loop-level kernels
  if (rc != SHC_OK) return rc;
  return ensure_seq(e);
}
static int plan_inputs(shc_engine *e, int64_t first, int64_t count, int reset_plan_step, const double *configuration, const double *body_pose) {
  int rc = ensure_planner(e);
  if (rc != SHC_OK) return rc;
  if (first < 0 || count < 0 || first + count > e->n) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if (count == 0) return SHC_OK;
  const size_t cfg_doubles = configuration ? size_t(count) * e->L * e->NJ : 0, pose_doubles = body_pose ? size_t(count) * 7 : 0;
  HostCall hc(e);
  const double *d_cfg = hc.in(configuration, cfg_doubles, 0), *d_pose = hc.in(body_pose, pose_doubles, 0);
  if ((rc = hc.status()) != SHC_OK) return rc;
  plan_inputs_kernel<<<grid256(count), dim3(256), 0, e->stream>>>(e->d_seq, first, count, e->L, e->NJ, reset_plan_step, d_cfg, d_pose);
  hc.wait_at_finish(); // (also when both arrays are NULL)
  return hc.finish();
}

extern "C" int shc_engine_set_planner_mode(shc_engine *e, int on) {
  SHC_ENTER_JOINED(e);
  if ((on != 0) == e->planner_mode) return SHC_OK; // plannerModeCallback acts on a change only (state_controller.cpp:1267)
  e->planner_mode = on != 0;
  return on ? plan_inputs(e, 0, e->n, 1, nullptr, nullptr) : SHC_OK; // plan_step_ = 0 (:1273)
}
extern "C" int shc_engine_set_target_configuration(shc_engine *e, int64_t first, int64_t count, const double *configuration) {
  SHC_ENTER_JOINED(e);
  if (!configuration) return fail(SHC_ERR_INVALID_ARG, "configuration is NULL");
  return plan_inputs(e, first, count, 0, configuration, nullptr);
}
extern "C" int shc_engine_set_target_body_pose(shc_engine *e, int64_t first, int64_t count, const double *pose) {
  SHC_ENTER_JOINED(e);
  if (!pose) return fail(SHC_ERR_INVALID_ARG, "pose is NULL");
  return plan_inputs(e, first, count, 0, nullptr, pose);
}

extern "C" int shc_engine_execute_plan(shc_engine *e, int32_t *progress, int32_t *plan_step) {
  SHC_ENTER_JOINED(e);
  int rc = ensure_planner(e);
  if (rc != SHC_OK) return rc;
  int32_t walking = 0; // the loop of the robots that are still walking is the normal control cycle (inputs zeroed); the others keep out of it
  HostCall hc(e);
  int32_t *d_progress = hc.scratch<int32_t>(size_t(e->n)), *d_step = hc.scratch<int32_t>(size_t(e->n)), *d_walking = hc.out(&walking, 1, 0);
  hc.back(progress, d_progress, size_t(e->n)), hc.back(plan_step, d_step, size_t(e->n));
  if ((rc = hc.status()) != SHC_OK) return rc;
  HIP_TRY(hipMemsetAsync(d_walking, 0, 4, e->stream));
  const SeqParams P = seq_params(e);
  const int reset_poser_tips = e->plan_poser_tips_current ? 0 : 1;
  const auto plan = [&](int phase) -> int {
    rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      execute_plan_kernel<L, NJ><<<robot_grid(e), dim3(64), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, e->d_seq, P, reset_poser_tips, d_progress,
                                                                           d_step, d_walking, phase);
      return SHC_OK;
    });
    if (rc != SHC_OK || phase == LOOP_MARK) return rc;
    HIP_TRY(hipGetLastError());
    e->plan_poser_tips_current = true;
    return SHC_OK;
  };
  return loop_call(e, hc, P.pose_pass, plan, &walking, [&] { return adjust_served_by_loop(e); }); // shc_adjust.hpp, row "toggle_leg_state, execute_plan"
}

// PoseController::packLegs / unpackLegs (pose_controller.cpp:615-707)
static int pack_transition(shc_engine *e, const double *packed_positions, int n_pack_steps, double transition_time, bool unpack, int32_t *progress) {
  if (!packed_positions || n_pack_steps < 1) return fail(SHC_ERR_INVALID_ARG, "packed_positions / n_pack_steps");
  if (!(transition_time > 0)) return fail(SHC_ERR_INVALID_ARG, "transition time must be > 0");
  HIP_TRY(hipSetDevice(e->device));
  if (e->pack_step >= n_pack_steps) e->pack_step = n_pack_steps - 1;
  // desired_configuration_ of every leg (:628-642, :676-693); the kernel latches it when a transition begins
  const int source_step = unpack ? e->pack_step - 1 : e->pack_step; // (unpacking from the first pack step: to the `unpacked` positions)
  const double *source = packed_positions + size_t(source_step < 0 ? 0 : source_step) * e->L * e->NJ;
  const std::vector<double> target =
      leg_joint_table(e, [&](int l, int j) { return source_step < 0 ? e->params.joint[l][j].unpacked : source[size_t(l) * e->NJ + j]; });
  const int rc = transition_every_leg(e, target, transition_time);
  if (rc != SHC_OK) return rc;
  const int num = round_to_int(transition_time / e->params.time_delta);
  int p = transition_progress(++e->transition_calls, num > 1 ? num : 1);
  if (p == 100) e->transition_calls = 0;
  e->executing_transition = (p != 0 && p != 100);
  if (!unpack) {
    if (p == 100 && e->pack_step < n_pack_steps - 1) {
      e->executing_transition = 0;
      e->pack_step++;
      p = 0;
    }
  } else if (p == 100 && e->pack_step != 0) {
    e->executing_transition = 0;
    e->pack_step--;
    p = 0;
  }
  if (progress) *progress = p;
  return SHC_OK;
}

extern "C" int shc_engine_pack_legs(shc_engine *e, const double *packed_positions, int n_pack_steps, double time_to_pack, int32_t *progress) {
  SHC_ENTER_JOINED(e);
  return pack_transition(e, packed_positions, n_pack_steps, time_to_pack, false, progress);
}

extern "C" int shc_engine_unpack_legs(shc_engine *e, const double *packed_positions, int n_pack_steps, double time_to_unpack, int32_t *progress) {
  SHC_ENTER_JOINED(e);
  return pack_transition(e, packed_positions, n_pack_steps, time_to_unpack, true, progress);
}

extern "C" int shc_engine_finish_sequence_startup(shc_engine *e) {
  SHC_ENTER_JOINED(e);
  HIP_TRY(hipSetDevice(e->device));
  // Auto posing on its own clock (pose_frequency != -1) poses the body through the sequence calls (sequence_launch), and the PoseController lives on through
  // walker_->init() (:306): its phase counter, the posers' latches and Model::current_pose_ carry over, Leg::generateWorkspace searches at the pose of THAT loop
  // (model.cpp:338) and the runningState() of the same loop reuses it (updateCurrentPose, :165-167, ran once, before the sequence call).  Here: the poser part of
  // every instance's state record is kept across the re-initialisation, the workspace search runs at the kept pose, and the phase counter is set back by one so
  // that the posing part of the full cycle below recomputes the pose of this loop instead of the next one - exact because that part is idempotent in this
  // configuration: with its own clock an AutoPoser's latches are OR-latches that are already set (pose_controller.cpp:1359-1371), LegPoser::updateAutoPose
  // (:1716-1778) is a function of the phase and a latch the same phase sets, the manual pose is checked to be at rest.  IMU posing is the exception
  // (updateIMUPose needs RUNNING, :836: the loop that completes START_UP poses with the auto pose, the cycle below would pose with the PID) and stays refused.
  const bool own_clock = e->params.auto_posing && e->params.pose_frequency != -1.0;
  std::vector<shc_instance_state> kept;
  Pose ws_pose = pose_identity();
  if (own_clock) {
    if (e->params.imu_posing)
      return fail(SHC_ERR_UNSUPPORTED, "finish_sequence_startup with auto posing on its own clock AND IMU posing (the loop that completes START_UP still poses with "
                                       "the auto pose, pose_controller.cpp:836; start such robots with the direct start-up, shc_engine_create)");
    if (e->cp.tip_align) return fail(SHC_ERR_UNSUPPORTED, "finish_sequence_startup with auto posing on its own clock on robots that carry the tip-align pose");
    kept.resize(size_t(e->n));
    int rck = shc_engine_get_state(e, 0, e->n, kept.data());
    if (rck != SHC_OK) return rck;
    const shc_instance_state &k0 = kept[0];
    for (int64_t i = 0; i < e->n; ++i) {
      const shc_instance_state &k = kept[size_t(i)];
      bool same = k.pose_phase == k0.pose_phase && memcmp(k.auto_poser_flags, k0.auto_poser_flags, sizeof(k.auto_poser_flags)) == 0;
      bool rest = k.manual_pose[0] == 0 && k.manual_pose[1] == 0 && k.manual_pose[2] == 0 && k.manual_pose[4] == 0 && k.manual_pose[5] == 0 && k.manual_pose[6] == 0;
      for (int a = 0; a < 3; ++a) rest = rest && k.translation_velocity_input[a] == 0 && k.rotation_velocity_input[a] == 0;
      if (!same)
        return fail(SHC_ERR_UNSUPPORTED, "finish_sequence_startup: the instances completed START_UP in different phases of the auto pose (instance " + std::to_string(i) +
                                             " vs instance 0): the workspace is searched at the body pose of the completing loop and one engine has one set of tables");
      if (!rest)
        return fail(SHC_ERR_UNSUPPORTED, "finish_sequence_startup with auto posing on its own clock while the manual body pose is in motion (instance " + std::to_string(i) + ")");
    }
    ws_pose = Pose{V3{k0.current_pose[0], k0.current_pose[1], k0.current_pose[2]}, Quat{k0.current_pose[3], k0.current_pose[4], k0.current_pose[5], k0.current_pose[6]}};
  }
  // Model::updateDefaultConfiguration + generateWorkspaces + generateWalkspace (state_controller.cpp:307-310): the tables of an
  // engine belong to its morphology, so the configuration of instance 0 stands for the batch.  Robots that were started from
  // different joint positions (shc_engine_begin_sequence_startup per_instance) end their sequences on the same READY stance
  // only up to the tip tolerances of the last steps (a few milliradians): the largest difference to instance 0 is checked here -
  // beyond 0.02 rad (IK_TOLERANCE, 5 mm, at the end of a 0.25 m leg) the batch does not share one configuration and the caller has to
  // start such robots in engines of their own.
  std::vector<double> q(size_t(e->n) * e->L * e->NJ);
  int rc = shc_engine_get_joint_state(e, q.data(), nullptr, 0);
  if (rc != SHC_OK) return rc;
  {
    const size_t row = size_t(e->L) * e->NJ;
    double worst = 0.0;
    for (int64_t i = 1; i < e->n; ++i)
      for (size_t k = 0; k < row; ++k) worst = fmax(worst, fabs(q[size_t(i) * row + k] - q[k]));
    if (!(worst <= 0.02))
      return fail(SHC_ERR_UNSUPPORTED, "finish_sequence_startup: the instances ended their start-up sequences on different configurations (max |dq| to instance 0 = " +
                                           std::to_string(worst) + " rad): one engine has one set of workspace / limit tables");
  }
  shc_tables t;
  const bool ok = dispatch_nj(e->NJ, [&](auto nj) { return hostinit::generate_tables<decltype(nj)::value>(e->params, t, q.data(), own_clock ? &ws_pose : nullptr); });
  if (!ok) return fail(SHC_ERR_INVALID_ARG, "init chain failed for the configuration the sequence ended on");
  e->tables = t;
  e->span_dirty = true;
  rebuild_cycle_params(e); // (shc_adjust.hpp, row "shc_engine_finish_sequence_startup")
  if ((rc = upload_consts(e)) != SHC_OK) return rc;
  // walker_->init() (:306): fresh LegSteppers / walk state; the joints stay where the sequence left them
  const int n_joint_planes = (2 * e->NJ + 1) / 2 + 1; // planes holding Q and QD (Fields: Q = 0, QD = NJ, TIP = 2 NJ)
  const int64_t count = int64_t(n_joint_planes) * e->n_slots;
  {
    HostCall hc(e);
    double2 *keep = hc.scratch<double2>(size_t(count));
    if ((rc = hc.status()) != SHC_OK) return rc;
    copy_joint_planes_kernel<<<grid256(count), dim3(256), 0, e->stream>>>(keep, reinterpret_cast<const double2 *>(e->st.legd), count);
    if ((rc = hc.finish()) != SHC_OK || (rc = init_state(e)) != SHC_OK) return rc;
    restore_joints_kernel<<<grid256(e->n * e->L), dim3(256), 0, e->stream>>>(e->st, keep, e->L, e->NJ);
    hc.wait_at_finish(); // (keep is read again)
    if ((rc = hc.finish()) != SHC_OK) return rc;
  }
  if (own_clock) { // the PoseController's part of the record carries over, one phase back (see above)
    std::vector<shc_instance_state> fresh(size_t(e->n));
    if ((rc = shc_engine_get_state(e, 0, e->n, fresh.data())) != SHC_OK) return rc;
    const int len = e->tables.pose_phase_length > 0 ? e->tables.pose_phase_length : 1;
    for (int64_t i = 0; i < e->n; ++i) {
      shc_instance_state &f = fresh[size_t(i)];
      const shc_instance_state &k = kept[size_t(i)];
      f.pose_phase = (k.pose_phase + len - 1) % len;
      f.auto_posing_state = k.auto_posing_state;
      memcpy(f.auto_poser_flags, k.auto_poser_flags, sizeof(f.auto_poser_flags));
      memcpy(f.auto_pose_rotation, k.auto_pose_rotation, sizeof(f.auto_pose_rotation));
      memcpy(f.current_pose, k.current_pose, sizeof(f.current_pose));
      for (int l = 0; l < SHC_MAX_LEGS; ++l) f.leg[l].negate_auto_pose = k.leg[l].negate_auto_pose;
    }
    const RtFlagsGuard flags(e); // (the injected manual pose is the identity it was: its group of the robot tile stays as live as it was)
    if ((rc = shc_engine_set_state(e, 0, e->n, fresh.data())) != SHC_OK) return rc;
  }
  // robot_state_ = RUNNING, and the runningState() of the same loop (:189-192)
  if ((rc = shc_engine_step(e, 1)) != SHC_OK) return rc;
  return shc_engine_synchronize(e);
}
