// shc_adjust.hpp — shc_engine_adjust_parameter and the one owner of a change that waits for its loop (host side only).
//
// StateController::adjustParameter does not take effect at once.  It runs at the end of runningState (state_controller.cpp:411-414), after the posing part of
// that loop (:165-180) and after transitionRobotState / legStateToggle / executePlan (:384-410), before updateWalk.  An adjusted parameter therefore waits
// for the next loop that reaches runningState.  In that loop
//   - the posing part and the loop-level kernels still read the old force gain / virtual spring / swing height (`params_held`), and
//   - an accepted step-frequency change maps the walking robots' phases onto the new step cycle between the posing part and updateWalk (`step_remap`).
// PendingAdjust holds that state; nothing outside this header reads or writes its members.  Who does what with it:
//
//   entry point                                   operation                    why (state_controller.cpp)
//   shc_engine_step, first cycle                  adjust_serve_in_cycle        the loop that reaches runningState: its cycle runs alone on the held block (:384-414)
//   shc_engine_step_k, cycle 1                    adjust_pending -> the serial form, i.e. shc_engine_step
//   shc_engine_finish_sequence_startup            (none: its shc_engine_step)  the loop that completes START_UP runs runningState itself (:305-314, :189-192)
//   toggle_leg_state, execute_plan, SHUT_DOWN     adjust_served_by_loop        loop-level calls inside runningState; adjustParameter follows them (:384-414)
//   START_UP sequence step, step_to_new_stance    (none: stays pending)        READY's loop() does not reach runningState (:184-192); stepToNewStance is no loop
//   a second step-frequency change, resident_begin adjust_serve_now            no stepped cycle comes between: the phases are mapped by a kernel of their own
//   resident_begin while parameters are held      adjust_needs_stepped_cycle   refused: the resident kernel reads one parameter block for its whole life
//   change_gait with every robot STOPPED          adjust_drop                  nothing is left of a change in flight
//   get_state / set_state                         phase_step_cycle             read only: a record shows the phases in the cycle they still count in
//   seq_params, toggle_leg_state                  posing_params                read only: the loop-level kernels of the serving loop read the old values
//   rebuild_cycle_params                          adjust_overlay               the launch-uniform block of the serving cycle
//   change_gait, adjust_parameter                 adjust_bump                  new tables / parameters are installed or queued: older device checkpoints are stale
//   checkpoint capture / restore                  adjust_generation            read only: a restore needs the generation of its capture and nothing pending
//
// Every transition ends with adjust_settle: join the split streams, rebuild the parameter block, upload the constants.
//
// Included twice by shc_engine.hip: before struct shc_engine for the state it owns, and below the engine's helpers for the operations.
#ifndef SHC_ADJUST_STATE
#define SHC_ADJUST_STATE

struct PendingAdjust {
  bool step_remap;        // an accepted step-frequency change waits for its cycle
  bool params_held;       // the posing part of the next cycle still runs on the values a just-adjusted parameter had
  shc_step_cycle old_step; // step_remap: the step cycle the legs' phases still count in
  shc_params held;        // params_held: the parameters as they were before the change
  uint64_t generation;    // counts every installed or queued change of tables / parameters, and every served one: what a device checkpoint was captured under
};

#else // ------------------------------------------------------------------------------------------ operations (struct shc_engine is complete)

static int launch_cycles(shc_engine *e, int n_cycles, bool generic);

static bool adjust_pending(const shc_engine *e) { return e->adjust.step_remap || e->adjust.params_held; }
// ... of a kind only a stepped cycle can serve (a second parameter block for the posing part); a phase remap alone can be served at once
static bool adjust_needs_stepped_cycle(const shc_engine *e) { return e->adjust.params_held; }
// What a reader before the serving loop sees: the parameters the posing part and the loop-level kernels run on ...
static const shc_params &posing_params(const shc_engine *e) { return e->adjust.params_held ? e->adjust.held : e->params; }
// ... and the step cycle the stored phases count in.
static const shc_step_cycle &phase_step_cycle(const shc_engine *e) { return e->adjust.step_remap ? e->adjust.old_step : e->tables.step; }

// What the change leaves of the old values in the launch-uniform block: the period the phases still count in, the posing part's constants.
static void adjust_overlay(const shc_engine *e, CycleParams &cp) {
  if (e->adjust.step_remap) cp.remap_old_period = e->adjust.old_step.period;
  if (e->adjust.params_held) {
    CycleParams h;
    build_cycle_params(e->adjust.held, e->tables, e->features, e->rt_flags, h);
    cp.adm_m00 = h.adm_m00, cp.adm_m01 = h.adm_m01, cp.adm_m10 = h.adm_m10, cp.adm_m11 = h.adm_m11;
    cp.adm_g0 = h.adm_g0, cp.adm_g1 = h.adm_g1;
    cp.virtual_stiffness = h.virtual_stiffness, cp.pose_force_gain = h.pose_force_gain, cp.pose_swing_height = h.pose_swing_height;
  }
}

// The end of every transition (rc: what the transition's own work returned).  upload_consts is ordered behind that work on the engine's stream, and synchronises it.
static int adjust_settle(shc_engine *e, int rc) {
  if (rc == SHC_OK) rc = join_side(e);
  rebuild_cycle_params(e);
  return rc == SHC_OK ? upload_consts(e) : rc;
}
// The generation of tables / parameters a device checkpoint (shc_checkpoint.hpp) is captured under.
static void adjust_bump(shc_engine *e) { ++e->adjust.generation; }
static uint64_t adjust_generation(const shc_engine *e) { return e->adjust.generation; }
// Nothing waits any more; returns whether the phases were still to be mapped.
static bool adjust_take(shc_engine *e) {
  const bool remap = e->adjust.step_remap;
  if (adjust_pending(e)) adjust_bump(e); // (a checkpoint captured while the change waited shows the state before its serving loop)
  e->adjust.step_remap = e->adjust.params_held = false;
  return remap;
}
static void adjust_drop(shc_engine *e) { (void)adjust_take(e); }

// Serve inside a cycle launch: the cycle runs alone in its launch on the held block (not rebuilt until it is through) - the posing part on the old values, the
// phases mapped between the posing part and updateWalk (cycle_front, on the runtime-flag kernels) - and the plain block of the new values follows it.
static int adjust_serve_in_cycle(shc_engine *e, bool generic) {
  const bool remap = adjust_take(e);
  return adjust_settle(e, launch_cycles(e, 1, generic || remap));
}
// Served by a loop-level call: its pose pass and its marked launch ran on the held block and remapped the phases of the robots that walked in it.
static int adjust_served_by_loop(shc_engine *e) {
  if (!adjust_pending(e)) return SHC_OK;
  adjust_drop(e);
  return adjust_settle(e, SHC_OK);
}

// The same arithmetic as in cycle_front, without the reference's ordering against the posing part of that loop.
__global__ void step_remap_kernel(int32_t *legi, const int32_t *robi, int rpw, int64_t n, int L, int old_period, int period, int swing_start, int swing_end,
                                  int stance_end, int stance_start) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n * L) return;
  const int64_t rob = t / L;
  const int leg = int(t - rob * L);
  if ((robi[rob_index(rob, RobotFields::I_WORD, rpw, RobotFields::I_COUNT)] & 3) != WS_MOVING) return;
  int w = legi[slot_of(rob, leg, L)];
  int ph = (w >> LW_PHASE_SHIFT) & LW_PHASE_MASK, st = w & 3;
  const double step_progress = double(ph) / double(old_period);
  ph = int(step_progress * double(period));
  if (st != SS_FORCE_STOP) {
    if (ph >= swing_start && ph < swing_end && st != SS_FORCE_STANCE) st = SS_SWING;
    else if (ph < stance_end || ph >= stance_start) st = SS_STANCE;
  }
  legi[slot_of(rob, leg, L)] = (w & ~(3 | (LW_PHASE_MASK << LW_PHASE_SHIFT))) | st | (ph << LW_PHASE_SHIFT);
}
static int launch_step_remap(shc_engine *e, int old_period) {
  HIP_TRY(hipSetDevice(e->device));
  const int rc = join_side(e);
  if (rc != SHC_OK) return rc;
  const int64_t threads = e->n * e->L;
  const shc_step_cycle &s = e->tables.step;
  step_remap_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, e->stream>>>(e->st.legi, e->st.robi, 64 / e->L, e->n, e->L, old_period, s.period, s.swing_start,
                                                                                       s.swing_end, s.stance_end, s.stance_start);
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}
// Serve outside any loop (the next cycle is not a stepped one): the phases are mapped now, the new values are in force for all of the next cycle.
static int adjust_serve_now(shc_engine *e) {
  if (!adjust_pending(e)) return SHC_OK;
  const int old_period = e->adjust.old_step.period;
  return adjust_settle(e, adjust_take(e) ? launch_step_remap(e, old_period) : SHC_OK);
}

// WalkController::getLimit (walk_controller.cpp:414-436) on the host, for the acceptance test of a step-frequency change: per leg the bearing of its
// stride velocity (linear + angular x the tip's lever arm), rounded to whole degrees, picks the two neighbouring entries of the 45-degree table; the
// interpolation input is an int / int division in the reference (0 except on a table bearing), the smallest value over the legs is the limit.
static double host_get_limit(const double *tips /* [L][3] walker tip positions */, int L, double lx, double ly, double ang, const double *limit /* [9] */) {
  double lowest = kUnassigned;
  for (int l = 0; l < L; ++l) {
    const double sx = lx + ang * -tips[l * 3 + 1], sy = ly + ang * tips[l * 3 + 0];
    int bearing = mod_i(round_to_int(atan2(sy, sx) * (180.0 / M_PI)), 360);
    int upper = ((bearing + 44) / 45) * 45;
    const int lower = mod_i(upper - 45, 360);
    if (bearing < lower) bearing += 360;
    if (upper < lower) upper += 360;
    const double c = double((bearing - lower) / (upper - lower));
    const double lo = limit[lower / 45], hi = limit[mod_i(upper, 360) / 45];
    lowest = fmin(lowest, lo * (1.0 - c) + hi * c);
  }
  return lowest;
}

static int adjust_step_frequency(shc_engine *e, double value, int64_t *pending) {
  shc_params &p = e->params;
  // What the posing part of the accepting loop reads from the legs' steppers must not depend on the step cycle's constants (it runs on the old cycle in the
  // reference, on the new constants here): the walk-plane blend of rough terrain mode and the tip rotations / tip-align pose of gravity_aligned_tips do.
  // WalkController::generateLimits takes its stance radius from leg 0's CURRENT default tip (walk_controller.cpp:322-326), which a stance span modifier moves.
  if (p.rough_terrain_mode || p.gravity_aligned_tips || p.stance_span_modifier != 0.0)
    return fail(SHC_ERR_UNSUPPORTED, "step_frequency cannot be adjusted at run time in rough_terrain_mode, with gravity_aligned_tips or with a stance span modifier "
                                     "(the other eight parameters can); change it between runs, shc_engine_create");
  if (!(value > 0.0)) return fail(SHC_ERR_INVALID_ARG, "step_frequency must be positive");
  int rc = adjust_serve_now(e); // (two changes without a cycle between them)
  if (rc != SHC_OK) return rc;
  shc_params np = p;
  np.step_frequency = value;
  const shc_step_cycle ns = hostinit::generate_step_cycle(np);
  if (ns.period <= 0 || ns.period > LW_PHASE_MASK) return fail(SHC_ERR_INVALID_ARG, "step_frequency gives a degenerate step cycle");
  adjust_bump(e);
  p.step_frequency = value; // p->current_value = new_parameter_value_ (:454): the sequence / transition timings read it from now on, accepted or not
  shc_tables tn = e->tables;
  tn.step = ns;
  hostinit::generate_limits(p, tn); // the four limit maps + the legs' phase offsets of the new cycle
  // :462-463 and generateLimits' setPhaseOffset (walk_controller.cpp:277): the speed maps and the phase offsets are the new cycle's from here on, whether the
  // change is accepted in this loop or not - the walker slows down to them (updateWalk :456-482), which is what makes a later call succeed
  for (int b = 0; b < SHC_N_BEARINGS; ++b) {
    e->tables.max_linear_speed[b] = tn.max_linear_speed[b];
    e->tables.max_angular_speed[b] = tn.max_angular_speed[b];
  }
  for (int l = 0; l < e->L; ++l) e->tables.phase_offset[l] = tn.phase_offset[l];
  // the test of :464-489, for every instance: desired body velocity inside what its velocity input maps to under the new limits
  std::vector<double> vin(size_t(e->n) * 3), vel(size_t(e->n) * 3), tips(size_t(e->n) * e->L * 3);
  if ((rc = gather_rob(e, vin.data(), 3, RobotFields::VIN, 0)) != SHC_OK) return rc;
  if ((rc = gather_rob(e, vel.data(), 3, RobotFields::VLIN, 0)) != SHC_OK) return rc;
  if ((rc = gather_leg(e, tips.data(), 3, LEG_FIELD(e, TIP), 0)) != SHC_OK) return rc;
  int64_t waiting = 0;
  for (int64_t i = 0; i < e->n; ++i) {
    const double *in = &vin[size_t(i) * 3], *v = &vel[size_t(i) * 3], *tp = &tips[size_t(i) * e->L * 3];
    const double max_lin = host_get_limit(tp, e->L, in[0], in[1], in[2], tn.max_linear_speed);
    const double max_ang = host_get_limit(tp, e->L, in[0], in[1], in[2], tn.max_angular_speed);
    double tx, ty, ta;
    if (p.velocity_input_mode == SHC_VEL_THROTTLE) {
      const double nrm = sqrt(in[0] * in[0] + in[1] * in[1]);
      const double k = nrm > 1.0 ? 1.0 / nrm : 1.0; // clamped(vector, 1.0)
      tx = in[0] * k * max_lin;
      ty = in[1] * k * max_lin;
      ta = clampd(in[2], -1.0, 1.0) * max_ang;
      tx *= 1.0 - fabs(in[2]);
      ty *= 1.0 - fabs(in[2]);
    } else {
      const double nrm = sqrt(in[0] * in[0] + in[1] * in[1]);
      const double k = nrm > max_lin ? max_lin / nrm : 1.0;
      tx = in[0] * k;
      ty = in[1] * k;
      ta = clampd(in[2], -max_ang, max_ang);
    }
    if (!(v[0] <= tx && v[1] <= ty && fabs(v[2]) <= fabs(ta))) ++waiting; // (signed comparisons of the linear components: as the reference has them)
  }
  if (pending) *pending = waiting;
  if (waiting) return upload_consts(e); // not yet: the new speed maps / phase offsets are in force, the step cycle and the acceleration maps are the old ones
  // accepted: walker_->generateStepCycle() + generateLimits() (:491-492).  setAutoPoseParams is NOT called (only init / changeGait do): the auto-pose phase
  // tables keep counting in the old step period, as in the reference.
  e->adjust.old_step = e->tables.step; // generateStepCycle's updatePhase for MOVING robots: inside the next cycle (cp.remap_old_period)
  e->adjust.step_remap = true;
  e->tables.step = ns;
  for (int b = 0; b < SHC_N_BEARINGS; ++b) {
    e->tables.max_linear_acceleration[b] = tn.max_linear_acceleration[b];
    e->tables.max_angular_acceleration[b] = tn.max_angular_acceleration[b];
  }
  rebuild_cycle_params(e);
  return upload_consts(e);
}

extern "C" int shc_engine_adjust_parameter(shc_engine *e, int which, double value, int64_t *pending) {
  SHC_ENTER_JOINED(e);
  if (pending) *pending = 0;
  if (!(value == value) || fabs(value) > 1e300) return fail(SHC_ERR_INVALID_ARG, "parameter value is not finite");
  HIP_TRY(hipSetDevice(e->device));
  shc_params &p = e->params;
  const shc_params old = p;
  switch (which) {
    case SHC_PARAM_STEP_FREQUENCY: return adjust_step_frequency(e, value, pending);
    case SHC_PARAM_SWING_HEIGHT: p.swing_height = value; break;          // LegStepper::updateStride's swing clearance, the dynamic-stiffness reference, sequence step heights
    case SHC_PARAM_SWING_WIDTH: p.swing_width = value; break;            // generateSecondarySwingControlNodes' lateral shift (walk_controller.cpp:1243)
    case SHC_PARAM_STEP_DEPTH: p.step_depth = value; break;              // the proactive step-plane target (:1099)
    case SHC_PARAM_STANCE_SPAN_MODIFIER: p.stance_span_modifier = value; e->span_dirty = true; break; // calculateStanceSpanChange (:966), applied at the next stop / swing start
    case SHC_PARAM_VIRTUAL_MASS:
      if (!(value > 0.0)) return fail(SHC_ERR_INVALID_ARG, "virtual_mass must be positive");
      p.virtual_mass = value;
      break;
    case SHC_PARAM_VIRTUAL_STIFFNESS:
      if (!(value > 0.0)) return fail(SHC_ERR_INVALID_ARG, "virtual_stiffness must be positive");
      p.virtual_stiffness = value;
      break;
    case SHC_PARAM_VIRTUAL_DAMPING: p.virtual_damping_ratio = value; break;
    case SHC_PARAM_FORCE_GAIN: p.force_gain = value; break;              // admittance input (admittance_controller.cpp:32), tip-force estimate (model.cpp:705), LegState tip force
    default: return fail(SHC_ERR_INVALID_ARG, "unknown adjustable parameter (SHC_PARAM_*)");
  }
  adjust_bump(e);
  // The eight parameters the control cycle reads as they are (params_.*.current_value): a new launch-uniform block, in force from the next cycle; no table is
  // regenerated and no state is touched.
  // ... except where the POSING part of the loop reads them (updateStiffness / updateAdmittance run before runningState, state_controller.cpp:170-180): the
  // virtual spring's constants, the force gain as the admittance input scales it and the swing height as the dynamic-stiffness reference divides by it stay
  // what they were for the posing part of the next cycle (the tip-force estimate and the stepper of that same cycle use the new values), then follow.
  if (which == SHC_PARAM_SWING_HEIGHT || which == SHC_PARAM_VIRTUAL_MASS || which == SHC_PARAM_VIRTUAL_STIFFNESS || which == SHC_PARAM_VIRTUAL_DAMPING ||
      which == SHC_PARAM_FORCE_GAIN) {
    if (!e->adjust.params_held) e->adjust.held = old; // (the values the last cycle's posing part ran on)
    e->adjust.params_held = true;
  }
  rebuild_cycle_params(e);
  return upload_consts(e);
}

#endif
