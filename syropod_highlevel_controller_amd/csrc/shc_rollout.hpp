// shc_rollout.hpp — rollout tensors: the two dense-tensor ends of shc_engine_step_k.  shc_engine_step_k_actions takes the inputs of K cycles from
// one dense [K][n][A] array of float64 or float32, shc_engine_get_step_k_observations hands the joints of a range of cycles back as one dense
// [cycles][n][D] array.  Included by shc_engine.hip behind shc_actions.hpp (uses the row pattern of shc_rows.hpp, the specs and checks of
// shc_observe.hpp / shc_actions.hpp, the group table, the K-cycle rules and the K-deep staging plan of shc_inputs.hpp, load_leg_fields of shc_leg_msgs.hpp, resident_fit and the output ring of shc_resident.hpp and the
// entry-point macros).  The fleet forms (shc_fleet_rollout.hpp) launch the same kernels with a part's caller ids as the row table.
//
// Neither end touches the batch kernel.  shc_engine_step_k reads up to six K-deep float64 arrays, each dense on its own:
//   STAGE   one launch converts the selected columns of every cycle's rows to double and stores them into the engine's own K-deep arrays
//           ([K][n][2], [K][n], [K][n][4], [K][n][3], [K][n][L][3], [K][n][L][NJ]); shc_engine_step_k then runs on those, unchanged - the batch
//           kernel or the serial form, a pending adjusted parameter's first cycle, touchdown detection, the first-effort switch, the split halves,
//           the normalisation of the quaternion are all its own.  Nothing is computed here but static_cast<double>.
//   JOINTS  one launch reads q / qd of the requested slots of the output ring where they lie (the leg state's own planes: leg_state_index) and
//           writes whole rows of the caller's array.  (Its TIPS instance serves the rollout kinematics of shc_rollout_kin.hpp, included behind this file.)
// The cycle is the second grid dimension (blockIdx.y): wave-uniform, built from block indices and kernel arguments only.
//
// The staged arrays belong to the engine: allocated by the first call that needs them, grown (never shrunk) by a call that needs more, freed with
// the engine.  The launch reads them - on the two half streams when the batch steps split, which only a join orders behind the engine's stream.
// So before a call overwrites them, an engine with split launches in flight is joined (join_side: events, no host wait); before they are freed
// to grow, the engine is joined and its stream drained, as step_k_out_ring does for the ring.  The caller's array is read by the stage kernel
// alone, on the engine's stream.
#pragma once

constexpr int kRolloutRobotGroups = SHC_ACT_POSE_TRANSLATION_VELOCITY; // the per-robot groups a K-cycle launch carries come first (shc_inputs.hpp)

// The stage kernel's view of a call
struct RolloutStageArgs : ActArgs {
  int64_t cycle_stride;  // elements between the rows of consecutive cycles
  int64_t n;             // robots of the engine: the staged arrays are [K][n][..]
  double *dst[BND_COUNT]; // the staged arrays by BND_* (unselected: NULL, never read)
};

// The geometry and the tile of shc_rows.hpp, copy-in, as actions_kernel: block (g, k) brings the rows of robot group g at cycle k into the tile
// with consecutive lanes on consecutive elements - rows at in + k * cycle_stride + row * row_stride, row = ids[robot] or the robot's own index -
// and lane (robot, leg) stores its tip-force and joint-effort columns, converted, into the staged arrays; the robot's lane g mod L stores robot
// group g.  The staged arrays are dense per robot, and the lanes of a wavefront are consecutive (robot, leg) pairs: a wavefront's stores of one
// array are one contiguous run.  Unselected fields are scalar branches on the mask.  The tile is that of actions_kernel.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void rollout_stage_kernel(const T *__restrict__ in, const RolloutStageArgs a, const int64_t *__restrict__ ids) {
  const RowGroup<L> rg(0, a.n);
  const int64_t k = blockIdx.y;
  T *tile = row_tile<T>();

  row_tile_in(tile, in + k * a.cycle_stride, rg, a, ids, 0);
  __syncthreads();
  if (!rg.live) return;

  const T *row = tile + rg.gi * a.pitch;
  const int leg = rg.leg;
  const int64_t at = k * a.n + rg.rob; // the robot's entry of a [K][n] array
  auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
  if (sel(SHC_ACT_TIP_FORCE)) {
    const T *s = row + a.col[SHC_ACT_TIP_FORCE] + leg * 3;
    double *d = a.dst[BND_FORCE] + (at * L + leg) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = static_cast<double>(s[c]);
  }
  if (sel(SHC_ACT_JOINT_EFFORT)) { // all NJ entries of every leg: a shorter leg's surplus joints hold what the caller put there
    const T *s = row + a.col[SHC_ACT_JOINT_EFFORT] + leg * a.dof;
    double *d = a.dst[BND_EFFORT] + (at * L + leg) * NJ;
#pragma unroll
    for (int j = 0; j < NJ; ++j) d[j] = static_cast<double>(s[j]);
  }
  if (a.mask & ((1u << kRolloutRobotGroups) - 1u)) {
#pragma unroll
    for (int g = 0; g < kRolloutRobotGroups; ++g) {
      if (g % L != leg || !sel(g)) continue;
      const T *s = row + a.col[g];
      double *d = a.dst[input_group(g).bound] + at * act_robot_width(g);
#pragma unroll
      for (int c = 0; c < act_robot_width(g); ++c) d[c] = static_cast<double>(s[c]); // (the quaternion as it is: the engine normalises)
    }
  }
}

// The joints kernel's view of a call: the columns of q, qd and - for shc_engine_get_step_k_kinematics (shc_rollout_kin.hpp) - model_tip
constexpr int kRolloutObsFields = SHC_OBS_MODEL_TIP + 1;
struct RolloutJointArgs : RowArgs<kRolloutObsFields> {
  int32_t dof;          // columns per leg of q / qd
  int64_t cycle_stride; // elements between the rows of consecutive cycles
  int64_t n, n_slots;
};
static_assert(SHC_OBS_Q == 0 && SHC_OBS_QD == 1, "q and qd are the first two observation fields");

// The geometry and the tile of shc_rows.hpp, copy-out, as observe_kernel: `ring` is the slot of the first requested cycle, block (g, k) reads
// the joints of robot group g in slot k - NJ planes of n_slots double2, Q and QD at the leg state's own addresses (leg_state_index: the lane's
// slot is slot_of(robot, leg)), read as whole 16-byte planes - and builds the rows in the tile, filled with `pad` first where the row geometry
// is larger than the robot; the rows leave with consecutive lanes on consecutive elements for out + k * cycle_stride.  SHC_OBS_MODEL_TIP - only
// shc_engine_get_step_k_kinematics lets it through - is derived_model_tip on the q just read, as in observe_kernel.  FK costs 102 - 154 VGPRs
// against the 20 - 24 of the copy, so it is an instance of its own (TIPS) that the host picks by the mask: a spec without model_tip runs the
// kernel it ran before, at 8 waves per SIMD.
template <int L, int NJ, class T, bool TIPS>
__global__ __launch_bounds__(64) void rollout_joints_kernel(T *__restrict__ out, const double2 *__restrict__ ring, const SharedConsts<L, NJ> *__restrict__ gc,
                                                            const RolloutJointArgs o, const int64_t *__restrict__ ids) {
  using FD = Fields<NJ>;
  static_assert(FD::Q == 0 && FD::QD == NJ, "a ring slot holds the planes of Q and QD");
  const RowGroup<L> rg(0, o.n);
  const int64_t k = blockIdx.y;
  T *tile = row_tile<T>();

  row_tile_pad(tile, rg, o);
  if (rg.live) {
    T *row = tile + rg.gi * o.pitch;
    double v[2 * NJ];
    load_leg_fields<FD::Q, 2 * NJ>(ring + k * NJ * o.n_slots, o.n_slots, rg.slot, v);
    if (o.mask >> SHC_OBS_Q & 1u) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) row[o.col[SHC_OBS_Q] + rg.leg * o.dof + j] = static_cast<T>(v[j]);
    }
    if (o.mask >> SHC_OBS_QD & 1u) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) row[o.col[SHC_OBS_QD] + rg.leg * o.dof + j] = static_cast<T>(v[NJ + j]);
    }
    if constexpr (TIPS) {
      double q[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) q[j] = v[j];
      const V3 tip = derived_model_tip<NJ>(gc->leg[rg.leg], q);
      T *d = row + o.col[SHC_OBS_MODEL_TIP] + rg.leg * 3;
      d[0] = static_cast<T>(tip.x), d[1] = static_cast<T>(tip.y), d[2] = static_cast<T>(tip.z);
    }
  }
  __syncthreads();
  row_tile_out(out + k * o.cycle_stride, tile, rg, o, ids, 0);
}

// ---- host side
// Where the groups of a spec lie in K-deep staging for an engine (input_plan of shc_inputs.hpp: shc_fleet_step_k's, too); pose groups are never staged
static InputPlan rollout_plan(const shc_engine *e, const RowLayout &lay, int K) { return input_plan(lay.mask & ~kPoseInputs, e->n, e->L, e->NJ, K); }

// What is wrong with a call whoever makes it: `n` rows per cycle in the caller's array
static int rollout_stride_check(const char *who, int64_t n, int64_t row_stride, int64_t cycle_stride) {
  if (cycle_stride != 0 && cycle_stride < n * row_stride) return fail(SHC_ERR_INVALID_ARG, std::string(who) + ": cycle_stride is non-zero and below n x the row stride");
  return SHC_OK;
}
static int rollout_actions_call_check(const char *who, const shc_act_spec *spec, const RowLayout &lay, int K, int64_t n, int64_t cycle_stride) {
  int rc = k_launch_cycles_check(who, K);
  if (rc != SHC_OK) return rc;
  if ((rc = rollout_stride_check(who, n, row_stride_of(spec, lay), cycle_stride)) != SHC_OK) return rc;
  if ((rc = input_pairs_check(lay.mask, kAllInputs & ~kPoseInputs, "given")) != SHC_OK) return rc;
  return k_launch_pose_check(who, lay.mask);
}
// ... and what an engine refuses of it: everything its shc_engine_step_k would refuse, asked before anything is staged
static int rollout_actions_engine_check(const char *who, const shc_engine *e, const shc_act_spec *spec, const RowLayout &lay, int K) {
  const int rc = actions_check(e, spec);
  return rc != SHC_OK ? rc : k_launch_engine_check(e, who, K, rollout_plan(e, lay, K).doubles);
}

// The stage launch on the engine's stream: the K x n rows of `actions` (row = ids[robot], a device table, or the robot's own index) into the
// K-deep arrays at `stage`, and `staged`, the shc_cycle_inputs over them.  The caller has checked everything, made room and joined split steps.
static int rollout_stage_launch(shc_engine *e, const shc_act_spec *spec, const RowLayout &lay, const void *actions, int64_t row_stride, int64_t cycle_stride,
                                const int64_t *ids, int K, double *stage, shc_cycle_inputs &staged) {
  const InputPlan plan = rollout_plan(e, lay, K);
  RolloutStageArgs a{};
  row_args(a, lay, spec->dtype, row_stride, false, 0.0);
  a.dof = spec->dof;
  a.cycle_stride = cycle_stride, a.n = e->n;
  for (int g = 0; g < kInputGroups; ++g)
    if (plan.at[g] >= 0) a.dst[input_group(g).bound] = stage + plan.at[g];
  const dim3 grid(row_grid(e->L, 0, e->n), unsigned(K));
  const size_t lds = row_tile_bytes(e->L, a.pitch, spec->dtype);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    if (spec->dtype == SHC_OBS_F32)
      rollout_stage_kernel<L, NJ, float><<<grid, dim3(64), lds, e->stream>>>(static_cast<const float *>(actions), a, ids);
    else
      rollout_stage_kernel<L, NJ, double><<<grid, dim3(64), lds, e->stream>>>(static_cast<const double *>(actions), a, ids);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  staged = input_plan_arrays(plan, stage);
  return SHC_OK;
}

// Room for `need` bytes of staging (the engine's own, or a fleet part's): what is there is kept when it is large enough; else the engine is joined
// and its stream drained - a launch may still be reading the arrays - before they are released and allocated again.
static int rollout_stage_room(shc_engine *e, char *&stage, size_t &stage_bytes, size_t need) {
  if (need <= stage_bytes) return SHC_OK;
  if (stage) {
    const int rc = join_side(e);
    if (rc != SHC_OK) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(stage));
    stage = nullptr, stage_bytes = 0;
  }
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&stage), need));
  stage_bytes = need;
  return SHC_OK;
}

extern "C" int shc_engine_step_k_actions(shc_engine *e, int n_cycles, const shc_act_spec *spec, const void *actions, int64_t cycle_stride) {
  SHC_ENTER(e);
  if (!spec || !actions) return fail(SHC_ERR_INVALID_ARG, "spec or actions is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ActRows>(spec, lay)) return bad;
  int rc = row_aligned(actions, spec->dtype, "actions");
  if (rc != SHC_OK) return rc;
  const char *who = "shc_engine_step_k_actions";
  if ((rc = rollout_actions_call_check(who, spec, lay, n_cycles, e->n, cycle_stride)) != SHC_OK) return rc;
  if ((rc = rollout_actions_engine_check(who, e, spec, lay, n_cycles)) != SHC_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if ((rc = rollout_stage_room(e, e->k_in, e->k_in_bytes, size_t(rollout_plan(e, lay, n_cycles).doubles) * 8)) != SHC_OK) return rc;
  // the halves of an earlier split launch may still be reading the arrays this call is about to overwrite: the engine's stream follows them first
  if (e->side_busy && (rc = join_side(e)) != SHC_OK) return rc;
  const int64_t stride = row_stride_of(spec, lay);
  shc_cycle_inputs staged;
  if ((rc = rollout_stage_launch(e, spec, lay, actions, stride, cycle_stride ? cycle_stride : e->n * stride, nullptr, n_cycles, reinterpret_cast<double *>(e->k_in), staged)) != SHC_OK)
    return rc;
  return shc_engine_step_k(e, n_cycles, &staged);
}

// What an engine refuses of an observation spec that is valid on its own, for the joints of the ring: `readable` is kRingJoints for
// shc_engine_get_step_k_observations, kRingKinematics - what is a pure function of those joints as well - for shc_engine_get_step_k_kinematics
constexpr uint32_t kRingJoints = 1u << SHC_OBS_Q | 1u << SHC_OBS_QD, kRingKinematics = kRingJoints | 1u << SHC_OBS_MODEL_TIP;
static int rollout_joints_check(const shc_engine *e, const shc_obs_spec *spec, const RowLayout &lay, uint32_t readable = kRingJoints) {
  if (lay.mask & ~readable)
    return fail(SHC_ERR_UNSUPPORTED, readable == kRingJoints ? "an output ring (K-cycle launches, resident loop) holds joints: SHC_OBS_Q and SHC_OBS_QD only"
                                                             : "an output ring (K-cycle launches, resident loop) holds joints: SHC_OBS_Q, SHC_OBS_QD and SHC_OBS_MODEL_TIP = FK(q) only");
  return observe_check(e, spec, lay);
}
// cycles [first, first + count) of the K of the latest launch
static int rollout_range_check(const char *who, int K, int first_cycle, int n_cycles) {
  if (K < 1 || first_cycle < 0 || n_cycles < 1 || first_cycle > K - n_cycles)
    return fail(SHC_ERR_INVALID_ARG, std::string(who) + ": cycles [first_cycle, first_cycle + n_cycles) of the K of the latest K-cycle launch");
  return SHC_OK;
}
// The joints launch on the engine's stream: every robot's q / qd of the n_cycles slots from `ring` on - NJ planes of n_slots double2 each, the
// layout of the K-cycle launches' output ring and of a slot of the resident loop's - into rows ids[robot] (a device table) or robot of
// out + cycle * cycle_stride.  The caller has checked everything.
static int rollout_joints_launch_at(shc_engine *e, const shc_obs_spec *spec, const RowLayout &lay, void *out, int64_t row_stride, int64_t cycle_stride,
                                    const int64_t *ids, const double2 *ring, int n_cycles) {
  RolloutJointArgs o{};
  row_args(o, lay, spec->dtype, row_stride, spec->legs > e->L || spec->dof > e->NJ, spec->pad);
  o.dof = spec->dof;
  o.cycle_stride = cycle_stride, o.n = e->n, o.n_slots = e->n_slots;
  const dim3 grid(row_grid(e->L, 0, e->n), unsigned(n_cycles));
  const size_t lds = row_tile_bytes(e->L, o.pitch, spec->dtype);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    const SharedConsts<L, NJ> *gc = (const SharedConsts<L, NJ> *)e->d_consts;
    auto launch = [&](auto *rows, auto tips) {
      using T = std::remove_pointer_t<decltype(rows)>;
      rollout_joints_kernel<L, NJ, T, decltype(tips)::value><<<grid, dim3(64), lds, e->stream>>>(rows, ring, gc, o, ids);
    };
    auto typed = [&](auto tips) { spec->dtype == SHC_OBS_F32 ? launch(static_cast<float *>(out), tips) : launch(static_cast<double *>(out), tips); };
    (o.mask >> SHC_OBS_MODEL_TIP & 1u) ? typed(std::true_type{}) : typed(std::false_type{});
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

// ... of ring slots [first_cycle, first_cycle + n_cycles) of the latest K-cycle launch.  The caller has joined split steps, too.
static int rollout_joints_launch(shc_engine *e, const shc_obs_spec *spec, const RowLayout &lay, void *out, int64_t row_stride, int64_t cycle_stride,
                                 const int64_t *ids, int first_cycle, int n_cycles) {
  const double2 *ring = reinterpret_cast<const double2 *>(e->k_out) + int64_t(first_cycle) * e->NJ * e->n_slots;
  return rollout_joints_launch_at(e, spec, lay, out, row_stride, cycle_stride, ids, ring, n_cycles);
}

// The read of the ring as rows, for the two entry points that differ in the fields they let through (`readable`)
static int rollout_read(shc_engine *e, const char *who, uint32_t readable, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  SHC_ENTER(e);
  if (!spec || !out) return fail(SHC_ERR_INVALID_ARG, "spec or out is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ObsRows>(spec, lay)) return bad;
  int rc = rollout_joints_check(e, spec, lay, readable);
  if (rc != SHC_OK) return rc;
  if ((rc = row_aligned(out, spec->dtype, "out")) != SHC_OK) return rc;
  if ((rc = rollout_range_check(who, e->k_out ? e->k_out_cycles : 0, first_cycle, n_cycles)) != SHC_OK) return rc;
  const int64_t stride = row_stride_of(spec, lay);
  if ((rc = rollout_stride_check(who, e->n, stride, cycle_stride)) != SHC_OK) return rc;
  if ((rc = join_side(e)) != SHC_OK) return rc; // split launches: the engine's stream follows both halves before it reads their ring
  HIP_TRY(hipSetDevice(e->device));
  return rollout_joints_launch(e, spec, lay, out, stride, cycle_stride ? cycle_stride : e->n * stride, nullptr, first_cycle, n_cycles);
}
extern "C" int shc_engine_get_step_k_observations(shc_engine *e, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  return rollout_read(e, "shc_engine_get_step_k_observations", kRingJoints, first_cycle, n_cycles, spec, out, cycle_stride);
}
