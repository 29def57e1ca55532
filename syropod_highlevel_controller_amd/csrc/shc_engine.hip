// shc_engine.hip — libshc_batch.so: C ABI (include/shc_batch.h), host init chain and HIP kernels (gfx950).
//
// Product code.  Nothing here links, includes or calls anything under oracle/.  There is no CPU fallback for
// the cycle: without a HIP device shc_engine_create fails with SHC_ERR_NO_DEVICE.
#include "../../include/shc_batch.h"
#include "shc_cycle.hpp"
#include "shc_cycle_launch.hpp"
#include "shc_host_init.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

using namespace shc;

#ifndef SHC_WAVES_PER_SIMD
#define SHC_WAVES_PER_SIMD 2
#endif

static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(SHC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// as HIP_TRY, running `cleanup` before the early return (error paths must not leak device buffers)
#define HIP_TRY_OR(expr, cleanup)                                                                       \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) {                                                                             \
      cleanup;                                                                                          \
      return fail(SHC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                     \
    }                                                                                                   \
  } while (0)

// ================================================================================================= kernels

// (the fused cycle kernels live in shc_cycle_kernel.hpp / shc_cycle_inst.hip: one translation unit per morphology)

__global__ void shc_plane_copy_kernel(const double2 *__restrict__ src, double2 *__restrict__ dst, int64_t n_pairs) {
  int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n_pairs) dst[i] = src[i];
}

// ---- layout conversion kernels (C ABI instance-major arrays <-> SoA fields)
// element index of field f of robot r in the AoSoA robot tiles ([wave][field][robots-per-wave])
__device__ __forceinline__ int64_t rob_index(int64_t r, int f, int rpw, int nf) { return ((r / rpw) * nf + f) * rpw + (r % rpw); }
__device__ __forceinline__ int64_t slot_of(int64_t rob, int leg, int L) {
  int rpw = 64 / L;
  int64_t w = rob / rpw;
  int gi = int(rob - w * rpw);
  return w * 64 + gi * L + leg;
}

#include "shc_leg_api.hpp"  // per-leg Leg methods, batched
#include "shc_sequence.hpp" // executeSequence / stepToNewStance: per-robot state machines over the per-leg primitives

// AoS [n][L][K] -> leg fields f0..f0+K-1
__global__ void scatter_leg_kernel(const double *src, double *legd, int64_t n_slots, int64_t n, int L, int K, int f0, int64_t r0 = 0) {
  int64_t t = r0 * L + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; // instances [r0, n)
  if (t >= n * L) return;
  int64_t rob = t / L;
  int leg = int(t - rob * L);
  int64_t slot = slot_of(rob, leg, L);
  for (int k = 0; k < K; ++k) legd[leg_field_index(f0 + k, slot, n_slots)] = src[t * K + k];
}
// element index of leg field f of (robot, leg) in the leg state planes - and in a slot of the step_k output ring, which keeps the planes of Q and QD in
// the same layout: the one address both gather_leg_kernel and the fleet's ring place (shc_fleet_step_k.hpp) read joints at
__device__ __forceinline__ int64_t leg_state_index(int f, int64_t rob, int leg, int L, int64_t n_slots) { return leg_field_index(f, slot_of(rob, leg, L), n_slots); }
__global__ void gather_leg_kernel(double *dst, const double *legd, int64_t n_slots, int64_t n, int L, int K, int f0) {
  int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n * L) return;
  int64_t rob = t / L;
  int leg = int(t - rob * L);
  for (int k = 0; k < K; ++k) dst[t * K + k] = legd[leg_state_index(f0 + k, rob, leg, L, n_slots)];
}
// LegState tips derived from the stored state (see store_leg): model tip = FK(q) in the robot frame (Leg::applyFK,
// model.cpp:975), poser tip = Model::current_pose_^-1 * walker tip (PoseController::updateStance, pose_controller.cpp:122-131).
// The three functions are the one implementation: derive_tips_kernel stores what they return, observe_kernel (shc_observe.hpp) uses it in place.
template <int NJ>
__device__ __forceinline__ V3 derived_model_tip(const LegConst<NJ> &lc, const double (&q)[NJ]) {
  Chain<NJ> ch;
  fk_chain<NJ>(lc, q, ch);
  return tip_robot_frame(lc, ch.pe);
}
__device__ __forceinline__ V3 derived_poser_tip(const double (&c)[7], V3 walker_tip) {
  return inverse_transform_vector(Pose{V3{c[0], c[1], c[2]}, Quat{c[3], c[4], c[5], c[6]}}, walker_tip);
}
// keep_marked: the last loop of the marked robots was a plan call under time-dependent posing - their LegPoser tips are state (the
// pose has moved on since the updateStance that produced them, see execute_plan_kernel LOOP_MARK)
__device__ __forceinline__ bool poser_tip_is_derived(const DevState &st, int64_t rob, int derive_poser, int keep_marked) {
  return derive_poser && !(keep_marked && st.manual != nullptr && st.manual[rob].skip_cycle != 0);
}
template <int L, int NJ>
__global__ void derive_tips_kernel(DevState st, const SharedConsts<L, NJ> *gc, int derive_poser, int keep_marked) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= st.n_robots * L) return;
  int64_t rob = t / L;
  int leg = int(t - rob * L);
  int64_t slot = slot_of(rob, leg, L);
  const LegConst<NJ> &lc = gc->leg[leg];
  double q[NJ];
  for (int j = 0; j < NJ; ++j) q[j] = st.legd[leg_field_index(FD::Q + j, slot, st.n_slots)];
  V3 tip = derived_model_tip<NJ>(lc, q);
  st.legd[leg_field_index(FD::MODEL_TIP, slot, st.n_slots)] = tip.x;
  st.legd[leg_field_index(FD::MODEL_TIP + 1, slot, st.n_slots)] = tip.y;
  st.legd[leg_field_index(FD::MODEL_TIP + 2, slot, st.n_slots)] = tip.z;
  if (poser_tip_is_derived(st, rob, derive_poser, keep_marked)) {
    constexpr int rpw = 64 / L;
    double c[7];
    for (int k = 0; k < 7; ++k) c[k] = st.robd[rob_index(rob, R::CPOSE + k, rpw, R::COUNT)];
    V3 w{st.legd[leg_field_index(FD::TIP, slot, st.n_slots)], st.legd[leg_field_index(FD::TIP + 1, slot, st.n_slots)],
         st.legd[leg_field_index(FD::TIP + 2, slot, st.n_slots)]};
    V3 pt = derived_poser_tip(c, w);
    st.legd[leg_field_index(FD::POSER_TIP, slot, st.n_slots)] = pt.x;
    st.legd[leg_field_index(FD::POSER_TIP + 1, slot, st.n_slots)] = pt.y;
    st.legd[leg_field_index(FD::POSER_TIP + 2, slot, st.n_slots)] = pt.z;
  }
}
// odometry_ideal_ is stored as (x, y, qw, qz): expand to the pose layout of the ABI (x, y, z, qw, qx, qy, qz)
__global__ void gather_odometry_kernel(double *dst, const double *robd, int rpw, int64_t n) {
  constexpr int nf = RobotFields::COUNT;
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double *o = dst + r * 7;
  o[0] = robd[rob_index(r, RobotFields::ODOM, rpw, nf)];
  o[1] = robd[rob_index(r, RobotFields::ODOM + 1, rpw, nf)];
  o[2] = 0.0;
  o[3] = robd[rob_index(r, RobotFields::ODOM + 2, rpw, nf)];
  o[4] = 0.0;
  o[5] = 0.0;
  o[6] = robd[rob_index(r, RobotFields::ODOM + 3, rpw, nf)];
}
// leg_status of shc_engine_get_leg_state from the leg word: bits 0-1 the step state, bit 2 the IK failure, the phase from bit 8
__device__ __forceinline__ int leg_status_of(int w) {
  int phase = (w >> LW_PHASE_SHIFT) & LW_PHASE_MASK;
  return (w & 3) | ((w & LW_IKFAIL) ? 4 : 0) | (phase << 8);
}
__global__ void gather_leg_status_kernel(int32_t *dst, const int32_t *legi, int64_t n, int L) {
  int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n * L) return;
  int64_t rob = t / L;
  int leg = int(t - rob * L);
  dst[t] = leg_status_of(legi[slot_of(rob, leg, L)]);
}
// AoS [n][K] -> robot fields

__global__ void scatter_rob_kernel(const double *src, double *robd, int rpw, int64_t n, int K, int f0, int normalize_quat, int64_t r0 = 0) {
  constexpr int nf = RobotFields::COUNT;
  int64_t r = r0 + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; // instances [r0, n)
  if (r >= n) return;
  if (normalize_quat) { // Model::setImuData normalises the orientation (model.h:150)
    Quat q = normalized(Quat{src[r * 4], src[r * 4 + 1], src[r * 4 + 2], src[r * 4 + 3]});
    robd[rob_index(r, f0 + 0, rpw, nf)] = q.w;
    robd[rob_index(r, f0 + 1, rpw, nf)] = q.x;
    robd[rob_index(r, f0 + 2, rpw, nf)] = q.y;
    robd[rob_index(r, f0 + 3, rpw, nf)] = q.z;
    return;
  }
  for (int k = 0; k < K; ++k) robd[rob_index(r, f0 + k, rpw, nf)] = src[r * K + k];
}
__global__ void gather_rob_kernel(double *dst, const double *robd, int rpw, int64_t n, int K, int f0) {
  constexpr int nf = RobotFields::COUNT;
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int k = 0; k < K; ++k) dst[r * K + k] = robd[rob_index(r, f0 + k, rpw, nf)];
}
__global__ void scatter_robi_kernel(const int32_t *src, int32_t *robi, int rpw, int64_t n, int f) {
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r < n) robi[rob_index(r, f, rpw, RobotFields::I_COUNT)] = src[r];
}
__global__ void count_walking_kernel(int32_t *count, const int32_t *robi, int rpw, int64_t n) {
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool walking = r < n && (robi[rob_index(r, RobotFields::I_WORD, rpw, RobotFields::I_COUNT)] & 3) != WS_STOPPED;
  unsigned long long m = __ballot(walking);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, __popcll(m));
}
__global__ void fill_rob_kernel(double *robd, int rpw, int64_t n, int f0, int K, double v) {
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int k = 0; k < K; ++k) robd[rob_index(r, f0 + k, rpw, RobotFields::COUNT)] = v;
}
__global__ void fill_robi_kernel(int32_t *robi, int rpw, int64_t n, int f, int32_t v) {
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r < n) robi[rob_index(r, f, rpw, RobotFields::I_COUNT)] = v;
}
__device__ __forceinline__ int walk_state_of(const int32_t *robi, int64_t r, int rpw) { return robi[rob_index(r, RobotFields::I_WORD, rpw, RobotFields::I_COUNT)] & 3; }
__global__ void gather_walk_state_kernel(int32_t *dst, const int32_t *robi, int rpw, int64_t n) {
  int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n) return;
  dst[r] = walk_state_of(robi, r, rpw);
}
// replicate the post-start-up state of one robot into every slot
__global__ void init_state_kernel(DevState st, const double *leg_template /*[L][nf]*/, const int32_t *legw_template /*[L]*/,
                                  const double *rob_template /*[nrf]*/, const int32_t *robi_template /*[nri]*/, int L, int nf,
                                  int nrf, int nri) {
  int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t n = st.n_robots;
  if (t < n * L) {
    int64_t rob = t / L;
    int leg = int(t - rob * L);
    int64_t slot = slot_of(rob, leg, L);
    for (int f = 0; f < nf; ++f) st.legd[leg_field_index(f, slot, st.n_slots)] = leg_template[leg * nf + f];
    st.legi[slot] = legw_template[leg];
  }
  if (t < n) {
    const int rpw = 64 / L;
    for (int f = 0; f < nrf; ++f) st.robd[rob_index(t, f, rpw, nrf)] = rob_template[f];
    for (int f = 0; f < nri; ++f) st.robi[rob_index(t, f, rpw, nri)] = robi_template[f];
  }
}

// ================================================================================================= engine

constexpr int64_t kPlanePadSlots = 192;

#include "shc_adjust.hpp" // struct PendingAdjust (the operations on it: included again below)
#include "shc_stage.hpp"  // struct StageArena (the per-call scope over it: included again below)

struct shc_engine {
  shc_params params;
  shc_tables tables;
  CycleParams cp;
  int L, NJ;
  int device;
  hipStream_t stream;
  int64_t n, n_waves, n_slots, n_rob_pad;
  int n_leg_fields;
  DevState st;
  void *d_consts;
  double *d_stage;     // staging for host <-> device conversions
  size_t stage_bytes;
  StageArena stage;    // ... handed out per call (shc_stage.hpp: HostCall)
  uint32_t features;
  uint32_t rt_flags; // RT_* facts passed to every launch
  int starting_up, startup_calls; // shc_engine_begin_direct_startup .. shc_engine_direct_startup
  SeqRobotState *d_seq;           // start-up / shut-down sequence state (shc_sequence.hpp), allocated by the first sequence call
  int pack_step, executing_transition, transition_calls; // PoseController::pack_step_ / executing_transition_ (pose_controller.h:294, :298)
  bool planner_mode = false;            // StateController::planner_mode_ (state_controller.h:337)
  bool plan_poser_tips_current = false; // no control cycle has run since the last shc_engine_execute_plan (SeqRobotState::poser_tip_from_plan holds)
  double *d_span = nullptr;             // SpanTable (rough terrain mode with a stance span modifier), rebuilt with the tables
  int half_steps = 0;                   // CycleLaunch::half_steps (development switch SHC_ROT_SPLIT = 0 / 1: never / always; unset: by launch size)
  bool span_dirty = true;
  PendingAdjust adjust{};               // a shc_engine_adjust_parameter that waits for its loop (shc_adjust.hpp)
  bool fresh_pose_controller = false;   // init_state for shc_engine_begin_sequence_startup: no direct start-up has run, the auto posers have not been called yet
  struct Resident *res = nullptr;       // resident mode (shc_resident.hpp)
  const double *bound_inputs[kBoundSets][BND_COUNT] = {}; // shc_engine_resident_bind_inputs: the caller's device arrays for direct posts
  // Large batches: a step is launched as two halves on two streams with no join between steps (see shc_engine_step).
  hipStream_t half_stream[2] = {nullptr, nullptr}; // the device's pair of split streams (split_streams()), once this engine has used them
  hipEvent_t ev_main = nullptr, ev_half[2] = {nullptr, nullptr};
  hipEvent_t ev_in[2] = {nullptr, nullptr}; // the half streams have read a device-resident input array (the engine's stream is ordered after them)
  double *k_out = nullptr;              // shc_engine_step_k: q / qd of each of the K cycles of the latest launch, [K][dof planes][n_slots] double2
  size_t k_out_bytes = 0;
  int k_out_cycles = 0;
  char *k_in = nullptr;                 // shc_engine_step_k_actions: the K-deep float64 input arrays staged from the caller's tensor (shc_rollout.hpp); grows on demand, kept
  size_t k_in_bytes = 0;
  bool side_busy = false;               // launches are outstanding on the split streams that the engine's stream has not been ordered after
  bool main_dirty = true;               // work other than steps was enqueued on the engine's stream since the last split step
  struct shc_checkpoint *checkpoints = nullptr; // the registry of this engine's device checkpoints (shc_checkpoint.hpp): released with the engine
  void *d_health = nullptr;             // shc_engine_scan_health: per-wavefront selection masks and the levels of their counts (shc_health.hpp), allocated by the first scan
};
struct Resident;
static bool resident_active(const shc_engine *e);
static void resident_shutdown(shc_engine *e); // stop a running resident loop and free its buffers (shc_engine_destroy)
static void release_checkpoints(shc_engine *e); // free the device arrays of the engine's checkpoints and orphan their handles (shc_engine_destroy)
// While the resident kernel owns the engine's stream and state, every other entry point that would touch them is refused.
static int join_side(shc_engine *e);
static void rebuild_cycle_params(shc_engine *e);
#include "shc_stage.hpp" // HostCall: the staging scope of one entry point
// Every entry point begins with one of these, before it does anything with `e`: a NULL engine is refused, and so is an engine in resident mode ...
#define SHC_ENTER(e)                                                                                                           \
  do {                                                                                                                         \
    if (!(e)) return fail(SHC_ERR_INVALID_ARG, "engine is NULL");                                                              \
    if (resident_active(e))                                                                                                    \
      return fail(SHC_ERR_BUSY, "the engine is in resident mode: only shc_engine_resident_* calls are valid until shc_engine_resident_end"); \
  } while (0)
// ... and whatever the entry point enqueues on the engine's stream is ordered after the second halves of earlier split steps - unless its input can ride
// the split streams (RIDES: split_inputs(), a join drains both halves)
#define SHC_ENTER_JOINED_UNLESS(e, RIDES)                                                                                      \
  do {                                                                                                                         \
    SHC_ENTER(e);                                                                                                              \
    if (!(RIDES)) {                                                                                                            \
      const int rc_join_ = join_side(e);                                                                                       \
      if (rc_join_ != SHC_OK) return rc_join_;                                                                                 \
    }                                                                                                                          \
  } while (0)
#define SHC_ENTER_JOINED(e) SHC_ENTER_JOINED_UNLESS(e, false)

// The kernel specialisation of the engine's morphology: fn(std::integral_constant<int, legs>, std::integral_constant<int, joints>) -> int runs for the
// entry of SHC_FOR_EACH_MORPHOLOGY (shc_cycle_launch.hpp: the one list of the morphologies this build has kernels for) that matches.
static int no_specialisation() { return fail(SHC_ERR_UNSUPPORTED, "no kernel specialisation for this (legs, dof)"); }
template <class Fn>
static int dispatch_morphology(const shc_engine *e, Fn &&fn) {
#define SHC_MORPHOLOGY_CASE(L_, NJ_) \
  if (e->L == L_ && e->NJ == NJ_) return fn(std::integral_constant<int, L_>{}, std::integral_constant<int, NJ_>{});
  SHC_FOR_EACH_MORPHOLOGY(SHC_MORPHOLOGY_CASE)
#undef SHC_MORPHOLOGY_CASE
  return no_specialisation();
}
// ... and of the leg count alone: fn(std::integral_constant<int, legs>)
template <class Fn>
static int dispatch_legs(const shc_engine *e, Fn &&fn) {
  switch (e->L) {
  case 3: return fn(std::integral_constant<int, 3>{});
  case 4: return fn(std::integral_constant<int, 4>{});
  case 5: return fn(std::integral_constant<int, 5>{});
  case 6: return fn(std::integral_constant<int, 6>{});
  case 7: return fn(std::integral_constant<int, 7>{});
  case 8: return fn(std::integral_constant<int, 8>{});
  default: return no_specialisation();
  }
}
// Everything a launch of the cycle kernel takes from the engine as it is; the caller names what is its own (grid, block, stream, cycles, loop form)
static CycleLaunch cycle_launch(const shc_engine *e) {
  CycleLaunch a{};
  a.st = e->st, a.consts = e->d_consts, a.cp = &e->cp, a.rt_flags = e->rt_flags, a.stream = e->stream;
  a.generic = (e->features & SHC_FEAT_GENERIC_KERNEL) != 0;
  return a;
}
// ... and the launch, on the engine's morphology (shc_cycle_inst.hip picks the specialisation: shc_cycle_select.hpp)
static int launch_cycle_for(const shc_engine *e, const CycleLaunch &a) {
#define SHC_LAUNCHER_CASE(L_, NJ_) \
  if (e->L == L_ && e->NJ == NJ_)  \
    return shc_launch_cycle_##L_##_##NJ_(a) ? SHC_OK : fail(SHC_ERR_UNSUPPORTED, "the kernel selection named a specialisation this build has no kernel for");
  SHC_FOR_EACH_MORPHOLOGY(SHC_LAUNCHER_CASE)
#undef SHC_LAUNCHER_CASE
  return no_specialisation();
}
// ... and of the joint count alone (validate_params: 3 .. 5): fn(std::integral_constant<int, joints>)
template <class Fn>
static auto dispatch_nj(int NJ, Fn &&fn) {
  switch (NJ) {
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    default: return fn(std::integral_constant<int, 5>{});
  }
}
#define LEG_FIELD(e, NAME) dispatch_nj((e)->NJ, [](auto nj) { return int(Fields<decltype(nj)::value>::NAME); })

template <int L, int NJ>
static void build_shared_consts(const shc_params &p, const shc_tables &t, const CycleParams &cp, SharedConsts<L, NJ> &c) {
  memset(&c, 0, sizeof c);
  c.P = cp;
  const shc_step_cycle &step = t.step;
  for (int l = 0; l < L; ++l) {
    hostinit::fill_leg_const<NJ>(p, l, c.leg[l]);
    LegConst<NJ> &lc = c.leg[l];
    lc.neg_ratio = p.negation_transition_ratio[l];
    { // calculateStanceSpanChange (walk_controller.cpp:949-980): workspace.size() == 1 -> radius = workspace.at(0.0).at(bearing)
      double m = p.stance_span_modifier;
      const bool positive_y = p.stance_position[l][1] > 0.0;
      const int bearing = (positive_y ^ (m > 0.0)) ? 270 : 90;
      m *= positive_y ? 1.0 : -1.0;
      lc.span_shift = t.workspace_radius[l][bearing / 45] * m;
    }
    lc.phase_offset = t.phase_offset[l];
    int ns = p.pose_negation_phase_starts[l] * t.pose_normaliser, ne = p.pose_negation_phase_ends[l] * t.pose_normaliser;
    if (ns == 0) ns = t.pose_phase_length; // pose_controller.cpp:1723-1730
    if (ne == 0) ne = t.pose_phase_length;
    lc.neg_start = ns;
    lc.neg_end = ne;
    int msp = mod_i(step.stance_end - lc.phase_offset, step.period); // walk_controller.cpp:1026-1031
    if (step.stance_end == lc.phase_offset) msp = step.period;
    lc.first_stance_period = msp;
    lc.first_stance_iterations = int((double(msp) / step.period) / (step.frequency * p.time_delta));
    lc.first_stance_dt = 1.0 / lc.first_stance_iterations;
    lc.first_stride_scaler = double(msp) / double(step.stance_period);
    lc.starts_in_swing = (lc.phase_offset > step.swing_start && lc.phase_offset < step.swing_end) ? 1 : 0;
  }
  for (int it = 0; it < cp.swing_c_count; ++it) { // LegStepper::updatePhase progress (walk_controller.cpp:878-880) -> control input
    double sp = clampd(double(it + 1) / double(step.swing_end - step.swing_start), 0.0, 1.0) * cp.swing_progress_scaler;
    c.swing_c[it] = smooth_step(sp);
  }
  for (int b = 0; b < 9; ++b) {
    c.limit[b][0] = t.max_linear_speed[b];
    c.limit[b][1] = t.max_angular_speed[b];
    c.limit[b][2] = t.max_linear_acceleration[b];
    c.limit[b][3] = t.max_angular_acceleration[b];
  }
}

// Parameters::leg_DOF is per leg (parameters_and_states.h:298): the engine runs a robot on the kernels of its LONGEST leg; a shorter leg
// is padded behind its tip with locked zero-length joints (LegConst::jactive, hostinit::fill_leg_const), which leaves every formula of
// that leg as the reference evaluates it for its own joint count (the padded Jacobian columns are zero, their cost terms too).
static int max_dof(const shc_params &p) {
  int nj = 0;
  for (int l = 0; l < p.leg_count && l < SHC_MAX_LEGS; ++l) nj = p.leg_dof[l] > nj ? p.leg_dof[l] : nj;
  return nj;
}
static bool mixed_dof(const shc_params &p) {
  for (int l = 1; l < p.leg_count; ++l)
    if (p.leg_dof[l] != p.leg_dof[0]) return true;
  return false;
}
// Tip rotations are part of the state: legs of more than 3 joints with gravity-aligned tips / in rough terrain mode, or 3-joint legs that
// joint_control leg manipulation hands their FK tip pose to (walk_controller.cpp:677-690).
static int rotations_tracked(const shc_engine *e) { return (e->cp.gravity_aligned || e->cp.joint_control == 2) ? 1 : 0; }
// ... and the parameter block the engine keeps has neutral entries for the padding (joint arrays of the ABI are [legs][longest leg's DOF]:
// the padded joints read 0 and ignore what is written to them)
static shc_params normalised_params(const shc_params &in) {
  shc_params p = in;
  const int nj = max_dof(p);
  for (int l = 0; l < p.leg_count; ++l)
    for (int j = p.leg_dof[l]; j < nj; ++j) {
      p.joint[l][j] = shc_joint_params{0.0, 0.0, 0.0, 0.0, 1.0};
      p.link[l][j + 1] = shc_link_params{0.0, 0.0, 0.0, 0.0};
    }
  return p;
}
static void set_step_cycle(CycleParams &c, const shc_step_cycle &s) { // the phase boundaries of a step cycle
  c.period = s.period, c.swing_period = s.swing_period, c.stance_period = s.stance_period;
  c.stance_end = s.stance_end, c.swing_start = s.swing_start, c.swing_end = s.swing_end, c.stance_start = s.stance_start;
}
static void build_cycle_params(const shc_params &p, const shc_tables &t, uint32_t features, unsigned rt_flags, CycleParams &c) {
  memset(&c, 0, sizeof c);
  const shc_step_cycle &s = t.step;
  c.dt = p.time_delta;
  set_step_cycle(c, s);
  int swing_iterations = int((double(s.swing_period) / s.period) / (s.frequency * p.time_delta)); // walk_controller.cpp:1035
  swing_iterations = round_to_even_int(swing_iterations);
  c.swing_iterations = swing_iterations;
  c.swing_delta_t = 1.0 / (swing_iterations / 2.0);
  c.inv_dt = 1.0 / p.time_delta;
  c.dt_over_swing_dt = p.time_delta / c.swing_delta_t;
  c.stance_iterations = int((double(s.stance_period) / s.period) / (s.frequency * p.time_delta)); // :1040
  c.stance_dt = 1.0 / c.stance_iterations;
  double on_ground_ratio = double(s.stance_period) / s.period;                                    // :940
  c.stride_scale = on_ground_ratio / s.frequency;
  c.swing_height = p.swing_height;
  c.swing_width = p.swing_width;
  c.body_clearance = p.body_clearance;
  c.swing_progress_scaler = fmax(1.0, double(p.swing_phase) / p.phase_offset); // pose_controller.cpp:1103
  c.swing_c_count = (s.swing_end - s.swing_start) <= kSwingTable ? (s.swing_end - s.swing_start) : 0;
  c.swing_c_valid = 0;
  for (int it = 0; it < c.swing_c_count; ++it) { // progress is non-decreasing in the iteration: the valid ones form a prefix
    double sp = clampd(double(it + 1) / double(s.swing_end - s.swing_start), 0.0, 1.0) * c.swing_progress_scaler;
    if (sp >= 0 && sp <= 1.0) c.swing_c_valid = it + 1;
  }
  c.velocity_input_mode = p.velocity_input_mode;
  c.manual_posing = p.manual_posing;
  c.auto_posing = p.auto_posing;
  c.inclination_posing = p.inclination_posing;
  c.imu_posing = p.imu_posing;
  c.admittance_control = p.admittance_control;
  c.dynamic_stiffness = p.dynamic_stiffness;
  c.use_joint_effort = p.use_joint_effort;
  c.clamp_joint_positions = p.clamp_joint_positions;
  c.clamp_joint_velocities = p.clamp_joint_velocities;
  c.force_normal_touchdown = p.force_normal_touchdown;
  // Leg::calculateTipForce (model.cpp:667-708) filters the force of the measured joint torques into tip_force_calculated_.
  // Until a torque has been supplied (RT_EFFORT_LIVE) it filters zeros into a zero state: the estimate is exactly zero and
  // stays it, so the kernels without the estimate run (its planes are neither loaded nor stored).
  c.tip_force = (((features & SHC_FEAT_TIP_FORCE) || p.use_joint_effort) && (rt_flags & RT_EFFORT_LIVE)) ? 1 : 0;
  c.odometry = (features & SHC_FEAT_ODOMETRY) ? 1 : 0;
  c.gravity_aligned = hostinit::tips_rotation_tracked(p, max_dof(p)) ? 1 : 0;
  c.gravity_target = hostinit::tips_rotation_constrained(p, max_dof(p)) ? 1 : 0;
  c.joint_control = 0;
  if (p.leg_manipulation_mode == SHC_MANIPULATION_JOINT_CONTROL) {
    c.joint_control = 1;
    for (int l = 0; l < p.leg_count; ++l)
      if (p.leg_dof[l] == 3) c.joint_control = 2; // (walk_controller.cpp:677: "works only for 3DOF legs")
  }
  c.rough_terrain = p.rough_terrain_mode ? 1 : 0;
  c.tip_align = (p.gravity_aligned_tips && p.leg_dof[0] <= 3) ? 1 : 0; // pose_controller.cpp:849: LEG 0's joint count decides for the whole robot
  c.step_depth = p.step_depth;
  {
    V3 d = hostinit::gravity_aligned_direction();
    c.target_dir[0] = d.x;
    c.target_dir[1] = d.y;
    c.target_dir[2] = d.z;
  }
#ifdef SHC_ABLATE // development builds only (scripts/ablate.py): phase ablation mask
  if (const char *dbg = getenv("SHC_DEBUG_SKIP")) c.debug_skip = atoi(dbg);
#endif
  for (int i = 0; i < 3; ++i) {
    c.max_translation[i] = p.max_translation[i];
    c.max_rotation[i] = p.max_rotation[i];
  }
  c.max_translation_velocity = p.max_translation_velocity;
  c.max_rotation_velocity = p.max_rotation_velocity;
  c.pid_p = p.rotation_pid_gains[0];
  c.pid_i = p.rotation_pid_gains[1];
  c.pid_d = p.rotation_pid_gains[2];
  hostinit::admittance_map(p, c.adm_m00, c.adm_m01, c.adm_m10, c.adm_m11, c.adm_g0, c.adm_g1);
  c.force_gain = c.pose_force_gain = p.force_gain;
  c.pose_swing_height = p.swing_height;
  c.virtual_stiffness = p.virtual_stiffness;
  c.swing_stiffness_scaler = p.swing_stiffness_scaler;
  c.load_stiffness_scaler = p.load_stiffness_scaler;
  c.n_auto_posers = p.n_auto_posers;
  c.pose_phase_length = t.pose_phase_length;
  c.pose_sync = (p.pose_frequency == -1.0) ? 1 : 0;
  c.auto_pose_reference_leg = t.auto_pose_reference_leg;
  for (int i = 0; i < p.n_auto_posers && i < kMaxAutoPosers; ++i) {
    c.ap_start[i] = p.pose_phase_starts[i] * t.pose_normaliser;
    c.ap_end[i] = p.pose_phase_ends[i] * t.pose_normaliser;
    c.ap_amp[i][0] = p.x_amplitudes[i];
    c.ap_amp[i][1] = p.y_amplitudes[i];
    c.ap_amp[i][2] = p.z_amplitudes[i];
    c.ap_amp[i][3] = p.gravity_amplitudes[i];
    c.ap_amp[i][4] = p.roll_amplitudes[i];
    c.ap_amp[i][5] = p.pitch_amplitudes[i];
    c.ap_amp[i][6] = p.yaw_amplitudes[i];
  }
}

static int upload_consts(shc_engine *e);
static int validate_params(const shc_params *p, int *L, int *NJ) {
  if (!p) return fail(SHC_ERR_INVALID_ARG, "params is NULL");
  if (p->leg_count < 3 || p->leg_count > SHC_MAX_LEGS) return fail(SHC_ERR_INVALID_ARG, "leg_count must be 3..8");
  const int nj = max_dof(*p);
  for (int l = 0; l < p->leg_count; ++l)
    if (p->leg_dof[l] < 3 || p->leg_dof[l] > 5) return fail(SHC_ERR_UNSUPPORTED, "supported joints per leg (leg_dof): 3..5 DOF");
  // (gravity_aligned_tips on a robot whose legs differ in DOF: the reference decides per leg - legs of more than 3 joints constrain their tip
  //  rotation, walk_controller.cpp:37, :1195, model.cpp:880 - and by LEG 0's joint count whether the tip-align pose runs, over ALL legs,
  //  pose_controller.cpp:849; both are run-time tests on the padded chains here)
  if (p->rough_terrain_mode && !(p->touchdown_threshold >= p->liftoff_threshold))
    return fail(SHC_ERR_INVALID_ARG, "touchdown_threshold must be >= liftoff_threshold");
  if (p->n_auto_posers < 0 || p->n_auto_posers > kMaxAutoPosers) return fail(SHC_ERR_INVALID_ARG, "n_auto_posers out of range");
  if (!(p->time_delta > 0) || !(p->step_frequency > 0)) return fail(SHC_ERR_INVALID_ARG, "time_delta / step_frequency must be > 0");
  // gait integers feed integer divisions / modulos on the host (generateStepCycle) and on the device (phase arithmetic)
  if (p->stance_phase <= 0 || p->swing_phase <= 0 || p->phase_offset <= 0 || p->stance_phase > 4096 || p->swing_phase > 4096)
    return fail(SHC_ERR_INVALID_ARG, "gait: stance_phase, swing_phase and phase_offset must be positive (and <= 4096)");
  for (int l = 0; l < p->leg_count; ++l)
    if (p->offset_multiplier[l] < 0) return fail(SHC_ERR_INVALID_ARG, "gait: offset_multiplier must be >= 0");
  {
    const double raw = ((1.0 / p->step_frequency) / p->time_delta) / (double(p->swing_phase) / double(p->stance_phase + p->swing_phase));
    const double periods = raw / double(p->stance_phase + p->swing_phase);
    if (!(periods >= 0.0) || !(periods * (p->stance_phase + p->swing_phase) < double(LW_PHASE_MASK)))
      return fail(SHC_ERR_INVALID_ARG, "gait: the step period (1 / (step_frequency * time_delta), rounded) does not fit the phase field");
    if (int(periods) == 0) // roundToEvenInt(raw / base) == 0: period 0
      return fail(SHC_ERR_INVALID_ARG, "gait: step period rounds to 0 iterations (step_frequency * time_delta too large)");
  }
  if (p->auto_posing && p->pose_frequency != -1.0 && (!(p->pose_frequency > 0) || p->pose_phase_length <= 0))
    return fail(SHC_ERR_INVALID_ARG, "auto pose: pose_frequency must be -1 (step-cycle sync) or > 0 with pose_phase_length > 0");
  *L = p->leg_count;
  *NJ = nj;
  return SHC_OK;
}

template <int NJ>
static int generate_tables_nj(const shc_params *p, shc_tables *out) {
  return hostinit::generate_tables<NJ>(*p, *out) ? SHC_OK : fail(SHC_ERR_INVALID_ARG, "init chain failed (unreachable stance?)");
}

extern "C" int shc_abi_version(void) { return 6; } // 6: shc_engine_adjust_parameter; 5: shc_engine_step_k (K cycles per launch, each with its own inputs); 4: shc_cycle_inputs.direct (launch-free posts); 3: shc_leg_snapshot carries the stepper target tip direction; resident mode, join, auxiliary state
extern "C" int64_t shc_sizeof_params(void) { return (int64_t)sizeof(shc_params); }
extern "C" int64_t shc_sizeof_tables(void) { return (int64_t)sizeof(shc_tables); }

extern "C" int shc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" const char *shc_last_error(void) { return g_last_error.c_str(); }

extern "C" int shc_debug_plane_copy(int device, int64_t n_doubles, int reps) {
  if (n_doubles < 2 || (n_doubles & 1) || reps < 1) return fail(SHC_ERR_INVALID_ARG, "n_doubles must be even and >= 2, reps >= 1");
  HIP_TRY(hipSetDevice(device));
  StageArena none{nullptr, 0, 0};
  HostCall hc(none, nullptr);
  double *a = hc.scratch<double>(size_t(n_doubles)), *b = hc.scratch<double>(size_t(n_doubles));
  if (const int rc = hc.status()) return rc;
  HIP_TRY(hipMemsetAsync(a, 0, size_t(n_doubles) * 8, hc.stream));
  const int64_t n_pairs = n_doubles / 2;
  for (int r = 0; r < reps; ++r)
    shc_plane_copy_kernel<<<dim3((unsigned)((n_pairs + 255) / 256)), dim3(256)>>>((const double2 *)a, (double2 *)b, n_pairs);
  return hc.finish();
}

extern "C" int shc_stream_create(int device, void **stream) {
  if (!stream) return fail(SHC_ERR_INVALID_ARG, "stream is NULL");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void *)s;
  return SHC_OK;
}
extern "C" int shc_stream_destroy(int device, void *stream) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamDestroy((hipStream_t)stream));
  return SHC_OK;
}

extern "C" int shc_generate_tables(const shc_params *params, shc_tables *out) {
  int L, NJ;
  int rc = validate_params(params, &L, &NJ);
  if (rc != SHC_OK) return rc;
  if (!out) return fail(SHC_ERR_INVALID_ARG, "out is NULL");
  const shc_params np = normalised_params(*params);
  return dispatch_nj(NJ, [&](auto nj) { return generate_tables_nj<decltype(nj)::value>(&np, out); });
}

// ---- init chain on the device: the same host + device functions as shc_generate_tables, fanned out over morphologies
template <int NJ>
__global__ void init_chain_legs_kernel(const shc_params *params, shc_tables *tables, const int32_t *status, int64_t count) {
  int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; // one thread per (morphology, leg, bearing)
  int64_t m = t / (SHC_MAX_LEGS * 8);
  int r = int(t - m * (SHC_MAX_LEGS * 8));
  int l = r / 8, b = r % 8 + 1;
  if (m >= count || status[m] != SHC_OK) return;
  const shc_params &p = params[m];
  // (a robot whose legs differ in DOF runs on the chain of its longest leg: the host has padded the shorter legs - normalised_params - exactly as
  //  shc_generate_tables does, so Model::generateWorkspaces' per-leg search, model.cpp:309-510, evaluates each leg's own joints)
  int nj = 0;
  for (int k = 0; k < p.leg_count && k < SHC_MAX_LEGS; ++k) nj = p.leg_dof[k] > nj ? p.leg_dof[k] : nj;
  if (nj != NJ || l >= p.leg_count) return;
  hostinit::generate_tables_leg<NJ>(p, l, tables[m], b, b);
}
__global__ void init_chain_head_kernel(const shc_params *params, shc_tables *tables, int32_t *status, int64_t count) {
  int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= count || status[m] != SHC_OK) return;
  if (!hostinit::generate_tables_head(params[m], tables[m])) status[m] = SHC_ERR_INVALID_ARG;
}
__global__ void init_chain_tail_kernel(const shc_params *params, shc_tables *tables, const int32_t *status, int64_t count) {
  int64_t m = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (m >= count || status[m] != SHC_OK) return;
  hostinit::generate_tables_tail(params[m], tables[m]);
}

extern "C" int shc_generate_tables_batch(const shc_params *params, int64_t count, shc_tables *out, int32_t *status, int device) {
  if (!params || !out || count < 1) return fail(SHC_ERR_INVALID_ARG, "params / out NULL or count < 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SHC_ERR_NO_DEVICE, "no HIP device visible");
  HIP_TRY(hipSetDevice(device));
  std::vector<int32_t> st(count);
  std::vector<shc_params> np(static_cast<size_t>(count));
  for (int64_t i = 0; i < count; ++i) { // parameter screening is host logic (same rules as shc_engine_create)
    int L, NJ;
    st[i] = validate_params(&params[i], &L, &NJ);
    np[size_t(i)] = st[i] == SHC_OK ? normalised_params(params[i]) : params[i]; // (neutral entries for the padded joints of legs shorter than the robot's longest)
  }
  StageArena none{nullptr, 0, 0};
  HostCall hc(none, nullptr);
  const shc_params *d_p = hc.in(np.data(), size_t(count), 0);
  shc_tables *d_t = hc.out(out, size_t(count), 0);
  int32_t *d_s = hc.scratch<int32_t>(size_t(count));
  if (const int rc = hc.status()) return rc;
  HIP_TRY(hipMemcpyAsync(d_s, st.data(), size_t(count) * 4, hipMemcpyHostToDevice, hc.stream));
  HIP_TRY(hipMemsetAsync(d_t, 0, size_t(count) * sizeof(shc_tables), hc.stream));
  hc.back(st.data(), d_s, size_t(count));
  const unsigned gm = (unsigned)((count + 63) / 64), gl = (unsigned)((count * SHC_MAX_LEGS * 8 + 63) / 64);
  init_chain_head_kernel<<<dim3(gm), dim3(64)>>>(d_p, d_t, d_s, count);
  init_chain_legs_kernel<3><<<dim3(gl), dim3(64)>>>(d_p, d_t, d_s, count);
  init_chain_legs_kernel<4><<<dim3(gl), dim3(64)>>>(d_p, d_t, d_s, count);
  init_chain_legs_kernel<5><<<dim3(gl), dim3(64)>>>(d_p, d_t, d_s, count);
  init_chain_tail_kernel<<<dim3(gm), dim3(64)>>>(d_p, d_t, d_s, count);
  if (const int rc = hc.finish()) return rc;
  for (int64_t i = 0; i < count; ++i) {
    if (st[i] != SHC_OK) memset(static_cast<void *>(&out[i]), 0, sizeof(shc_tables));
    if (status) status[i] = st[i];
  }
  return SHC_OK;
}

// rough terrain mode with a stance span modifier: LegStepper::calculateStanceSpanChange interpolates the layered workspace at the
// default tip's height at every swing / stance start - the planes of every leg's workspace, searched again from the default
// configuration the tables hold (the init chain itself only keeps the plane at height 0)
template <int NJ>
static int build_span_table(shc_engine *e) {
  e->span_dirty = false;
  const shc_params &p = e->params;
  if (!(p.rough_terrain_mode && p.stance_span_modifier != 0.0)) {
    e->st.span = nullptr;
    return SHC_OK;
  }
  std::vector<double> tab(size_t(e->L) * SpanTable::kStride, 0.0);
  static_assert(SpanTable::kPlanes >= hostinit::kMaxWorkspacePlanes, "span table holds every plane of the layered workspace");
  for (int l = 0; l < e->L; ++l) {
    hostinit::LayeredPlanes planes;
    shc_tables scratch = e->tables;
    hostinit::generate_tables_leg<NJ>(p, l, scratch, 1, 8, e->tables.default_joint_position[l], &planes);
    double m = p.stance_span_modifier;
    const bool positive_y = p.stance_position[l][1] > 0.0;
    const int bearing = (positive_y ^ (m > 0.0)) ? 270 : 90;
    m *= positive_y ? 1.0 : -1.0;
    double *t = &tab[size_t(l) * SpanTable::kStride];
    t[0] = planes.n;
    t[1] = m;
    for (int k = 0; k < planes.n; ++k) t[2 + 2 * k] = planes.height[k], t[3 + 2 * k] = planes.radius[k][bearing / 45];
  }
  if (!e->d_span) HIP_TRY(hipMalloc(&e->d_span, tab.size() * 8));
  HIP_TRY(hipMemcpyAsync(e->d_span, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->st.span = e->d_span;
  return SHC_OK;
}

static int upload_consts(shc_engine *e) {
  if (e->span_dirty) {
    const int rc = dispatch_nj(e->NJ, [&](auto nj) { return build_span_table<decltype(nj)::value>(e); });
    if (rc != SHC_OK) return rc;
  }
  return dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    SharedConsts<L, NJ> c;
    build_shared_consts<L, NJ>(e->params, e->tables, e->cp, c);
    if (!e->d_consts) HIP_TRY(hipMalloc(&e->d_consts, sizeof c));
    HIP_TRY(hipMemcpyAsync(e->d_consts, &c, sizeof c, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SHC_OK;
  });
}

template <int NJ>
static void build_templates(const shc_engine *e, std::vector<double> &legt, std::vector<int32_t> &legw, std::vector<double> &robt,
                            std::vector<int32_t> &robi) {
  using F = Fields<NJ>;
  using R = RobotFields;
  const int nf = F::COUNT;
  legt.assign(size_t(e->L) * nf, 0.0);
  legw.assign(e->L, 0);
  for (int l = 0; l < e->L; ++l) {
    double *t = &legt[size_t(l) * nf];
    for (int j = 0; j < NJ; ++j) {
      t[F::Q + j] = e->tables.default_joint_position[l][j];
      // Joint::current_position_ until a joint state message arrives: Leg::init(true) copied the initial default positions
      // (model.cpp:292-296, :1038) and nothing on this path writes it again
      t[F::MEAS_Q + j] = clampd(0.0, e->params.joint[l][j].min, e->params.joint[l][j].max);
    }
    double sx = e->params.stance_position[l][0], sy = e->params.stance_position[l][1];
    // LegStepper constructor (walk_controller.cpp:795-819): everything at the identity tip pose
    const int at_identity[] = {F::TIP, F::SORG, F::TORG, F::DFLT, F::TARG};
    for (int f : at_identity) {
      t[f] = sx;
      t[f + 1] = sy;
      t[f + 2] = 0.0;
    }
    // model tip of the start-up configuration (for getters before the first cycle)
    LegConst<NJ> lc;
    hostinit::fill_leg_const<NJ>(e->params, l, lc);
    double q[NJ];
    for (int j = 0; j < NJ; ++j) q[j] = t[F::Q + j];
    Chain<NJ> ch;
    fk_chain<NJ>(lc, q, ch);
    V3 tip = tip_robot_frame(lc, ch.pe);
    t[F::MODEL_TIP] = tip.x;
    t[F::MODEL_TIP + 1] = tip.y;
    t[F::MODEL_TIP + 2] = tip.z;
    // step_state STANCE, phase 0, progress "none" (walk_controller.h:493-501)
    legw[l] = SS_STANCE | (PM_NONE << LW_PM_SHIFT);
    if (hostinit::tips_rotation_constrained(e->params, e->params.leg_dof[l])) { // current / origin / target tip poses start at the identity tip pose (:800-803)
      V3 d = hostinit::gravity_aligned_direction();
      t[F::ORG_DIR] = t[F::CUR_DIR] = t[F::TARG_DIR] = d.x;
      t[F::ORG_DIR + 1] = t[F::CUR_DIR + 1] = t[F::TARG_DIR + 1] = d.y;
      t[F::ORG_DIR + 2] = t[F::CUR_DIR + 2] = t[F::TARG_DIR + 2] = d.z;
      legw[l] |= LW_ROTDEF | LW_TARGROT;
    } else if (hostinit::tips_rotation_tracked(e->params, NJ)) { // ... at UNDEFINED_ROTATION, whose rotated x axis is x itself (also a <= 3-joint leg next to longer ones)
      t[F::ORG_DIR] = t[F::CUR_DIR] = 1.0;
    }
  }
  robt.assign(R::COUNT, 0.0);
  robt[R::PNORM + 2] = 1.0;
  robt[R::PNORM_PREV + 2] = 1.0;
  robt[R::OWPP + 2] = e->params.body_clearance; // pose_controller.cpp:39-40
  robt[R::OWPP + 3] = 1.0;
  robt[R::MPOSE + 3] = 1.0;
  robt[R::IMUQ + 0] = 1.0;
  robt[R::APREV + 0] = 1.0;
  robt[R::CPOSE + 2] = e->params.body_clearance;
  robt[R::CPOSE + 3] = 1.0;
  robt[R::WPP + 2] = e->params.body_clearance;
  robt[R::WPP + 3] = 1.0;
  robt[R::ODOM + 2] = 1.0; // identity (walk_controller.cpp:28): x, y, qw, qz
  robt[R::TALIGN + 3] = robt[R::OTALIGN + 3] = 1.0; // identity (pose_controller.h:132-133)
  robi.assign(R::I_COUNT, 0);
  robi[R::I_WORD] = WS_STOPPED | (PS_POSING_COMPLETE << RW_APS_SHIFT);
  // Auto posing on its own clock (pose_frequency != -1): PoseController::updateCurrentPose already runs in every loop of
  // the direct start-up (state_controller.cpp:165-167 with robot_state PACKED; one loop per transitionConfiguration step,
  // pose_controller.cpp:1476-1567), and every call advances the pose phase counter and lets the posers latch on
  // (start_check is unconditional without step-cycle sync, :1359-1371).  Replay those calls for the flags / counter the
  // first RUNNING cycle starts from; the walk state is STOPPED throughout, hence auto_posing_state STOP_POSING.
  if (e->params.auto_posing && e->params.pose_frequency != -1.0 && e->tables.pose_phase_length > 0 && !e->fresh_pose_controller) { // (a start-up SEQUENCE begins with a fresh PoseController:
    int calls = round_to_int(e->params.time_to_start / e->params.time_delta);                                                    //  its loops run the pose themselves, sequence_launch)
    if (calls < 1) calls = 1;
    const int len = e->tables.pose_phase_length, nrm = e->tables.pose_normaliser;
    int phase_counter = 0, flags = 0;
    for (int c = 0; c < calls; ++c) {
      const int master_phase = phase_counter;
      phase_counter = (phase_counter + 1) % len;
      for (int i = 0; i < e->params.n_auto_posers && i < kMaxAutoPosers; ++i) {
        int fl = (flags >> (4 * i)) & 15;
        bool start_check = fl & 1, end1 = fl & 2, end2 = fl & 4, allow = fl & 8;
        int phase = master_phase, sp = e->params.pose_phase_starts[i] * nrm, ep = e->params.pose_phase_ends[i] * nrm;
        if (sp > ep) {
          ep += len;
          if (phase < sp) phase += len;
        }
        start_check = true;
        end1 = end1 || phase == sp;          // auto_posing_state == STOP_POSING
        end2 = end2 || (phase == ep && end1);
        if (!allow && start_check) {
          allow = true;
          end1 = end2 = false;
        }
        flags = (flags & ~(15 << (4 * i))) | ((int(start_check) | int(end1) << 1 | int(end2) << 2 | int(allow) << 3) << (4 * i));
      }
    }
    robi[R::I_POSE_PHASE] = phase_counter;
    robi[R::I_APOSER] = flags;
    // ... and each leg's negation latch (LegPoser::updateAutoPose :1716-1731; step state STANCE throughout the start-up)
    for (int l = 0; l < e->L; ++l) {
      int ns = e->params.pose_negation_phase_starts[l] * nrm, ne = e->params.pose_negation_phase_ends[l] * nrm;
      if (ns == 0) ns = len;
      if (ne == 0) ne = len;
      bool neg = false;
      for (int c = 0; c < calls; ++c) {
        int sp = ns, ep = ne, np = c % len;
        if (sp > ep) {
          ep += len;
          if (np < sp) np += len;
        }
        if (np == sp) neg = true;
        if (np < sp || np > ep) neg = false;
      }
      if (neg) legw[l] |= LW_NEG;
    }
  }
}

static int init_state(shc_engine *e) {
  std::vector<double> legt, robt;
  std::vector<int32_t> legw, robi;
  dispatch_nj(e->NJ, [&](auto nj) { build_templates<decltype(nj)::value>(e, legt, legw, robt, robi); });
  HostCall hc(e);
  const double *d_legt = hc.in(legt.data(), legt.size(), 0), *d_robt = hc.in(robt.data(), robt.size(), 0);
  const int32_t *d_legw = hc.in(legw.data(), legw.size(), 0), *d_robi = hc.in(robi.data(), robi.size(), 0);
  if (const int rc = hc.status()) return rc;
  HIP_TRY(hipMemsetAsync(e->st.legd, 0, size_t(e->n_leg_fields) * e->n_slots * 8, e->stream));
  HIP_TRY(hipMemsetAsync(e->st.legi, 0, size_t(e->n_slots) * 4, e->stream));
  int64_t threads = e->n * e->L;
  init_state_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, e->stream>>>(
      e->st, d_legt, d_legw, d_robt, d_robi, e->L, e->n_leg_fields, RobotFields::COUNT, RobotFields::I_COUNT);
  return hc.finish();
}

static int engine_create(const shc_params *params, const shc_tables *tables, int64_t n_instances, int device, void *stream,
                         shc_engine **out);
extern "C" int shc_engine_create(const shc_params *params, int64_t n_instances, int device, void *stream, shc_engine **out) {
  return engine_create(params, nullptr, n_instances, device, stream, out);
}
extern "C" int shc_engine_create_with_tables(const shc_params *params, const shc_tables *tables, int64_t n_instances, int device,
                                             void *stream, shc_engine **out) {
  if (!tables) return fail(SHC_ERR_INVALID_ARG, "tables is NULL");
  if (tables->step.period <= 0) return fail(SHC_ERR_INVALID_ARG, "tables were not generated (step period 0)");
  return engine_create(params, tables, n_instances, device, stream, out);
}
static int engine_create(const shc_params *params, const shc_tables *tables, int64_t n_instances, int device, void *stream,
                         shc_engine **out) {
  int L, NJ;
  int rc = validate_params(params, &L, &NJ);
  if (rc != SHC_OK) return rc;
  if (!out || n_instances < 1) return fail(SHC_ERR_INVALID_ARG, "n_instances must be >= 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(SHC_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(SHC_ERR_INVALID_ARG, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  shc_engine *e = new shc_engine();
  memset(static_cast<void *>(e), 0, sizeof *e);
  e->span_dirty = e->main_dirty = true; // (the memset above also clears the members' default initialisers)
  e->params = normalised_params(*params); // (legs shorter than the robot's longest: neutral entries for their padded joints)
  e->L = L;
  e->NJ = NJ;
  e->device = device;
  e->stream = (hipStream_t)stream;
  e->n = n_instances;
  e->features = SHC_FEAT_TIP_FORCE | SHC_FEAT_ODOMETRY;
  if (const char *v = getenv("SHC_ROT_SPLIT")) e->half_steps = atoi(v) > 0 ? 1 : -1;
  if (tables) {
    e->tables = *tables;
    e->span_dirty = true;
  } else {
    rc = shc_generate_tables(params, &e->tables);
    if (rc != SHC_OK) {
      delete e;
      return rc;
    }
  }
  build_cycle_params(e->params, e->tables, e->features, e->rt_flags, e->cp);
  const int rpw = 64 / L;
  e->n_waves = (n_instances + rpw - 1) / rpw;
  // Plane stride: 64 slots per wave + 3 KiB of padding.  A wave touches the same 1 KiB offset of ~30 planes; with a stride that
  // is a multiple of a large power of two (8 192 hexapod waves: 8 MiB, 16 384 octopod waves: 16 MiB) those accesses fall on
  // the same HBM channels.  Measured with 192 slots of padding: 81 920 hexapods 62.3 -> 53.1 us per launch, 131 072 octopods
  // 135.7 -> 129.2, 65 536 hexapods 45.8 -> 44.4, neutral at 4 096 (64 ... 65 600 slots all give the same).
  e->n_slots = e->n_waves * 64 + kPlanePadSlots;
  e->n_rob_pad = e->n_waves * rpw; // robots incl. the padding of the last wave's tile
  e->n_leg_fields = LEG_FIELD(e, COUNT);
  e->st.n_slots = e->n_slots;
  e->st.n_rob_pad = e->n_rob_pad;
  e->st.n_robots = e->n;
  HIP_TRY_OR(hipMalloc(&e->st.legd, size_t(e->n_leg_fields) * e->n_slots * 8), shc_engine_destroy(e));
  HIP_TRY_OR(hipMalloc(&e->st.legi, size_t(e->n_slots) * 4), shc_engine_destroy(e));
  // robot state: one contiguous [field][rpw] tile per wave
  HIP_TRY_OR(hipMalloc(&e->st.robd, size_t(RobotFields::COUNT) * e->n_rob_pad * 8), shc_engine_destroy(e));
  HIP_TRY_OR(hipMalloc(&e->st.robi, size_t(RobotFields::I_COUNT) * e->n_rob_pad * 4), shc_engine_destroy(e));
  HIP_TRY_OR(hipMemsetAsync(e->st.robd, 0, size_t(RobotFields::COUNT) * e->n_rob_pad * 8, e->stream), shc_engine_destroy(e));
  HIP_TRY_OR(hipMemsetAsync(e->st.robi, 0, size_t(RobotFields::I_COUNT) * e->n_rob_pad * 4, e->stream), shc_engine_destroy(e));
  e->stage_bytes = size_t(e->n) * L * (NJ > 3 ? NJ : 3) * 8 + size_t(e->n) * 8 * 8 + size_t(SHC_MAX_LEGS) * SHC_MAX_JOINTS * 8 + 4096;
  HIP_TRY_OR(hipMalloc(&e->d_stage, e->stage_bytes), shc_engine_destroy(e));
  e->stage = StageArena{reinterpret_cast<char *>(e->d_stage), e->stage_bytes, 0};
  rc = upload_consts(e);
  if (rc == SHC_OK) rc = init_state(e);
  // The reference's loop() that enters RUNNING also executes runningState() once with the (zero) inputs present at
  // that moment (state_controller.cpp:277-281 then :189-192): the engine's initial state includes that cycle.
  if (rc == SHC_OK) rc = shc_engine_step(e, 1);
  if (rc == SHC_OK) rc = shc_engine_synchronize(e);
  if (rc != SHC_OK) {
    shc_engine_destroy(e);
    return rc;
  }
  *out = e;
  return SHC_OK;
}

extern "C" int shc_engine_destroy(shc_engine *e) {
  if (!e) return SHC_OK;
  (void)hipSetDevice(e->device);
  resident_shutdown(e);
  for (hipStream_t hs : e->half_stream) // (the halves of split steps: nothing may still be running on the buffers freed below)
    if (hs) (void)hipStreamSynchronize(hs);
  (void)hipStreamSynchronize(e->stream);
  release_checkpoints(e);
  (void)hipFree(e->st.legd);
  (void)hipFree(e->st.legi);
  (void)hipFree(e->st.robd);
  (void)hipFree(e->st.robi);
  (void)hipFree(e->st.ext);
  (void)hipFree(e->st.manual);
  (void)hipFree(e->d_seq);
  (void)hipFree(e->d_consts);
  (void)hipFree(e->d_stage);
  (void)hipFree(e->d_span);
  (void)hipFree(e->k_out);
  (void)hipFree(e->k_in);
  (void)hipFree(e->d_health);
  if (e->half_stream[0]) { // (the streams belong to the process-wide pair)
    (void)hipEventDestroy(e->ev_main);
    (void)hipEventDestroy(e->ev_half[0]);
    (void)hipEventDestroy(e->ev_half[1]);
    for (hipEvent_t ev : e->ev_in)
      if (ev) (void)hipEventDestroy(ev);
  }
  delete e;
  return SHC_OK;
}

extern "C" int shc_engine_set_stream(shc_engine *e, void *stream) {
  SHC_ENTER_JOINED(e);
  e->stream = (hipStream_t)stream;
  return SHC_OK;
}

extern "C" int shc_engine_set_features(shc_engine *e, uint32_t features) {
  SHC_ENTER_JOINED(e);
  e->features = features;
  rebuild_cycle_params(e);
  return upload_consts(e);
}

extern "C" int shc_engine_get_tables(const shc_engine *e, shc_tables *out) {
  if (!e || !out) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  *out = e->tables;
  return SHC_OK;
}

extern "C" int64_t shc_engine_instances(const shc_engine *e) { return e ? e->n : 0; }

// ---- input / output plumbing (host arrays: shc_stage.hpp)
// While split steps are in flight (large batches, shc_engine_step) a device-resident input array is scattered by EACH HALF'S OWN
// stream - ordered after that half's earlier steps and before its later ones by stream order alone, so that new inputs cost no
// join (a join drains both halves and costs the overlap the split exists for).  The caller's array is ready on the engine's
// stream: both half streams first wait for that.
static bool split_inputs(const shc_engine *e, int on_device) { return on_device && e->side_busy; }
static int split_inputs_begin(shc_engine *e) {
  HIP_TRY(hipEventRecord(e->ev_main, e->stream));
  HIP_TRY(hipStreamWaitEvent(e->half_stream[0], e->ev_main, 0));
  HIP_TRY(hipStreamWaitEvent(e->half_stream[1], e->ev_main, 0));
  return SHC_OK;
}
// ... and once both halves have read the caller's array the engine's stream is ordered after those reads (events, no host wait, no
// join of the steps): whatever the caller queues on the engine's stream next - a copy_ into the same tensor, a free that the caching
// allocator turns into a reuse - cannot overtake the scatter kernels, which may sit behind several queued steps of their half.
static int split_inputs_end(shc_engine *e) {
  for (int h = 0; h < 2; ++h) {
    if (!e->ev_in[h]) HIP_TRY(hipEventCreateWithFlags(&e->ev_in[h], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e->ev_in[h], e->half_stream[h]));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_in[h], 0));
  }
  return SHC_OK;
}
// How a launch of the cycle kernel cuts the batch - for shc_engine_step, shc_engine_step_k and the inputs scattered between split steps alike.
// One wave per workgroup while the batch has about as many waves as the chip has SIMDs (1 024): the dispatcher then spreads
// them one per SIMD (two-wave groups put pairs on the same SIMDs: 12.9 instead of 9.4 us at 768 waves, 12.2 instead of 10.2 at
// 1 024; equal at 1 536).  Above that, 128-thread groups
// (two waves share one LDS copy of the tables): measured against 64 and 256 threads up to 131 072 instances they are the
// fastest or within noise (-2 ... 3 % on 65 536 hexapods).
struct LaunchGeometry {
  int block;               // threads per workgroup
  int64_t waves_per_block;
  int64_t half;            // split steps: the first wave of the second half (whole workgroups)
  int64_t whole_blocks(int64_t waves) const { return ((waves + waves_per_block - 1) / waves_per_block) * waves_per_block; } // waves, rounded up to whole workgroups
  unsigned grid(int64_t waves) const { return (unsigned)(whole_blocks(waves) / waves_per_block); }
};
static LaunchGeometry launch_geometry(const shc_engine *e) {
  LaunchGeometry g{e->n_waves < 1536 ? 64 : 128, 0, 0};
  g.waves_per_block = g.block / 64;
  g.half = g.whole_blocks(e->n_waves / 2);
  return g;
}
static int64_t split_first_instance_of_second_half(const shc_engine *e) {
  const int64_t r = launch_geometry(e).half * (64 / e->L);
  return r < e->n ? r : e->n;
}

#include "shc_inputs.hpp" // the eight input groups, their rules and their K-deep staging: the one description every route into the cycle reads

// One input array of the caller into the state.  launch(stream, array, r0, r1): the scatter kernel over instances [r0, r1)
template <class Launch>
static int scatter_input(shc_engine *e, const double *src, size_t doubles_per_instance, int on_device, Launch &&launch) {
  if (!src) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  if (split_inputs(e, on_device)) {
    const int rc = split_inputs_begin(e);
    if (rc != SHC_OK) return rc;
    const int64_t mid = split_first_instance_of_second_half(e);
    launch(e->half_stream[0], src, int64_t(0), mid);
    if (e->n > mid) launch(e->half_stream[1], src, mid, e->n);
    HIP_TRY(hipGetLastError());
    return split_inputs_end(e);
  }
  HostCall hc(e);
  const double *d = hc.in(src, size_t(e->n) * doubles_per_instance, on_device);
  if (const int rc = hc.status()) return rc;
  launch(e->stream, d, int64_t(0), e->n);
  return hc.finish();
}
// (input group g of shc_inputs.hpp, per robot / per leg; Model::setImuData normalises the orientation)
static int scatter_rob(shc_engine *e, const double *src, int g, int on_device) {
  const int K = input_group(g).width, f0 = input_group(g).field, normalize_quat = g == SHC_ACT_IMU_ORIENTATION;
  return scatter_input(e, src, size_t(K), on_device, [=](hipStream_t stream, const double *d, int64_t r0, int64_t r1) {
    scatter_rob_kernel<<<dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, stream>>>(d, e->st.robd, 64 / e->L, r1, K, f0, normalize_quat, r0);
  });
}
static int scatter_leg(shc_engine *e, const double *src, int g, int on_device) {
  const int K = input_k(g, e->NJ), f0 = dispatch_nj(e->NJ, [g](auto nj) { return input_leg_field<decltype(nj)::value>(g); });
  return scatter_input(e, src, size_t(e->L) * K, on_device, [=](hipStream_t stream, const double *d, int64_t r0, int64_t r1) {
    scatter_leg_kernel<<<dim3((unsigned)(((r1 - r0) * e->L + 255) / 256)), dim3(256), 0, stream>>>(d, e->st.legd, e->n_slots, r1, e->L, K, f0, r0);
  });
}

// One output array of the caller from the state.  launch(array): the gather kernel on the engine's stream; a host array is copied back and waited for
template <class T, class Launch>
static int gather_output(shc_engine *e, T *dst, size_t count, int on_device, Launch &&launch) {
  if (!dst) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  HostCall hc(e);
  T *d = hc.out(dst, count, on_device);
  if (const int rc = hc.status()) return rc;
  launch(d);
  return hc.finish();
}
static dim3 grid256(int64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }
static int gather_leg(shc_engine *e, double *dst, int K, int f0, int on_device) {
  const int64_t threads = e->n * e->L;
  return gather_output(e, dst, size_t(threads) * K, on_device, [&](double *d) {
    gather_leg_kernel<<<grid256(threads), dim3(256), 0, e->stream>>>(d, e->st.legd, e->n_slots, e->n, e->L, K, f0);
  });
}
static int gather_rob(shc_engine *e, double *dst, int K, int f0, int on_device) {
  return gather_output(e, dst, size_t(e->n) * K, on_device, [&](double *d) {
    gather_rob_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(d, e->st.robd, 64 / e->L, e->n, K, f0);
  });
}

static int derive_tips(shc_engine *e);

extern "C" int shc_engine_set_velocity(shc_engine *e, const double *linear_xy, const double *angular, int on_device) {
  SHC_ENTER_JOINED_UNLESS(e, split_inputs(e, on_device));
  int rc = scatter_rob(e, linear_xy, SHC_ACT_LINEAR_XY, on_device);
  if (rc != SHC_OK) return rc;
  return scatter_rob(e, angular, SHC_ACT_ANGULAR, on_device);
}

extern "C" int shc_engine_set_imu(shc_engine *e, const double *orientation_wxyz, const double *angular_velocity, int on_device) {
  SHC_ENTER_JOINED_UNLESS(e, split_inputs(e, on_device));
  int rc = scatter_rob(e, orientation_wxyz, SHC_ACT_IMU_ORIENTATION, on_device);
  if (rc != SHC_OK) return rc;
  return scatter_rob(e, angular_velocity, SHC_ACT_IMU_ANGULAR_VELOCITY, on_device);
}

// Leg::touchdownDetection (model.cpp:712-722), run by tipStatesCallback right after it stored the measured force
// (state_controller.cpp:1644-1646): the step plane is where the tip is when the force first exceeds the touchdown threshold.
template <int L, int NJ>
__global__ void touchdown_detection_kernel(DevState st, const SharedConsts<L, NJ> *gc, double touchdown_threshold, double liftoff_threshold) {
  using FD = Fields<NJ>;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= st.n_robots * L) return;
  const int64_t rob = t / L;
  const int leg = int(t - rob * L);
  const int64_t slot = slot_of(rob, leg, L);
  auto f = [&](int field) -> double & { return st.legd[leg_field_index(field, slot, st.n_slots)]; };
  const double fn = norm(V3{f(FD::FORCE_IN), f(FD::FORCE_IN + 1), f(FD::FORCE_IN + 2)});
  if (fn > touchdown_threshold && f(FD::STEP_PLANE + 3) == 0.0) {
    double q[NJ];
    for (int j = 0; j < NJ; ++j) q[j] = f(FD::Q + j);
    Chain<NJ> ch;
    fk_chain<NJ>(gc->leg[leg], q, ch);
    const V3 tip = tip_robot_frame(gc->leg[leg], ch.pe); // step_plane_pose_ = current_tip_pose_
    f(FD::STEP_PLANE) = tip.x, f(FD::STEP_PLANE + 1) = tip.y, f(FD::STEP_PLANE + 2) = tip.z, f(FD::STEP_PLANE + 3) = 1.0;
  } else if (fn < liftoff_threshold) {
    f(FD::STEP_PLANE + 3) = 0.0;
  }
}

// What follows fresh tip forces in the state, on the engine's stream (shc_engine_set_tip_force, the action pass)
static int tip_force_given(shc_engine *e) {
  e->rt_flags |= RT_TOUCHDOWN; // LegStepper::setTouchdownDetection(true) (state_controller.cpp:1642)
  if (!e->params.rough_terrain_mode) return SHC_OK; // the step plane is only read in rough terrain mode (walk_controller.cpp:1065, :1110)
  const int64_t threads = e->n * e->L;
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    touchdown_detection_kernel<L, NJ><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, e->stream>>>(
        e->st, (const SharedConsts<L, NJ> *)e->d_consts, e->params.touchdown_threshold, e->params.liftoff_threshold);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

extern "C" int shc_engine_set_tip_force(shc_engine *e, const double *tip_force, int on_device) {
  SHC_ENTER_JOINED_UNLESS(e, split_inputs(e, on_device && !e->params.rough_terrain_mode));
  int rc = scatter_leg(e, tip_force, SHC_ACT_TIP_FORCE, on_device);
  if (rc != SHC_OK || !tip_force) return rc;
  return tip_force_given(e);
}

// First joint effort (or non-zero filter state): switch to the kernels that evaluate the tip-force estimate.
static int effort_live(shc_engine *e) {
  if (e->rt_flags & RT_EFFORT_LIVE) return SHC_OK;
  e->rt_flags |= RT_EFFORT_LIVE;
  rebuild_cycle_params(e);
  return upload_consts(e);
}

extern "C" int shc_engine_set_joint_effort(shc_engine *e, const double *joint_effort, int on_device) {
  SHC_ENTER_JOINED_UNLESS(e, split_inputs(e, on_device && (e->rt_flags & RT_EFFORT_LIVE)));
  if (joint_effort) { // Leg::calculateTipForce has something to filter from now on
    const int rc = effort_live(e);
    if (rc != SHC_OK) return rc;
  }
  return scatter_leg(e, joint_effort, SHC_ACT_JOINT_EFFORT, on_device);
}

extern "C" int shc_engine_set_pose_input(shc_engine *e, const double *translation_velocity, const double *rotation_velocity,
                                         int on_device) {
  SHC_ENTER_JOINED_UNLESS(e, split_inputs(e, on_device));
  if (translation_velocity || rotation_velocity) e->rt_flags |= RT_MANUAL_LIVE;
  int rc = scatter_rob(e, translation_velocity, SHC_ACT_POSE_TRANSLATION_VELOCITY, on_device);
  if (rc != SHC_OK) return rc;
  return scatter_rob(e, rotation_velocity, SHC_ACT_POSE_ROTATION_VELOCITY, on_device);
}

extern "C" int shc_engine_set_pose_reset_mode(shc_engine *e, const int32_t *mode, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!mode) return SHC_OK;
  e->rt_flags |= RT_MANUAL_LIVE;
  HIP_TRY(hipSetDevice(e->device));
  HostCall hc(e);
  const int32_t *d = hc.in(mode, size_t(e->n), on_device);
  if (const int rc = hc.status()) return rc;
  scatter_robi_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(d, e->st.robi, 64 / e->L, e->n, RobotFields::I_RESET_MODE);
  return hc.finish();
}

// The two streams the halves of split steps run on: ONE pair per device for the whole process, created back to back so that they
// sit on two different hardware queues whatever the caller's own stream is (HIP maps streams to a few hardware queues in
// creation order; two streams on one queue serialise, and a pair created per engine did land on the caller's queue now and then).
// ... "created back to back" is not enough: the runtime hands a new stream the least-used hardware queue of its priority class, and in
// a process that has created and destroyed other streams before (engines that came and went) both streams of the pair can be given the
// same one - the halves then run one after the other and a split step costs what a single launch costs.  The pair is therefore TESTED once: a one-wave kernel on the first
// stream waits (bounded) for a flag that a kernel launched afterwards on the second stream sets - it sees the flag only if the two run
// concurrently, i.e. sit on different queues.  A second stream that fails is kept aside (so that the next one is given another queue)
// and replaced, a few times at most.
__device__ unsigned long long g_queue_probe[2]; // [0] the flag, [1] what the waiting kernel saw
__global__ void queue_probe_reset_kernel() {
  if (threadIdx.x == 0) g_queue_probe[0] = g_queue_probe[1] = 0;
}
__global__ void queue_probe_wait_kernel(unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long seen = 0;
  while ((seen = __hip_atomic_load(&g_queue_probe[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  if (threadIdx.x == 0) g_queue_probe[1] = seen;
}
__global__ void queue_probe_set_kernel() {
  if (threadIdx.x == 0) __hip_atomic_store(&g_queue_probe[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (stream-ordered calls only: no allocation, no null-stream copy - another engine of this process may have a resident loop alive)
static bool streams_run_concurrently(int device, hipStream_t a, hipStream_t b) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
  void *sym = nullptr;
  if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_queue_probe)) != hipSuccess) return true; // (cannot tell: keep the pair)
  unsigned long long h[2] = {0, 1};
  queue_probe_reset_kernel<<<dim3(1), dim3(64), 0, a>>>();
  if (hipStreamSynchronize(a) != hipSuccess) return true;
  queue_probe_wait_kernel<<<dim3(1), dim3(64), 0, a>>>(2ull * (unsigned long long)khz); // 2 ms at most
  queue_probe_set_kernel<<<dim3(1), dim3(64), 0, b>>>();
  bool ok = true;
  if (hipMemcpyAsync(h, sym, 16, hipMemcpyDeviceToHost, a) == hipSuccess && hipStreamSynchronize(a) == hipSuccess) ok = h[1] != 0;
  (void)hipStreamSynchronize(b);
  (void)hipGetLastError();
  return ok;
}
static int split_streams(int device, hipStream_t out[2]) {
  static hipStream_t pool[64][2] = {};
  static std::mutex pool_mutex; // engines of one process may be created and stepped from different host threads
  if (device < 0 || device >= 64) return fail(SHC_ERR_INVALID_ARG, "device index");
  std::lock_guard<std::mutex> lock(pool_mutex);
  if (!pool[device][0]) {
    // The pair is built in locals and published only once both streams exist: a failure on the way destroys what was created (streams set
    // aside included) and leaves the pool empty, so that a later call starts over instead of handing out a null second stream - which
    // would be the legacy default stream.
    hipStream_t a = nullptr, b = nullptr, aside[6] = {};
    int n_aside = 0;
    hipError_t err = hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
    while (err == hipSuccess && n_aside < 6 && !streams_run_concurrently(device, a, b)) {
      aside[n_aside++] = b;
      b = nullptr;
      err = hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
    }
    for (int k = 0; k < n_aside; ++k) (void)hipStreamDestroy(aside[k]);
    if (err != hipSuccess) {
      if (a) (void)hipStreamDestroy(a);
      if (b) (void)hipStreamDestroy(b);
      return fail(SHC_ERR_HIP, std::string("split streams: ") + hipGetErrorString(err));
    }
    if (getenv("SHC_DEBUG_STREAMS")) fprintf(stderr, "shc: split-stream pair of device %d found after %d replacement(s)\n", device, n_aside);
    pool[device][0] = a, pool[device][1] = b;
  }
  out[0] = pool[device][0], out[1] = pool[device][1];
  return SHC_OK;
}
// ... and an engine takes them, with the events that order them against its own stream, the first time it launches a split step
static int ensure_split_streams(shc_engine *e) {
  if (e->half_stream[0]) return SHC_OK;
  const int rc = split_streams(e->device, e->half_stream);
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_half[0], hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_half[1], hipEventDisableTiming));
  return SHC_OK;
}
// Order the engine's stream after everything earlier split steps launched on the split streams (no host wait).
static int join_side(shc_engine *e) {
  e->main_dirty = true;
  if (!e->side_busy) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  for (int h = 0; h < 2; ++h) {
    HIP_TRY(hipEventRecord(e->ev_half[h], e->half_stream[h]));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_half[h], 0));
  }
  e->side_busy = false;
  return SHC_OK;
}
extern "C" int shc_engine_join(shc_engine *e) {
  SHC_ENTER(e);
  return join_side(e);
}

// A launch of W waves on S wave slots runs ceil(W / S) rounds; the last, partly filled round and the next launch's ramp-up leave
// most of the machine idle, and a kernel boundary is a barrier the algorithm does not need: step k + 1 of a robot depends on
// step k of THAT robot only.  From kSplitWaves waves on, a step is therefore launched as two halves of the batch on two streams
// with no join between steps, so that one half's tail overlaps the other half's full rounds (measured on 1 x MI355X: 65 536
// hexapods with admittance + IMU 57.7 -> 48.8 us per step, 131 072 octopods 106 -> 98.7 us).
constexpr int64_t kSplitWaves = 4096;

#include "shc_adjust.hpp" // the operations on a pending shc_engine_adjust_parameter, and the entry point itself
// The launch-uniform parameter block of the engine's parameters, with what a change still waiting for its loop leaves of the old ones.
static void rebuild_cycle_params(shc_engine *e) {
  build_cycle_params(e->params, e->tables, e->features, e->rt_flags, e->cp);
  adjust_overlay(e, e->cp);
}

extern "C" int shc_engine_step(shc_engine *e, int n_cycles) {
  SHC_ENTER(e);
  if (n_cycles < 1) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  const bool marked = (e->rt_flags & (RT_SKIP_MARKED | RT_POSE_MARKED)) != 0; // (the launch of a loop-level call: that call serves the change)
  const bool generic = (e->features & SHC_FEAT_GENERIC_KERNEL) != 0;
  if (adjust_pending(e) && !marked) { // shc_adjust.hpp, row "shc_engine_step, first cycle"
    const int rc = adjust_serve_in_cycle(e, generic);
    if (rc != SHC_OK || n_cycles == 1) return rc;
    --n_cycles;
  }
  return launch_cycles(e, n_cycles, generic);
}

// n control cycles in one launch (generic: on the runtime-flag kernel)
static int launch_cycles(shc_engine *e, int n_cycles, bool generic) {
  if (!(e->rt_flags & (RT_SKIP_MARKED | RT_POSE_MARKED))) e->plan_poser_tips_current = false; // PoseController::updateStance rewrites every LegPoser's tip pose
  const LaunchGeometry g = launch_geometry(e);
  const bool split = e->n_waves >= kSplitWaves && !(e->features & SHC_FEAT_SINGLE_STREAM) && !(e->rt_flags & (RT_SKIP_MARKED | RT_POSE_MARKED));
  CycleLaunch a = cycle_launch(e);
  a.generic = generic, a.block = g.block, a.n_cycles = n_cycles, a.half_steps = e->half_steps;
  int rc;
  if (!split) {
    if ((rc = join_side(e)) != SHC_OK) return rc;
    a.grid = g.grid(e->n_waves);
    if ((rc = launch_cycle_for(e, a)) != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    return SHC_OK;
  }
  if ((rc = ensure_split_streams(e)) != SHC_OK) return rc;
  const bool resync = e->main_dirty; // inputs or state were touched on the engine's stream since the last split step: both halves follow them
  if (resync) {
    HIP_TRY(hipEventRecord(e->ev_main, e->stream));
    HIP_TRY(hipStreamWaitEvent(e->half_stream[0], e->ev_main, 0));
    HIP_TRY(hipStreamWaitEvent(e->half_stream[1], e->ev_main, 0));
    e->main_dirty = false;
  }
  a.stream = e->half_stream[0];
  a.grid = g.grid(g.half);
  if (resync) {
    // Two halves that start together end together - their tails and ramp-ups coincide and nothing overlaps (measured: a join
    // every tenth step costs the whole gain).  After a join the halves are therefore STAGGERED: the first half of this one step
    // goes out as two launches and the second half starts when the first of them is through, i.e. a quarter of a step late;
    // both halves take the same time from then on, so the stagger stays until the next join.
    const int64_t quarter = g.whole_blocks(g.half / 2); // (a quarter or three quarters of a half instead: the same step time within 1 %, profiles/r04_probe_build_variants.txt)
    a.grid = g.grid(quarter);
    if ((rc = launch_cycle_for(e, a)) != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_half[0], e->half_stream[0]));
    HIP_TRY(hipStreamWaitEvent(e->half_stream[1], e->ev_half[0], 0));
    a.wave0 = quarter;
    a.grid = g.grid(g.half - quarter);
  }
  if ((rc = launch_cycle_for(e, a)) != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  a.stream = e->half_stream[1];
  a.wave0 = g.half;
  a.grid = g.grid(e->n_waves - g.half);
  if ((rc = launch_cycle_for(e, a)) != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  e->side_busy = true;
  return SHC_OK;
}

extern "C" int shc_engine_synchronize(shc_engine *e) {
  SHC_ENTER_JOINED(e);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return SHC_OK;
}

#include "shc_resident.hpp" // resident mode: the control loop kept on the chip (shc_engine_resident_*)
static bool resident_active(const shc_engine *e) { return e->res && e->res->active; }
static void resident_shutdown(shc_engine *e) {
  if (e->res && e->res->active) (void)shc_engine_resident_end(e, nullptr);
  if (e->res && e->res->active) { // the loop did not answer: its buffers must outlive it - wait for the kernel itself (it is bounded: max_cycles,
    (void)hipSetDevice(e->device); //  idle timeout, the workers' emergency bound), however long that takes
    (void)hipStreamSynchronize(e->res->loop_stream);
    e->res->active = false;
  }
  resident_free(e->res);
  e->res = nullptr;
}

extern "C" int shc_engine_get_joint_state(shc_engine *e, double *q, double *qd, int on_device) {
  SHC_ENTER_JOINED(e);
  int rc = gather_leg(e, q, e->NJ, LEG_FIELD(e, Q), on_device);
  if (rc != SHC_OK) return rc;
  return gather_leg(e, qd, e->NJ, LEG_FIELD(e, QD), on_device);
}

extern "C" int shc_engine_joint_buffer(shc_engine *e, double **device_ptr, int64_t *n_doubles) {
  SHC_ENTER_JOINED(e);
  if (!device_ptr || !n_doubles) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  *device_ptr = e->st.legd; // fields Q (and, for odd DOF, the first QD) occupy the first ceil(NJ / 2) paired planes of the leg state
  *n_doubles = int64_t((e->NJ + 1) / 2) * e->n_slots * 2;
  return SHC_OK;
}

extern "C" int64_t shc_engine_joint_index(const shc_engine *e, int64_t instance, int leg, int joint) {
  if (!e) return -1;
  int rpw = 64 / e->L;
  int64_t w = instance / rpw;
  int gi = int(instance - w * rpw);
  return leg_field_index(joint, w * 64 + gi * e->L + leg, e->n_slots);
}

extern "C" int shc_engine_get_leg_state(shc_engine *e, double *walker_tip, double *poser_tip, double *model_tip, double *tip_force,
                                        double *admittance, int32_t *leg_status, int on_device) {
  SHC_ENTER_JOINED(e);
  int rc;
  if ((rc = gather_leg(e, walker_tip, 3, LEG_FIELD(e, TIP), on_device)) != SHC_OK) return rc;
  if ((poser_tip || model_tip) && (rc = derive_tips(e)) != SHC_OK) return rc; // derived on demand from q / walker tip / body pose
  if ((rc = gather_leg(e, poser_tip, 3, LEG_FIELD(e, POSER_TIP), on_device)) != SHC_OK) return rc;
  if ((rc = gather_leg(e, model_tip, 3, LEG_FIELD(e, MODEL_TIP), on_device)) != SHC_OK) return rc;
  if ((rc = gather_leg(e, tip_force, 3, LEG_FIELD(e, TF), on_device)) != SHC_OK) return rc;
  if ((rc = gather_leg(e, admittance, 3, LEG_FIELD(e, ADM_DELTA), on_device)) != SHC_OK) return rc;
  const int64_t threads = e->n * e->L;
  return gather_output(e, leg_status, size_t(threads), on_device, [&](int32_t *d) {
    gather_leg_status_kernel<<<grid256(threads), dim3(256), 0, e->stream>>>(d, e->st.legi, e->n, e->L);
  });
}

extern "C" int shc_engine_change_gait(shc_engine *e, const shc_params *ng, int64_t *still_walking) {
  SHC_ENTER_JOINED(e);
  if (!ng) return fail(SHC_ERR_INVALID_ARG, "new gait is NULL");
  HIP_TRY(hipSetDevice(e->device));
  const unsigned grid = (unsigned)((e->n + 255) / 256);
  const int rpw = 64 / e->L;
  int32_t walking = 0;
  {
    HostCall hc(e);
    int32_t *d_count = hc.out(&walking, 1, 0);
    if (const int rc = hc.status()) return rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, 4, e->stream));
    count_walking_kernel<<<dim3(grid), dim3(256), 0, e->stream>>>(d_count, e->st.robi, rpw, e->n);
    if (const int rc = hc.finish()) return rc;
  }
  if (still_walking) *still_walking = walking;
  if (walking) { // state_controller.cpp:531-537
    fill_rob_kernel<<<dim3(grid), dim3(256), 0, e->stream>>>(e->st.robd, rpw, e->n, RobotFields::VIN, 3, 0.0);
    HIP_TRY(hipGetLastError());
    return SHC_OK;
  }
  shc_params p = e->params; // initGaitParameters (state_controller.cpp:1941-1969)
  p.stance_phase = ng->stance_phase;
  p.swing_phase = ng->swing_phase;
  p.phase_offset = ng->phase_offset;
  memcpy(p.offset_multiplier, ng->offset_multiplier, sizeof p.offset_multiplier);
  if (p.auto_posing) { // initAutoPoseParameters (:1973-1999)
    p.pose_frequency = ng->pose_frequency;
    p.pose_phase_length = ng->pose_phase_length;
    p.n_auto_posers = ng->n_auto_posers;
    memcpy(p.pose_phase_starts, ng->pose_phase_starts, sizeof p.pose_phase_starts);
    memcpy(p.pose_phase_ends, ng->pose_phase_ends, sizeof p.pose_phase_ends);
    memcpy(p.pose_negation_phase_starts, ng->pose_negation_phase_starts, sizeof p.pose_negation_phase_starts);
    memcpy(p.pose_negation_phase_ends, ng->pose_negation_phase_ends, sizeof p.pose_negation_phase_ends);
    memcpy(p.negation_transition_ratio, ng->negation_transition_ratio, sizeof p.negation_transition_ratio);
    memcpy(p.x_amplitudes, ng->x_amplitudes, sizeof p.x_amplitudes);
    memcpy(p.y_amplitudes, ng->y_amplitudes, sizeof p.y_amplitudes);
    memcpy(p.z_amplitudes, ng->z_amplitudes, sizeof p.z_amplitudes);
    memcpy(p.gravity_amplitudes, ng->gravity_amplitudes, sizeof p.gravity_amplitudes);
    memcpy(p.roll_amplitudes, ng->roll_amplitudes, sizeof p.roll_amplitudes);
    memcpy(p.pitch_amplitudes, ng->pitch_amplitudes, sizeof p.pitch_amplitudes);
    memcpy(p.yaw_amplitudes, ng->yaw_amplitudes, sizeof p.yaw_amplitudes);
  }
  int L, NJ;
  int rc = validate_params(&p, &L, &NJ);
  if (rc != SHC_OK) return rc;
  shc_tables t;
  if ((rc = shc_generate_tables(&p, &t)) != SHC_OK) return rc; // generateStepCycle + generateLimits (morphology tables come out unchanged)
  e->params = p;
  e->tables = t;
  e->span_dirty = true;
  adjust_bump(e); // new tables: a device checkpoint of the old gait counts its phases in another step cycle
  adjust_drop(e); // shc_adjust.hpp, row "change_gait with every robot STOPPED"
  build_cycle_params(e->params, e->tables, e->features, e->rt_flags, e->cp);
  if ((rc = upload_consts(e)) != SHC_OK) return rc;
  if (p.auto_posing) { // setAutoPoseParams builds fresh AutoPosers: their start / end checks are reset (pose_controller.cpp:39-61)
    fill_robi_kernel<<<dim3(grid), dim3(256), 0, e->stream>>>(e->st.robi, rpw, e->n, RobotFields::I_APOSER, 0);
    HIP_TRY(hipGetLastError());
  }
  return shc_engine_synchronize(e);
}

extern "C" int shc_engine_get_odometry(shc_engine *e, double *pose, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!e->cp.odometry) return fail(SHC_ERR_UNSUPPORTED, "SHC_FEAT_ODOMETRY is off");
  return gather_output(e, pose, size_t(e->n) * 7, on_device, [&](double *d) {
    gather_odometry_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(d, e->st.robd, 64 / e->L, e->n);
  });
}

extern "C" int shc_engine_get_virtual_stiffness(shc_engine *e, double *stiffness, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!e->params.admittance_control) return fail(SHC_ERR_UNSUPPORTED, "admittance_control is off: updateStiffness never runs");
  return gather_leg(e, stiffness, 1, LEG_FIELD(e, ADM_DELTA) + 3, on_device);
}

// The two launch-uniform facts of the derivation (derive_tips_kernel, observe_kernel)
static int derive_poser_tips(const shc_engine *e) { return !(e->cp.auto_posing && !e->cp.imu_posing); } // the auto-pose path stores its per-leg poser tip
static int keep_marked_poser_tips(const shc_engine *e) {
  return e->plan_poser_tips_current && (e->params.imu_posing || e->params.auto_posing || e->params.inclination_posing);
}
static int derive_tips(shc_engine *e) {
  HIP_TRY(hipSetDevice(e->device));
  const int64_t threads = e->n * e->L;
  const int derive_poser = derive_poser_tips(e), keep_marked = keep_marked_poser_tips(e);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    derive_tips_kernel<L, NJ><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, derive_poser,
                                                                                                keep_marked);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

#include "shc_rows.hpp"     // the row pattern of the passes below: block geometry, LDS tile and mover, resolved specs, launch sizes, host forms
#include "shc_leg_msgs.hpp" // the derived LegState fields (one device implementation), shc_engine_get_leg_state_msgs and, through it, shc_engine_read_leg_state_msg
#include "shc_frames.hpp"   // publishFrameTransforms: every joint / tip frame and the body frames, shc_engine_get_frame_transforms
#include "shc_health.hpp"   // the reference's IK / clamping warnings per robot, a restore map and the selected robots: shc_engine_scan_health
#include "shc_observe.hpp"  // chosen fields of every robot as one dense [rows][D] array: shc_engine_get_observations
#include "shc_actions.hpp"  // chosen input groups of every robot from one dense [n][A] array: shc_engine_set_actions
#include "shc_rollout.hpp"  // K cycles per launch from one dense [K][n][A] array, their joints as one dense [cycles][n][D] array: shc_engine_step_k_actions / _get_step_k_observations
#include "shc_rollout_kin.hpp" // what is a pure function of that ring, per cycle: foot tips = FK(q) and the joint-limit health records: shc_engine_get_step_k_kinematics / _scan_step_k_health
#include "shc_resident_rows.hpp" // the resident loop driven from one dense [n][A] array, its joints and tips as one dense [n][D] array: shc_engine_resident_post_actions / _get_observations_async

// ---- the other messages of the path (include/shc_batch.h)
// raw motor positions - Joint::offset_ -> measured joint positions (jointStatesCallback, state_controller.cpp:1581)
__global__ void store_measured_q_kernel(const double *src, double *legd, int64_t n_slots, int64_t n, int L, int NJ, int f0, const double *offset /*[L][NJ]*/) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n * L) return;
  const int64_t rob = t / L;
  const int leg = int(t - rob * L);
  const int64_t slot = slot_of(rob, leg, L);
  for (int j = 0; j < NJ; ++j) legd[leg_field_index(f0 + j, slot, n_slots)] = src[t * NJ + j] - offset[leg * NJ + j];
}
// desired joint state + per-joint position commands (publishDesiredJointState, state_controller.cpp:777-805)
__global__ void joint_commands_kernel(double *pos, double *vel, double *eff, double *cmd, const double *legd, int64_t n_slots, int64_t n, int L, int NJ,
                                      int fq, int fqd, int feff, const double *offset) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n * L) return;
  const int64_t rob = t / L;
  const int leg = int(t - rob * L);
  const int64_t slot = slot_of(rob, leg, L);
  for (int j = 0; j < NJ; ++j) {
    const double q = legd[leg_field_index(fq + j, slot, n_slots)];
    if (pos) pos[t * NJ + j] = q;
    if (vel) vel[t * NJ + j] = legd[leg_field_index(fqd + j, slot, n_slots)];
    if (eff) eff[t * NJ + j] = legd[leg_field_index(feff + j, slot, n_slots)];
    if (cmd) cmd[t * NJ + j] = q + offset[leg * NJ + j];
  }
}
// range-sensor step plane (tipStatesCallback, state_controller.cpp:1657-1672): the surface lies `z` along the tip's x axis
template <int L, int NJ>
__global__ void step_plane_range_kernel(DevState st, const SharedConsts<L, NJ> *gc, const double *step_plane /*[n][L][3]*/) {
  using FD = Fields<NJ>;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= st.n_robots * L) return;
  const int64_t rob = t / L;
  const int leg = int(t - rob * L);
  const int64_t slot = slot_of(rob, leg, L);
  auto f = [&](int field) -> double & { return st.legd[leg_field_index(field, slot, st.n_slots)]; };
  const double z = step_plane[t * 3 + 2];
  if (z != kUnassigned) {
    double q[NJ];
    for (int j = 0; j < NJ; ++j) q[j] = f(FD::Q + j);
    Chain<NJ> ch;
    fk_chain<NJ>(gc->leg[leg], q, ch);
    const V3 p = tip_robot_frame(gc->leg[leg], ch.pe) + base_rotate(gc->leg[leg], ch.xe) * z; // Tip::getPoseRobotFrame(Pose((z, 0, 0), ..))
    f(FD::STEP_PLANE) = p.x, f(FD::STEP_PLANE + 1) = p.y, f(FD::STEP_PLANE + 2) = p.z, f(FD::STEP_PLANE + 3) = 1.0;
  } else {
    f(FD::STEP_PLANE + 3) = 0.0; // lost contact with the range sensor: Pose::Undefined()
  }
}

template <class Fn>
static std::vector<double> leg_joint_table(const shc_engine *e, Fn &&value) { // an [L][NJ] table of value(leg, joint), shared by all instances
  std::vector<double> table(size_t(e->L) * e->NJ);
  for (int l = 0; l < e->L; ++l)
    for (int j = 0; j < e->NJ; ++j) table[size_t(l) * e->NJ + j] = value(l, j);
  return table;
}
static std::vector<double> joint_offsets(const shc_engine *e) { // Joint::offset_
  return leg_joint_table(e, [&](int l, int j) { return e->params.joint[l][j].offset; });
}

extern "C" int shc_engine_set_joint_states_msg(shc_engine *e, const double *position, const double * /*velocity*/, const double *effort, int on_device) {
  SHC_ENTER_JOINED(e);
  HIP_TRY(hipSetDevice(e->device));
  if (position) {
    const std::vector<double> off = joint_offsets(e);
    HostCall hc(e);
    const double *d_off = hc.in(off.data(), off.size(), 0), *d = hc.in(position, size_t(e->n) * e->L * e->NJ, on_device);
    int rc = hc.status();
    if (rc != SHC_OK) return rc;
    const int64_t threads = e->n * e->L;
    store_measured_q_kernel<<<grid256(threads), dim3(256), 0, e->stream>>>(d, e->st.legd, e->n_slots, e->n, e->L, e->NJ, LEG_FIELD(e, MEAS_Q), d_off);
    if ((rc = hc.finish()) != SHC_OK) return rc;
  }
  return effort ? shc_engine_set_joint_effort(e, effort, on_device) : SHC_OK;
}

extern "C" int shc_engine_set_tip_states_msg(shc_engine *e, const double *wrench_force, const double *step_plane, int on_device) {
  SHC_ENTER_JOINED(e);
  int rc = SHC_OK;
  if (wrench_force && (rc = shc_engine_set_tip_force(e, wrench_force, on_device)) != SHC_OK) return rc;
  if (step_plane) {
    HIP_TRY(hipSetDevice(e->device));
    e->rt_flags |= RT_TOUCHDOWN; // setTouchdownDetection(true) (:1655)
    HostCall hc(e);
    const double *d = hc.in(step_plane, size_t(e->n) * e->L * 3, on_device);
    if ((rc = hc.status()) != SHC_OK) return rc;
    const int64_t threads = e->n * e->L;
    rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      step_plane_range_kernel<L, NJ><<<grid256(threads), dim3(256), 0, e->stream>>>(e->st, (const SharedConsts<L, NJ> *)e->d_consts, d);
      return SHC_OK;
    });
    if (rc != SHC_OK) return rc;
    return hc.finish();
  }
  return rc;
}

// ---- externally requested tip targets / default poses (rough terrain mode; struct ExternalTarget, walk_controller.h:38-46)
struct ExtRow { // shc_external_target as doubles (staged on the device)
  double pose[7], transform[7], swing_clearance, flags /* bit 0 defined, bit 1 odom_ideal */;
};
struct ExtAt { int base, flags; };
__host__ __device__ inline ExtAt ext_record(int which) { // 0 LegStepper::external_target_, 1 external_default_, 2 LegPoser::external_target_
  return which == 0 ? ExtAt{ExtFields::T_POSE, ExtFields::T_FLAGS} : which == 1 ? ExtAt{ExtFields::D_POSE, ExtFields::D_FLAGS} : ExtAt{ExtFields::P_POSE, ExtFields::P_FLAGS};
}
__global__ void set_external_kernel(DevState st, int L, int64_t first, int64_t count, int leg_sel, int which, const ExtRow *rows, int transform_only,
                                    unsigned long long *ignored, SeqRobotState *seq, int rough_terrain) {
  const int legs = leg_sel < 0 ? L : 1;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= count * legs) return;
  const int64_t rob = first + t / legs;
  const int leg = leg_sel < 0 ? int(t % legs) : leg_sel;
  const int64_t slot = slot_of(rob, leg, L);
  int base = ext_record(which).base, flags_at = ext_record(which).flags;
  auto f = [&](int field) -> double & { return st.ext[leg_field_index(field, slot, st.n_slots)]; };
  const ExtRow &r = rows[t];
  if (transform_only) { // generateExternalTargetTransforms (state_controller.cpp:703-773): only defined requests are refreshed
    if ((int(f(flags_at)) & 1) != 0)
      for (int k = 0; k < 7; ++k) f(base + 7 + k) = r.transform[k];
    return;
  }
  const int defined = int(r.flags) & 1;
  if (!defined) { // withdrawn: defined_ = false, the rest of the record stays
    f(flags_at) = double(int(f(flags_at)) & ~1);
    return;
  }
  // targetTipPoseCallback (:1734-1757): the LegStepper takes a request only while its robot is not STOPPED; the target of a robot
  // that stands goes to its LegPoser for planner mode (target_tip_pose_acquired_, :1738-1742), a default for it is dropped
  const int walk_state = st.robi[rob_index(rob, RobotFields::I_WORD, 64 / L, RobotFields::I_COUNT)] & 3;
  if (which == 2 || (which == 0 && walk_state == WS_STOPPED)) {
    which = 2;
    base = ext_record(2).base, flags_at = ext_record(2).flags;
    seq[rob].tip_pose_acquired = 1;
  } else if (walk_state == WS_STOPPED || !rough_terrain) { // (without rough_terrain_mode no stepper ever reads its requests)
    atomicAdd(ignored, 1ull);
    return;
  }
  for (int k = 0; k < 7; ++k) f(base + k) = r.pose[k], f(base + 7 + k) = r.transform[k];
  if (which == 0) f(ExtFields::T_CLEARANCE) = r.swing_clearance;
  if (which == 2) f(ExtFields::P_CLEARANCE) = r.swing_clearance;
  f(flags_at) = r.flags;
}
__global__ void get_external_kernel(DevState st, int L, int64_t first, int64_t count, int leg_sel, int which, ExtRow *rows) {
  const int legs = leg_sel < 0 ? L : 1;
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= count * legs) return;
  const int64_t slot = slot_of(first + t / legs, leg_sel < 0 ? int(t % legs) : leg_sel, L);
  const int base = ext_record(which).base;
  auto f = [&](int field) { return st.ext[leg_field_index(field, slot, st.n_slots)]; };
  ExtRow &r = rows[t];
  for (int k = 0; k < 7; ++k) r.pose[k] = f(base + k), r.transform[k] = f(base + 7 + k);
  r.swing_clearance = which == 0 ? f(ExtFields::T_CLEARANCE) : which == 2 ? f(ExtFields::P_CLEARANCE) : 0.0;
  r.flags = f(ext_record(which).flags);
}

static int ensure_seq(shc_engine *e);
static int ensure_manual(shc_engine *e);
static int ensure_manual_records(shc_engine *e);
static int external_select(shc_engine *e, int which, int64_t first, int64_t count, int leg, int64_t *rows_out) {
  if (which != SHC_EXTERNAL_TARGET && which != SHC_EXTERNAL_DEFAULT && which != SHC_EXTERNAL_PLANNER_TARGET)
    return fail(SHC_ERR_INVALID_ARG, "which must be SHC_EXTERNAL_TARGET, SHC_EXTERNAL_DEFAULT or SHC_EXTERNAL_PLANNER_TARGET");
  if (first < 0 || count < 0 || first + count > e->n || leg >= e->L) return fail(SHC_ERR_INVALID_ARG, "instance range / leg out of bounds");
  if (which == SHC_EXTERNAL_DEFAULT && !e->params.rough_terrain_mode)
    return fail(SHC_ERR_UNSUPPORTED, "external default poses are read in rough_terrain_mode only (walk_controller.cpp:988)");
  *rows_out = count * (leg < 0 ? e->L : 1);
  HIP_TRY(hipSetDevice(e->device));
  if (which != SHC_EXTERNAL_DEFAULT) { // a target may end up with the planner-mode LegPoser of a robot that stands
    const int rc = ensure_seq(e);
    if (rc != SHC_OK) return rc;
  }
  if (!e->st.ext) { // first request: allocate the records (all undefined)
    const size_t bytes = size_t(ExtFields::COUNT) * e->n_slots * 8;
    HIP_TRY(hipMalloc(&e->st.ext, bytes));
    HIP_TRY(hipMemsetAsync(e->st.ext, 0, bytes, e->stream));
  }
  return SHC_OK;
}

static int external_write(shc_engine *e, int which, int64_t first, int64_t count, int leg, const std::vector<ExtRow> &host, int transform_only,
                          int64_t *ignored) {
  unsigned long long h_ignored = 0;
  HostCall hc(e);
  const ExtRow *d_rows = hc.in(host.data(), host.size(), 0);
  unsigned long long *d_ignored = hc.out(&h_ignored, 1, 0);
  if (const int rc = hc.status()) return rc;
  HIP_TRY(hipMemsetAsync(d_ignored, 0, 8, e->stream));
  set_external_kernel<<<grid256(int64_t(host.size())), dim3(256), 0, e->stream>>>(e->st, e->L, first, count, leg, which, d_rows, transform_only, d_ignored, e->d_seq, e->params.rough_terrain_mode);
  if (const int rc = hc.finish()) return rc;
  if (ignored) *ignored = int64_t(h_ignored);
  return SHC_OK;
}

extern "C" int shc_engine_set_external_target(shc_engine *e, int which, int64_t first, int64_t count, int leg, const shc_external_target *rows,
                                              int64_t *ignored) {
  SHC_ENTER_JOINED(e);
  int64_t n_rows = 0;
  int rc = external_select(e, which, first, count, leg, &n_rows);
  if (rc != SHC_OK) return rc;
  if (!rows) return fail(SHC_ERR_INVALID_ARG, "rows is NULL");
  if (ignored) *ignored = 0;
  if (n_rows == 0) return SHC_OK;
  std::vector<ExtRow> host((size_t)n_rows);
  for (int64_t i = 0; i < n_rows; ++i) {
    const shc_external_target &t = rows[i];
    // (a requested target rotation on > 3-DOF legs becomes LegStepper::target_tip_pose_.rotation_: the cycle kernels with the
    //  tip-rotation logic run for such legs whenever rough terrain mode is on; legs with <= 3 joints never read it)
    for (int k = 0; k < 7; ++k) host[i].pose[k] = t.pose[k], host[i].transform[k] = t.transform[k];
    host[i].swing_clearance = t.swing_clearance;
    host[i].flags = double((t.defined ? 1 : 0) | (t.frame_is_odom_ideal ? 2 : 0));
  }
  e->rt_flags |= RT_EXTERNAL;
  return external_write(e, which, first, count, leg, host, 0, ignored);
}

extern "C" int shc_engine_set_external_transform(shc_engine *e, int which, int64_t first, int64_t count, int leg, const double *transform) {
  SHC_ENTER_JOINED(e);
  int64_t n_rows = 0;
  int rc = external_select(e, which, first, count, leg, &n_rows);
  if (rc != SHC_OK) return rc;
  if (!transform) return fail(SHC_ERR_INVALID_ARG, "transform is NULL");
  if (n_rows == 0) return SHC_OK;
  std::vector<ExtRow> host((size_t)n_rows);
  for (int64_t i = 0; i < n_rows; ++i)
    for (int k = 0; k < 7; ++k) host[i].transform[k] = transform[i * 7 + k];
  return external_write(e, which, first, count, leg, host, 1, nullptr);
}

extern "C" int shc_engine_get_external_target(shc_engine *e, int which, int64_t first, int64_t count, int leg, shc_external_target *rows) {
  SHC_ENTER_JOINED(e);
  int64_t n_rows = 0;
  int rc = external_select(e, which, first, count, leg, &n_rows);
  if (rc != SHC_OK) return rc;
  if (!rows) return fail(SHC_ERR_INVALID_ARG, "rows is NULL");
  if (n_rows == 0) return SHC_OK;
  std::vector<ExtRow> host((size_t)n_rows);
  if ((rc = gather_output(e, host.data(), host.size(), 0, [&](ExtRow *d_rows) {
         get_external_kernel<<<grid256(n_rows), dim3(256), 0, e->stream>>>(e->st, e->L, first, count, leg, which, d_rows);
       })) != SHC_OK)
    return rc;
  for (int64_t i = 0; i < n_rows; ++i) {
    for (int k = 0; k < 7; ++k) rows[i].pose[k] = host[i].pose[k], rows[i].transform[k] = host[i].transform[k];
    rows[i].swing_clearance = host[i].swing_clearance;
    rows[i].defined = int(host[i].flags) & 1;
    rows[i].frame_is_odom_ideal = (int(host[i].flags) >> 1) & 1;
  }
  return SHC_OK;
}

#include "shc_footholds.hpp" // the three calls above for every robot from / into one dense [n][F] device array: shc_engine_set_footholds / _get_footholds
#include "shc_reach.hpp"     // which of C candidate tip targets per robot every leg can reach, by the IK line search, nothing written: shc_engine_probe_reach
#include "shc_step_plan.hpp" // every LegStepper's Bezier nodes, stride, clearance and remaining tip path as rows, nothing written: shc_engine_get_step_plan

extern "C" int shc_engine_get_joint_commands(shc_engine *e, double *position, double *velocity, double *effort, double *position_command, int on_device) {
  SHC_ENTER_JOINED(e);
  HIP_TRY(hipSetDevice(e->device));
  const std::vector<double> off = joint_offsets(e);
  const size_t rows = size_t(e->n) * e->L * e->NJ;
  HostCall hc(e);
  const double *d_off = hc.in(off.data(), off.size(), 0);
  double *out[4] = {position, velocity, effort, position_command}, *dev[4];
  for (int k = 0; k < 4; ++k) dev[k] = hc.out(out[k], rows, on_device);
  if (const int rc = hc.status()) return rc;
  const int64_t threads = e->n * e->L;
  joint_commands_kernel<<<grid256(threads), dim3(256), 0, e->stream>>>(dev[0], dev[1], dev[2], dev[3], e->st.legd, e->n_slots, e->n, e->L, e->NJ, LEG_FIELD(e, Q),
                                                                    LEG_FIELD(e, QD), LEG_FIELD(e, EFFORT_IN), d_off);
  return hc.finish();
}

// ---- per-leg Leg API (include/shc_batch.h "Per-leg methods")
struct LegCall {
  LegSel sel;
  int64_t rows; // count * selected legs
  int init(shc_engine *e, int64_t first, int64_t count, int leg) {
    if (first < 0 || count < 0 || first + count > e->n) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
    if (leg < -1 || leg >= e->L) return fail(SHC_ERR_INVALID_ARG, "leg out of range (-1 = every leg)");
    sel = LegSel{first, count, leg, e->L};
    rows = count * (leg < 0 ? e->L : 1);
    HIP_TRY(hipSetDevice(e->device));
    return SHC_OK;
  }
  dim3 grid() const { return dim3((unsigned)((rows + 63) / 64)); }
};
#define LEG_KERNEL(KERNEL, ...)                                                                                              \
  dispatch_morphology(e, [&](auto l_, auto nj_) -> int {                                                                        \
    constexpr int L_ = decltype(l_)::value, NJ_ = decltype(nj_)::value;                                                      \
    if (c.rows) KERNEL<L_, NJ_><<<c.grid(), dim3(64), 0, e->stream>>>(e->st, (const SharedConsts<L_, NJ_> *)e->d_consts, c.sel, __VA_ARGS__); \
    return SHC_OK;                                                                                                           \
  })

extern "C" int shc_leg_set_desired_tip_pose(shc_engine *e, int64_t first, int64_t count, int leg, const double *tip_pose, int apply_delta,
                                            int on_device) {
  SHC_ENTER_JOINED(e);
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  if (!tip_pose && (rc = derive_tips(e)) != SHC_OK) return rc; // Pose::Undefined() = "the poser's tip pose" (model.cpp:657)
  HostCall hc(e);
  const double *d = hc.in(tip_pose, size_t(c.rows) * 7, on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_set_desired_kernel, d, apply_delta, e->params.admittance_control, rotations_tracked(e))) != SHC_OK) return rc;
  return hc.finish();
}

extern "C" int shc_leg_solve_ik(shc_engine *e, int64_t first, int64_t count, int leg, const double *delta, int solve_rotation,
                                double *joint_delta, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!delta || !joint_delta) return fail(SHC_ERR_INVALID_ARG, "delta / joint_delta is NULL");
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(delta, size_t(c.rows) * 6, on_device);
  double *o = hc.out(joint_delta, size_t(c.rows) * e->NJ, on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_solve_ik_kernel, d, solve_rotation, o)) != SHC_OK) return rc;
  return hc.finish();
}

extern "C" int shc_leg_update_joint_positions(shc_engine *e, int64_t first, int64_t count, int leg, const double *joint_delta, int simulation,
                                              double *limit_proximity, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!joint_delta) return fail(SHC_ERR_INVALID_ARG, "joint_delta is NULL");
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(joint_delta, size_t(c.rows) * e->NJ, on_device);
  double *o = hc.out(limit_proximity, size_t(c.rows), on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_update_joints_kernel, d, simulation, o, e->params.time_delta, e->params.clamp_joint_velocities,
                       e->params.clamp_joint_positions)) != SHC_OK)
    return rc;
  return hc.finish();
}

extern "C" int shc_leg_apply_ik(shc_engine *e, int64_t first, int64_t count, int leg, int simulation, double *ik_result, int on_device) {
  SHC_ENTER_JOINED(e);
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  double *o = hc.out(ik_result, size_t(c.rows), on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_apply_ik_kernel, simulation, o, e->params.time_delta, e->params.clamp_joint_velocities,
                       e->params.clamp_joint_positions, e->cp.tip_force, e->params.force_gain)) != SHC_OK)
    return rc;
  return hc.finish();
}

extern "C" int shc_leg_apply_fk(shc_engine *e, int64_t first, int64_t count, int leg, const double *joint_position, double *tip_pose,
                                int on_device) {
  SHC_ENTER_JOINED(e);
  if (!tip_pose) return fail(SHC_ERR_INVALID_ARG, "tip_pose is NULL");
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(joint_position, size_t(c.rows) * e->NJ, on_device);
  double *o = hc.out(tip_pose, size_t(c.rows) * 7, on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_apply_fk_kernel, d, o)) != SHC_OK) return rc;
  return hc.finish();
}

// ---- sequences
extern "C" int shc_leg_step_to_position(shc_engine *e, int64_t first, int64_t count, int leg, const double *target_tip_pose, const double *target_pose,
                                        double lift_height, double time_to_step, int apply_delta, double *tip_pose, int32_t *progress, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!target_pose || !tip_pose) return fail(SHC_ERR_INVALID_ARG, "target_pose / tip_pose is NULL");
  if (!(time_to_step >= 0.0)) return fail(SHC_ERR_INVALID_ARG, "time_to_step must be >= 0");
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *dt = hc.in(target_tip_pose, size_t(c.rows) * 7, on_device);
  const double *dp = hc.in(target_pose, size_t(count) * 7, on_device); // one row per INSTANCE
  double *o = hc.out(tip_pose, size_t(c.rows) * 7, on_device);
  int32_t *prog = hc.out(progress, size_t(c.rows), on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_step_to_position_kernel, dt, dp, lift_height, time_to_step, apply_delta, e->params.admittance_control,
                       e->params.time_delta, o, prog)) != SHC_OK)
    return rc;
  return hc.finish();
}

extern "C" int shc_leg_transition_configuration(shc_engine *e, int64_t first, int64_t count, int leg, const double *desired_configuration,
                                                double transition_time, int32_t *progress, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!desired_configuration) return fail(SHC_ERR_INVALID_ARG, "desired_configuration is NULL");
  LegCall c;
  int rc = c.init(e, first, count, leg);
  if (rc != SHC_OK) return rc;
  HostCall hc(e);
  const double *d = hc.in(desired_configuration, size_t(c.rows) * e->NJ, on_device);
  int32_t *prog = hc.out(progress, size_t(c.rows), on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  if ((rc = LEG_KERNEL(leg_transition_configuration_kernel, d, 1, transition_time, e->params.time_delta, prog)) != SHC_OK) return rc;
  return hc.finish();
}

#include "shc_loop_calls.hpp" // every StateController::loop() that is not the plain control cycle: start-ups, sequences, leg toggles, plan steps, pack / unpack

#include "shc_snapshot.hpp" // shc_engine_get_state / set_state, auxiliary state: kernels and host side
#include "shc_checkpoint.hpp" // device checkpoints and the indexed restore (shc_engine_checkpoint_*, shc_engine_restore_instances)

extern "C" int shc_engine_get_body_state(shc_engine *e, double *pose, double *velocity, int32_t *walk_state, int on_device) {
  SHC_ENTER_JOINED(e);
  int rc;
  if ((rc = gather_rob(e, pose, 7, RobotFields::CPOSE, on_device)) != SHC_OK) return rc;
  if ((rc = gather_rob(e, velocity, 3, RobotFields::VLIN, on_device)) != SHC_OK) return rc;
  return gather_output(e, walk_state, size_t(e->n), on_device, [&](int32_t *d) {
    gather_walk_state_kernel<<<grid256(e->n), dim3(256), 0, e->stream>>>(d, e->st.robi, 64 / e->L, e->n);
  });
}

#include "shc_fleet.hpp" // shc_fleet_*: mixed morphologies + multi-device sharding (uses the entry points above)
