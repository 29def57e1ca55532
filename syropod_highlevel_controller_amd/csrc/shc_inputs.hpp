// shc_inputs.hpp — the eight input groups of a cycle, described once: what each is (per robot or per leg, its width, where it is stored, which
// bound-set entry and resident group it is, which group it is given together with), the member of shc_cycle_inputs and of shc_fleet_inputs that
// carries it, the rules every route into the cycle asks of a set of groups, and the K-deep staging of the groups a K-cycle launch is given.
// Included by shc_engine.hip ahead of the setters, and by nothing the cycle kernels are built from.  Every route reads this table: the setters,
// the action pass (shc_actions.hpp), the rollout tensors (shc_rollout.hpp), resident posts / bound sets / shc_engine_step_k (shc_resident.hpp)
// and the fleet's host and device forms (shc_fleet.hpp, shc_fleet_io.hpp, shc_fleet_step_k.hpp).
#pragma once

// The groups are numbered by SHC_ACT_*: six per robot, then the two per leg.  All but the two pose groups can be bound, K-deep or directly posted.
constexpr int kInputGroups = SHC_ACT_FIELD_COUNT, kRobotInputGroups = SHC_ACT_TIP_FORCE;
static_assert(kRobotInputGroups == 6 && SHC_ACT_JOINT_EFFORT == 7 && kInputGroups == 8, "six per-robot groups, then tip force and joint effort");
constexpr uint32_t kPoseInputs = 1u << SHC_ACT_POSE_TRANSLATION_VELOCITY | 1u << SHC_ACT_POSE_ROTATION_VELOCITY, kAllInputs = (1u << kInputGroups) - 1u;

struct InputGroup {
  int width;     // doubles per robot (per-robot groups) or per leg (0: the longest leg's DOF)
  int field;     // per-robot groups: the robot field of the first component (per-leg groups: input_leg_field)
  int bound, rg; // BND_* (-1: none) and RG_*
  int with;      // the group it is given together with (its own number: none)
};
__host__ __device__ constexpr InputGroup input_group(int g) {
  using R = RobotFields;
  switch (g) {
  case SHC_ACT_LINEAR_XY: return {2, R::VIN, BND_LIN, RG_VEL, SHC_ACT_ANGULAR};
  case SHC_ACT_ANGULAR: return {1, R::WIN, BND_ANG, RG_VEL, SHC_ACT_LINEAR_XY};
  case SHC_ACT_IMU_ORIENTATION: return {4, R::IMUQ, BND_IMUQ, RG_IMU, SHC_ACT_IMU_ANGULAR_VELOCITY};
  case SHC_ACT_IMU_ANGULAR_VELOCITY: return {3, R::GYRO, BND_IMUW, RG_IMU, SHC_ACT_IMU_ORIENTATION};
  case SHC_ACT_POSE_TRANSLATION_VELOCITY: return {3, R::TVI, -1, RG_POSE, SHC_ACT_POSE_ROTATION_VELOCITY};
  case SHC_ACT_POSE_ROTATION_VELOCITY: return {3, R::RVI, -1, RG_POSE, SHC_ACT_POSE_TRANSLATION_VELOCITY};
  case SHC_ACT_TIP_FORCE: return {3, -1, BND_FORCE, RG_FORCE, SHC_ACT_TIP_FORCE};
  default: return {0, -1, BND_EFFORT, RG_EFFORT, SHC_ACT_JOINT_EFFORT};
  }
}
__host__ __device__ constexpr bool input_per_leg(int g) { return g >= kRobotInputGroups; }
// doubles of a group per robot or per leg, and per robot in all; the padded caller side of a fleet: (max_legs, max_dof)
__host__ __device__ constexpr int input_k(int g, int dof) { return input_group(g).width ? input_group(g).width : dof; }
__host__ __device__ constexpr int input_width(int g, int legs, int dof) { return (input_per_leg(g) ? legs : 1) * input_k(g, dof); }
// (the accessors the row kernels call inside unrolled loops, g < kRobotInputGroups)
__host__ __device__ constexpr int act_robot_width(int g) { return input_group(g).width; }
__host__ __device__ constexpr int act_robot_field(int g) { return input_group(g).field; }
// the leg field the first component of a per-leg group is stored at
template <int NJ>
__host__ __device__ constexpr int input_leg_field(int g) {
  return g == SHC_ACT_TIP_FORCE ? Fields<NJ>::FORCE_IN : Fields<NJ>::EFFORT_IN;
}

// The member of each struct that carries group g (shc_fleet_inputs is these eight pointers and nothing else)
static const double *shc_cycle_inputs::*const kCycleInput[kInputGroups] = {
    &shc_cycle_inputs::linear_xy,  &shc_cycle_inputs::angular, &shc_cycle_inputs::imu_orientation_wxyz, &shc_cycle_inputs::imu_angular_velocity, &shc_cycle_inputs::pose_translation_velocity,
    &shc_cycle_inputs::pose_rotation_velocity, &shc_cycle_inputs::tip_force, &shc_cycle_inputs::joint_effort};
static const double *shc_fleet_inputs::*const kFleetInput[kInputGroups] = {
    &shc_fleet_inputs::linear_xy,  &shc_fleet_inputs::angular, &shc_fleet_inputs::imu_orientation_wxyz, &shc_fleet_inputs::imu_angular_velocity, &shc_fleet_inputs::pose_translation_velocity,
    &shc_fleet_inputs::pose_rotation_velocity, &shc_fleet_inputs::tip_force, &shc_fleet_inputs::joint_effort};
static_assert(sizeof(shc_fleet_inputs) == kInputGroups * sizeof(double *), "shc_fleet_inputs is eight pointers");
// The groups present (bit g: group g; NULL struct: none), and the resident groups of a set of groups
template <class In>
static unsigned input_mask(const In *in, const double *In::*const (&member)[kInputGroups]) {
  unsigned mask = 0;
  for (int g = 0; in && g < kInputGroups; ++g) mask |= unsigned(in->*member[g] != nullptr) << g;
  return mask;
}
static unsigned input_mask(const shc_cycle_inputs *in) { return input_mask(in, kCycleInput); }
static unsigned input_mask(const shc_fleet_inputs *in) { return input_mask(in, kFleetInput); }
static unsigned input_resident_groups(unsigned mask) {
  unsigned rg = 0;
  for (int g = 0; g < kInputGroups; ++g)
    if (mask >> g & 1u) rg |= 1u << input_group(g).rg;
  return rg;
}

// ---- the rules
// Paired groups `among` those named are given together; `how` is the caller's verb ("given", "bound", "posted")
static int input_pairs_check(unsigned mask, unsigned among, const char *how) {
  for (int g = 0; g < kInputGroups; ++g)
    if ((among >> g & 1u) && (mask >> g & 1u) != (mask >> input_group(g).with & 1u))
      return fail(SHC_ERR_INVALID_ARG, g < SHC_ACT_IMU_ORIENTATION   ? std::string("linear_xy and angular are ") + how + " together"
                                       : g < SHC_ACT_POSE_TRANSLATION_VELOCITY ? std::string("the two IMU arrays are ") + how + " together"
                                                                                : std::string("the two pose input arrays are ") + how + " together");
  return SHC_OK;
}
// A K-cycle launch carries no pose group (reset_modes: the caller's struct has reset modes, and they are given)
static int k_launch_pose_check(const char *who, unsigned mask, bool reset_modes = false) {
  if ((mask & kPoseInputs) || reset_modes)
    return fail(SHC_ERR_UNSUPPORTED, std::string(who) + " carries velocity, IMU, tip force and joint effort; give pose inputs / reset modes with their setters before the call (held for the K cycles)");
  return SHC_OK;
}
// What is refused of a K-cycle launch, one plain question each (every entry point asks them in the order it has always asked them in; `who` is
// the entry point's name and the message is built only where one fails)
constexpr size_t kKLaunchMaxBytes = size_t(1) << 31; // the output ring and the K-deep staging both stay below 2 GiB
static int k_launch_cycles_check(const char *who, int K) { return K < 1 || K > 4096 ? fail(SHC_ERR_INVALID_ARG, std::string(who) + ": 1 .. 4096 cycles per launch") : SHC_OK; }
static int k_launch_running_check(const shc_engine *e, const char *who) {
  return e->starting_up ? fail(SHC_ERR_UNSUPPORTED, std::string(who) + ": the K-cycle launches start from a running engine (finish the start-up first)") : SHC_OK;
}
static int k_launch_ring_check(const shc_engine *e, const char *who, int K) {
  if (size_t(e->NJ) * e->n_slots * 16 * size_t(K) < kKLaunchMaxBytes) return SHC_OK;
  return fail(SHC_ERR_INVALID_ARG, std::string(who) + ": cycles x batch - the output ring must stay below 2 GiB (fewer cycles per launch)");
}
// ... and what an engine refuses of one that stages `staging_doubles` doubles, asked before anything is staged: running, ring, staging, fit
static int resident_fit(const shc_engine *e, ResidentFit &fit);
static int k_launch_engine_check(const shc_engine *e, const char *who, int K, int64_t staging_doubles) {
  if (const int rc = k_launch_running_check(e, who)) return rc;
  if (const int rc = k_launch_ring_check(e, who, K)) return rc;
  if (size_t(staging_doubles) * 8 >= kKLaunchMaxBytes)
    return fail(SHC_ERR_INVALID_ARG, std::string(who) + ": cycles x batch x the groups given - the K-deep staging must stay below 2 GiB (fewer cycles per launch)");
  ResidentFit fit;
  return resident_fit(e, fit);
}

// ---- K-deep staging: the groups of `mask`, each a dense [K][rows][width] array of doubles, one behind the other in table order
struct InputPlan {
  int64_t at[kInputGroups]; // doubles from the start of staging (-1: not selected)
  int64_t doubles;
};
static InputPlan input_plan(unsigned mask, int64_t rows, int L, int NJ, int K) {
  InputPlan p{};
  for (int g = 0; g < kInputGroups; ++g) {
    p.at[g] = -1;
    if (!(mask >> g & 1u)) continue;
    p.at[g] = p.doubles;
    p.doubles += int64_t(K) * rows * input_width(g, L, NJ);
  }
  return p;
}
// ... and the device arrays of a plan over staging at `base`, as the engine's calls take them
static shc_cycle_inputs input_plan_arrays(const InputPlan &p, const double *base) {
  shc_cycle_inputs in{};
  for (int g = 0; g < kInputGroups; ++g)
    if (p.at[g] >= 0) in.*kCycleInput[g] = base + p.at[g];
  in.on_device = 1;
  return in;
}
