// shc_rollout_kin.hpp — rollout kinematics: what is a pure function of the joints a K-cycle launch left in its output ring, per cycle, without a
// cycle kernel touched.  shc_engine_get_step_k_kinematics hands model_tip = FK(q) back beside q / qd as one dense [cycles][n][D] array,
// shc_engine_scan_step_k_health the joint-limit half of the health record of every robot and cycle and the first cycle a robot was selected in.
// Included by shc_engine.hip behind shc_rollout.hpp (uses its ring read, range check and rollout_joints_kernel, RowGroup of shc_rows.hpp,
// leg_health / robot_health of shc_health.hpp, Group of shc_cycle.hpp, load_leg_fields of shc_leg_msgs.hpp and the entry-point macros).  The
// fleet forms (shc_fleet_rollout.hpp) launch the same kernels with a part's caller ids as the row / record table.
//
//   TIPS     rollout_joints_kernel itself (shc_rollout.hpp): its TIPS instance adds derived_model_tip on the q of the slot, the function
//            observe_kernel runs on the stored q - this entry point lets the field through, shc_engine_get_step_k_observations keeps refusing it.
//   HEALTH   rollout_health_kernel below: leg_health on (q, qd) of the slot with the tips, the admittance delta and the IK bit the ring does not
//            hold set to what shc_debug_robot_health is given by the definition (model tip = poser tip, no delta, no IK failure, a finite pose).
// Neither writes into an engine.
#pragma once

// The health kernel's view of a call
struct RolloutHealthArgs {
  int64_t n, n_slots;   // robots and leg slots of the engine
  int64_t rows;         // records per cycle of the caller's array: the engine's n, or the fleet's
  int32_t first_cycle;  // of ring slot 0 as the kernel sees it: first_hit counts from the launch's first cycle
  int32_t n_cycles;
};

// The geometry of health_scan_kernel (RowGroup, the per-leg figures met over the L lanes of a robot through Group<L>, a wavefront's 32-byte
// records through an LDS strip as 16-byte stores).  One workgroup per robot group walks the requested cycles - a wave-uniform loop over kernel
// arguments - with the planes of slot k + 1 requested before slot k is evaluated; `ring` is the slot of the first requested cycle.  The first
// cycle with flags & select != 0 stays in a register and goes out once behind the loop: one launch, no atomics, nothing to initialise, and the
// same bytes on every run.  Record (k, i) lies at health[k * rows + i], i = ids[robot] (a fleet part's caller ids) or the robot's own index;
// without ids the stores of a wavefront are one contiguous run.  The strip is double-buffered: one barrier per cycle orders the stores of cycle
// k + 2 behind the reads of cycle k.
template <int L, int NJ>
__global__ __launch_bounds__(64) void rollout_health_kernel(ulonglong2 *__restrict__ health, int32_t *__restrict__ first_hit, const double2 *__restrict__ ring,
                                                            const SharedConsts<L, NJ> *__restrict__ gc, const shc_health_criteria crit, const RolloutHealthArgs a,
                                                            const int64_t *__restrict__ ids) {
  using FD = Fields<NJ>;
  static_assert(FD::Q == 0 && FD::QD == NJ, "a ring slot holds the planes of Q and QD");
  constexpr int rpw = 64 / L;
  __shared__ ulonglong2 strip[2][2 * rpw];
  const RowGroup<L> rg(0, a.n);
  // (every lane of the wavefront takes part in the cross-lane reads; the lanes past the last group read group 0 and are not used)
  const Group<L> grp{rg.gi < rpw ? rg.gi * L : 0};
  const bool leader = rg.live && rg.leg == 0;
  const bool writer = rg.lane < 2 * rg.n_rob; // lane 2 r + h stores half h of the record of the block's robot r
  int64_t record = 0;
  if (writer) {
    const int64_t rob = rg.rob_lo + (rg.lane >> 1);
    record = ids ? ids[rob] : rob;
  }
  const int64_t slot_planes = int64_t(NJ) * a.n_slots;
  const V3 none{0.0, 0.0, 0.0};

  double next[2 * NJ];
#pragma unroll
  for (int j = 0; j < 2 * NJ; ++j) next[j] = 0.0;
  if (rg.live) load_leg_fields<FD::Q, 2 * NJ>(ring, a.n_slots, rg.slot, next);
  int hit = -1;
  for (int k = 0; k < a.n_cycles; ++k) {
    double q[NJ], qd[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = next[j], qd[j] = next[NJ + j];
    if (rg.live && k + 1 < a.n_cycles) load_leg_fields<FD::Q, 2 * NJ>(ring + (k + 1) * slot_planes, a.n_slots, rg.slot, next);
    LegHealth lh{1.0, 0.0, 0.0, 0u};
    if (rg.live) lh = leg_health<NJ>(gc->leg[rg.leg], q, qd, none, none, none, none, true, false);
    const shc_robot_health rec = robot_health(
        L, [&](int l) { return LegHealth{grp.get(lh.proximity, l), grp.get(lh.deviation, l), grp.get(lh.speed_ratio, l), uint32_t(grp.get(int(lh.bits), l))}; },
        true, crit);
    if (hit < 0 && (rec.flags & crit.select) != 0) hit = a.first_cycle + k;
    if (health != nullptr) {
      ulonglong2 *s = strip[k & 1];
      if (leader) {
        s[2 * rg.gi] = ulonglong2{(unsigned long long)__double_as_longlong(rec.min_limit_proximity), (unsigned long long)__double_as_longlong(rec.max_tip_deviation)};
        s[2 * rg.gi + 1] = ulonglong2{(unsigned long long)__double_as_longlong(rec.max_speed_ratio), (unsigned long long)rec.flags | ((unsigned long long)rec.leg_masks << 32)};
      }
      __syncthreads();
      if (writer) health[2 * (k * a.rows + record) + (rg.lane & 1)] = s[2 * rg.g0 + rg.lane];
    }
  }
  if (first_hit != nullptr && leader) first_hit[ids ? ids[rg.rob] : rg.rob] = hit;
}

// ---- host side
// What is wrong with a health call whoever makes it, and `crit`, the criteria in force (NULL: select 0, thresholds no value passes)
static int rollout_health_call_check(const shc_health_criteria *criteria, const shc_robot_health *health, const int32_t *first_hit, shc_health_criteria &crit) {
  if (!health && !first_hit) return fail(SHC_ERR_INVALID_ARG, "health and first_hit are both NULL");
  crit = health_criteria(criteria);
  if (crit.reserved != 0) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.reserved must be 0");
  if (crit.select & ~kHealthAllFlags) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.select has bits outside SHC_HEALTH_*");
  if (crit.select & (SHC_HEALTH_IK_DEVIATION | SHC_HEALTH_TIP_DEVIATION))
    return fail(SHC_ERR_UNSUPPORTED, "the output ring of the K-cycle launches holds joints: SHC_HEALTH_IK_DEVIATION and SHC_HEALTH_TIP_DEVIATION cannot be watched per cycle");
  if ((reinterpret_cast<uintptr_t>(health) & 15) || (reinterpret_cast<uintptr_t>(first_hit) & 3))
    return fail(SHC_ERR_INVALID_ARG, "device buffers: health must be 16-byte aligned, first_hit 4-byte aligned");
  return SHC_OK;
}
// The health launch on the engine's stream: ring slots [first_cycle, first_cycle + n_cycles), record (k, ids[robot]) of [n_cycles][rows] (ids: a
// device table) or (k, robot).  The caller has checked everything, joined split steps and made the engine's device current.
static int rollout_health_launch(shc_engine *e, const shc_health_criteria &crit, shc_robot_health *health, int32_t *first_hit, int64_t rows, const int64_t *ids,
                                 int first_cycle, int n_cycles) {
  const RolloutHealthArgs a{e->n, e->n_slots, rows, first_cycle, n_cycles};
  const double2 *ring = reinterpret_cast<const double2 *>(e->k_out) + int64_t(first_cycle) * e->NJ * e->n_slots;
  const unsigned grid = row_grid(e->L, 0, e->n);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    rollout_health_kernel<L, NJ><<<dim3(grid), dim3(64), 0, e->stream>>>(reinterpret_cast<ulonglong2 *>(health), first_hit, ring, (const SharedConsts<L, NJ> *)e->d_consts, crit,
                                                                        a, ids);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

extern "C" int shc_engine_get_step_k_kinematics(shc_engine *e, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  return rollout_read(e, "shc_engine_get_step_k_kinematics", kRingKinematics, first_cycle, n_cycles, spec, out, cycle_stride);
}

extern "C" int shc_engine_scan_step_k_health(shc_engine *e, int first_cycle, int n_cycles, const shc_health_criteria *criteria, shc_robot_health *health,
                                             int32_t *first_hit) {
  SHC_ENTER(e);
  shc_health_criteria crit;
  int rc = rollout_health_call_check(criteria, health, first_hit, crit);
  if (rc != SHC_OK) return rc;
  if ((rc = rollout_range_check("shc_engine_scan_step_k_health", e->k_out ? e->k_out_cycles : 0, first_cycle, n_cycles)) != SHC_OK) return rc;
  if ((rc = join_side(e)) != SHC_OK) return rc; // split launches: the engine's stream follows both halves before it reads their ring
  HIP_TRY(hipSetDevice(e->device));
  return rollout_health_launch(e, crit, health, first_hit, e->n, nullptr, first_cycle, n_cycles);
}
