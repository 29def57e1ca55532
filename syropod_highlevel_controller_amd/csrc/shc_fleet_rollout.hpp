// shc_fleet_rollout.hpp — shc_fleet_step_k_actions_device, shc_fleet_get_step_k_observations_device: the rollout tensors (shc_rollout.hpp) for a
// mixed fleet, in the caller's instance order.  Included by shc_fleet.hpp behind shc_fleet_step_k.hpp and shc_fleet_actions.hpp; uses the
// readiness check, ids and ordering calls of shc_fleet_io.hpp and the K-deep staging of shc_fleet_step_k.hpp.
//
// shc_fleet_step_k packs float64 record arrays; here robot r of a part reads row ids[r] of every cycle of the caller's [K][n][A] array - the
// part's caller ids (fleet_part_ids, the table device I/O keeps on the device) are the kernels' row table.  Per part and call: one launch of
// rollout_stage_kernel into the part's K-deep staging (the buffer shc_fleet_step_k uses, with its rules: grown on demand, counted by
// shc_fleet_io_bytes, joined before it is overwritten), one shc_engine_step_k on it, and for the way back one launch of rollout_joints_kernel
// out of the part's ring, all on the part's stream.  The rows of the parts are disjoint, so the parts' streams need no order among themselves.
// The rollout kinematics (shc_rollout_kin.hpp: shc_fleet_get_step_k_kinematics_device, shc_fleet_scan_step_k_health_device) are read launches of
// the same kind: one per part, the part's caller ids as the row / record table, nothing staged.
#pragma once

extern "C" int shc_fleet_step_k_actions_device(shc_fleet *f, int n_cycles, const shc_act_spec *spec, const void *actions, int64_t cycle_stride) {
  RowLayout lay;
  // every part is asked before the first launch and before anything is allocated (what is wrong with the call itself is found at the first)
  int rc = fleet_rows_begin<ActRows>(f, spec, actions, "actions", lay, [&](const shc_engine *e) {
    const char *who = "shc_fleet_step_k_actions_device";
    const int bad = rollout_actions_call_check(who, spec, lay, n_cycles, f->n, cycle_stride);
    return bad != SHC_OK ? bad : rollout_actions_engine_check(who, e, spec, lay, n_cycles);
  });
  if (rc != SHC_OK) return rc;
  rc = fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    shc_engine *e = p.engine;
    HIP_TRY(hipSetDevice(p.device));
    int part = rollout_stage_room(e, p.k_stage, p.k_stage_bytes, size_t(rollout_plan(e, lay, n_cycles).doubles) * 8);
    // the halves of an earlier split launch may still be reading the rows this call is about to overwrite: the part's stream follows them first
    if (part == SHC_OK && e->side_busy) part = shc_engine_join(e);
    shc_cycle_inputs staged;
    if (part == SHC_OK)
      part = rollout_stage_launch(e, spec, lay, actions, stride, cycle_stride ? cycle_stride : f->n * stride, p.d_ids, n_cycles, reinterpret_cast<double *>(p.k_stage), staged);
    return part != SHC_OK ? part : shc_engine_step_k(e, n_cycles, &staged);
  });
  if (rc == SHC_OK) f->k_cycles = n_cycles;
  return rc;
}

// The K of the fleet's latest K-cycle launch, 0 when the ring of a part does not hold it
static int fleet_rollout_cycles(const shc_fleet *f) {
  for (const auto &p : f->parts) // (a part stepped on its own since, through shc_fleet_part: its ring holds another launch)
    if (!p.engine->k_out || p.engine->k_out_cycles != f->k_cycles) return 0;
  return f->k_cycles;
}

// The read of the parts' rings as rows, for the two entry points that differ in the fields they let through (rollout_read of shc_rollout.hpp)
static int fleet_rollout_read(shc_fleet *f, const char *who, uint32_t readable, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  RowLayout lay;
  int rc = fleet_rows_begin<ObsRows>(f, spec, out, "out", lay, [&](const shc_engine *e) { return rollout_joints_check(e, spec, lay, readable); });
  if (rc != SHC_OK) return rc;
  if ((rc = rollout_range_check(who, fleet_rollout_cycles(f), first_cycle, n_cycles)) != SHC_OK) return rc;
  if ((rc = rollout_stride_check(who, f->n, row_stride_of(spec, lay), cycle_stride)) != SHC_OK) return rc;
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const int rc = fleet_part_join(p); // split launches: the part's stream follows both halves before it reads their ring
    return rc != SHC_OK ? rc : rollout_joints_launch(p.engine, spec, lay, out, stride, cycle_stride ? cycle_stride : f->n * stride, p.d_ids, first_cycle, n_cycles);
  });
}
extern "C" int shc_fleet_get_step_k_observations_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  return fleet_rollout_read(f, "shc_fleet_get_step_k_observations_device", kRingJoints, first_cycle, n_cycles, spec, out, cycle_stride);
}
// ... and the rollout kinematics (shc_rollout_kin.hpp): model_tip = FK(q) beside the joints, from the same kernel
extern "C" int shc_fleet_get_step_k_kinematics_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out, int64_t cycle_stride) {
  return fleet_rollout_read(f, "shc_fleet_get_step_k_kinematics_device", kRingKinematics, first_cycle, n_cycles, spec, out, cycle_stride);
}

// The joint-limit records of every cycle: one launch of rollout_health_kernel per part on the part's stream, record (k, ids[r]) and first_hit[ids[r]]
// for robot r of the part - the caller's order without staging.
extern "C" int shc_fleet_scan_step_k_health_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_health_criteria *criteria, shc_robot_health *health,
                                                   int32_t *first_hit) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  shc_health_criteria crit;
  int rc = rollout_health_call_check(criteria, health, first_hit, crit);
  if (rc == SHC_OK) rc = fleet_io_ready(f);
  if (rc == SHC_OK) rc = rollout_range_check("shc_fleet_scan_step_k_health_device", fleet_rollout_cycles(f), first_cycle, n_cycles);
  if (rc == SHC_OK) rc = fleet_io_prepare(f);
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i) {
    FleetPart &p = f->parts[i];
    if ((rc = fleet_part_join(p)) == SHC_OK) rc = rollout_health_launch(p.engine, crit, health, first_hit, f->n, p.d_ids, first_cycle, n_cycles);
  }
  return rc;
}
