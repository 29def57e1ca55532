// shc_fleet_step_k.hpp — K cycles per launch for a mixed fleet, from K-deep device arrays in the caller's order: shc_fleet_step_k,
// shc_fleet_get_step_k_joints_device.  Included by shc_fleet.hpp behind shc_fleet_io.hpp, whose pack launch, grid rule, readiness checks, ids and
// ordering events it uses; the groups, their staging plan and what is refused of them are shc_inputs.hpp's.
//
// The cycle-by-cycle device route (shc_fleet_set_inputs_device, shc_fleet_step(1), shc_fleet_get_outputs_device) pays per part and CYCLE one pack
// launch, the engine's setters, the step, two engine gathers and two place launches.  Here a part and CALL pays one pack launch, one
// shc_engine_step_k and one place launch per requested array:
//   K-deep PACK   fleet_pack of shc_fleet_io.hpp - the one pack kernel, the cycle its blockIdx.z - with K cycles.  Group g of the caller is
//                 [K][n][src_robot] doubles; the part's rows of cycle k land at k_stage[g.dst + k * rows * legs * k_width ..], so that each staged
//                 group is the dense [K][rows][..] array shc_engine_step_k reads with its own kstride (rows x width).  Bytes are copied as they
//                 are: the engine normalises.
//   ring PLACE    reads the part's step_k output ring where it lies ([K][NJ planes][n_slots] double2, the leg state's own layout: leg_state_index)
//                 and writes whole rows of the caller's [cycle][n][max_legs][max_dof] buffer at ids[r], NaN where the morphology has no such leg
//                 or joint.  No dense copy in between: shc_engine_get_step_k_joint_state + fleet_place would move every joint twice and launch
//                 2 x cycles x parts times.
// Everything between the two - the batch kernel or the serial form, a pending adjusted parameter's first cycle, touchdown detection on fresh tip
// forces, the first-effort switch, the last row staying as the held input - is shc_engine_step_k's, unchanged.
//
// K-deep staging: one buffer per part next to io_stage, K x rows x (the widths of the groups GIVEN) doubles - fleet_input_plan: input_plan of
// shc_inputs.hpp for the part, the plan the rollout tensors stage by, and input_plan_arrays the shc_cycle_inputs over it -, allocated by the
// first call that needs it, grown (never shrunk) by a call that needs more, counted by shc_fleet_io_bytes, released with the fleet.  A call with
// the same or a smaller K and the same groups allocates nothing.  The part's launch reads it - on the two half streams when the part steps split
// (alone on its device, 4 096 wavefronts or more), which only a join orders behind the part's stream.  So before a pack overwrites it, a part
// with split launches in flight is joined (shc_engine_join: events, no host wait); before it is freed to grow, the part is joined and its stream
// drained, as step_k_out_ring does for the ring.  The caller's arrays are read by the pack alone, on the part's stream.
#pragma once

// PLACE out of the ring.  `ring` is the slot of the first requested cycle; cycle c (blockIdx.y, wave-uniform) lies c * cycle_words further and goes
// to dst + c * n * row.  One thread per word of a DESTINATION row, as fleet_place_kernel: a robot's stores are one contiguous run and every word
// of the row is written.  f0: the leg field of joint 0 (Q or QD).  Words are copied as 64-bit patterns.
// (The index walk is fleet_place_kernel's, written out again: shared through a load functor both kernels ran 1 - 2 % slower.)
__global__ void fleet_place_ring_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ ring, const int64_t *__restrict__ ids, int64_t rows, int64_t n,
                                        int64_t n_slots, int64_t cycle_words, int legs, int k, int f0, int dst_legs, int dst_k, uint64_t pad) {
  const uint32_t row = uint32_t(dst_legs * dst_k), dk = uint32_t(dst_k);
  const uint64_t *__restrict__ slot = ring + int64_t(blockIdx.y) * cycle_words;
  uint64_t *__restrict__ out = dst + int64_t(blockIdx.y) * n * row;
  const int64_t total = rows * row, stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t0 = int64_t(blockIdx.x) * blockDim.x; t0 < total; t0 += stride) {
    const int64_t r0 = t0 / row; // uniform over the workgroup
    const uint32_t u = uint32_t(t0 - r0 * row) + threadIdx.x, dr = u / row, c = u - dr * row, l = c / dk, j = c - l * dk;
    const int64_t r = r0 + dr;
    if (r >= rows) continue;
    uint64_t v = pad;
    if (l < uint32_t(legs) && j < uint32_t(k)) v = slot[leg_state_index(f0 + int(j), r, int(l), legs, n_slots)];
    out[ids[r] * row + c] = v;
  }
}

extern "C" int shc_fleet_step_k(shc_fleet *f, int n_cycles, const shc_fleet_inputs *rows) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  const char *who = "shc_fleet_step_k";
  const unsigned mask = input_mask(rows);
  int rc = k_launch_cycles_check(who, n_cycles);
  if (rc == SHC_OK) rc = input_pairs_check(mask, kAllInputs & ~kPoseInputs, "given");
  if (rc == SHC_OK) rc = k_launch_pose_check(who, mask);
  if (rc == SHC_OK) rc = fleet_io_ready(f);
  // every part is asked before the first launch (and before anything is allocated): what its shc_engine_step_k would refuse
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i)
    rc = k_launch_engine_check(f->parts[i].engine, who, n_cycles, fleet_input_plan(f, f->parts[i], mask, n_cycles).doubles);
  if (rc != SHC_OK || (rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  for (auto &p : f->parts) { // staging that is too small: drained (the part's launches may still read it), released, allocated again
    HIP_TRY(hipSetDevice(p.device));
    if ((rc = rollout_stage_room(p.engine, p.k_stage, p.k_stage_bytes, size_t(fleet_input_plan(f, p, mask, n_cycles).doubles) * 8)) != SHC_OK) return rc;
  }
  for (auto &p : f->parts) {
    if (mask == 0) { // every input is held
      if ((rc = shc_engine_step_k(p.engine, n_cycles, nullptr)) != SHC_OK) return rc;
      continue;
    }
    const InputPlan plan = fleet_input_plan(f, p, mask, n_cycles);
    HIP_TRY(hipSetDevice(p.device));
    // the halves of an earlier split shc_engine_step_k may still be reading the rows this pack is about to overwrite: the part's stream follows them first
    if (p.engine->side_busy && (rc = shc_engine_join(p.engine)) != SHC_OK) return rc;
    if ((rc = fleet_pack(f, p, rows, plan, n_cycles, reinterpret_cast<double *>(p.k_stage))) != SHC_OK) return rc;
    const shc_cycle_inputs staged = input_plan_arrays(plan, reinterpret_cast<const double *>(p.k_stage));
    if ((rc = shc_engine_step_k(p.engine, n_cycles, &staged)) != SHC_OK) return rc;
  }
  f->k_cycles = n_cycles;
  return SHC_OK;
}

extern "C" int shc_fleet_get_step_k_joints_device(shc_fleet *f, int first_cycle, int n_cycles, double *q, double *qd) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  if (!q && !qd) return fail(SHC_ERR_INVALID_ARG, "q and qd are both NULL");
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(qd)) & 7) return fail(SHC_ERR_INVALID_ARG, "q / qd must be 8-byte aligned");
  int rc = fleet_io_ready(f);
  if (rc != SHC_OK) return rc;
  const char *range = "shc_fleet_get_step_k_joints_device: cycles [first_cycle, first_cycle + n_cycles) of the K of the latest shc_fleet_step_k";
  if (f->k_cycles < 1 || first_cycle < 0 || n_cycles < 1 || first_cycle > f->k_cycles - n_cycles) return fail(SHC_ERR_INVALID_ARG, range);
  for (const auto &p : f->parts) // (a part stepped on its own since, through shc_fleet_part: its ring holds another launch)
    if (!p.engine->k_out || p.engine->k_out_cycles != f->k_cycles) return fail(SHC_ERR_INVALID_ARG, range);
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;

  for (auto &p : f->parts) {
    shc_engine *e = p.engine;
    const int64_t n_rows = int64_t(p.ids.size()), cycle_words = int64_t(e->NJ) * e->n_slots * 2;
    if ((rc = shc_engine_join(e)) != SHC_OK) return rc; // split launches: the part's stream follows both halves before it reads their ring
    HIP_TRY(hipSetDevice(p.device));
    const uint64_t *ring = reinterpret_cast<const uint64_t *>(e->k_out) + int64_t(first_cycle) * cycle_words;
    for (int which = 0; which < 2; ++which) {
      double *dst = which == 0 ? q : qd;
      if (!dst) continue;
      fleet_place_ring_kernel<<<dim3(fleet_io_grid(n_rows * f->max_legs * f->max_dof, n_cycles), unsigned(n_cycles)), dim3(256), 0, e->stream>>>(
          reinterpret_cast<uint64_t *>(dst), ring, p.d_ids, n_rows, f->n, e->n_slots, cycle_words, e->L, e->NJ, which == 0 ? LEG_FIELD(e, Q) : LEG_FIELD(e, QD),
          f->max_legs, f->max_dof, nan_word());
      HIP_TRY(hipGetLastError());
    }
  }
  return SHC_OK;
}
