// shc_fleet_actions.hpp — shc_fleet_set_actions_device: the action pass (shc_actions.hpp) for a mixed fleet, straight from the caller's device
// array in the caller's instance order.  Included by shc_fleet.hpp, beside shc_fleet_observe.hpp; uses the readiness check, ids and ordering
// calls of shc_fleet_io.hpp.
//
// shc_fleet_set_inputs_device reaches the state through a pack kernel, the part's staging and one scatter kernel per array.  Here one launch of
// actions_kernel per part, on the part's own stream (or its two half streams while split steps are in flight, as the engines' setters), reads
// row ids[r] of the caller's array for robot r of the part - the part's caller ids (fleet_part_ids, the table device I/O keeps on the device) are
// the kernel's row table - converts the selected columns and stores them into the part's state.  Nothing is staged and nothing is allocated once
// device I/O is prepared.  Every host-side effect is the engine's (actions_apply), so it is what shc_fleet_set_inputs_device leaves.
#pragma once

extern "C" int shc_fleet_set_actions_device(shc_fleet *f, const shc_act_spec *spec, const void *actions) {
  if (!f || !spec || !actions) return fail(SHC_ERR_INVALID_ARG, "fleet, spec or actions NULL");
  ActLayout lay;
  if (const char *why = act_layout(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  if (spec->legs < f->max_legs || spec->dof < f->max_dof) return fail(SHC_ERR_INVALID_ARG, "shc_act_spec.legs / dof are below the fleet's shape (shc_fleet_shape)");
  if (reinterpret_cast<uintptr_t>(actions) & (act_element_bytes(spec) - 1)) return fail(SHC_ERR_INVALID_ARG, "actions must be aligned to its element size");
  int rc = fleet_io_ready(f);
  if (rc != SHC_OK) return rc;
  for (const auto &p : f->parts) // every part is asked before the first launch
    if ((rc = actions_check(p.engine, spec)) != SHC_OK) return rc;
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  const int64_t stride = spec->row_stride ? spec->row_stride : lay.width;
  for (auto &p : f->parts) {
    const bool ride = actions_ride(p.engine, lay, 1);
    if (!ride && (rc = shc_engine_join(p.engine)) != SHC_OK) return rc; // split steps in flight: the part's stream follows both halves first
    if ((rc = actions_apply(p.engine, spec, lay, actions, stride, p.d_ids, ride)) != SHC_OK) return rc;
  }
  return SHC_OK;
}
