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
  RowLayout lay;
  int rc = fleet_rows_begin<ActRows>(f, spec, actions, "actions", lay, [&](const shc_engine *e) { return actions_check(e, spec); });
  if (rc != SHC_OK) return rc;
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const bool ride = actions_ride(p.engine, lay, 1);
    const int rc = ride ? SHC_OK : shc_engine_join(p.engine); // split steps in flight: the part's stream follows both halves first
    return rc != SHC_OK ? rc : actions_apply(p.engine, spec, lay, actions, stride, p.d_ids, ride);
  });
}
