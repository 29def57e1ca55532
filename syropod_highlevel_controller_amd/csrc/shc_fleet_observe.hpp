// shc_fleet_observe.hpp — shc_fleet_get_observations_device: the observation pass (shc_observe.hpp) for a mixed fleet, straight into the caller's
// device array in the caller's instance order.  Included by shc_fleet.hpp, beside shc_fleet_io.hpp, whose readiness check, ids and ordering calls it
// uses.
//
// shc_fleet_get_outputs_device reaches the caller's buffers through the engines' getters, a staging buffer and a place kernel, per part and per
// output, and moves whole records.  Here one launch of observe_kernel per part, on the part's own stream, reads the part's state and writes the
// selected columns of robot r of the part into row ids[r] of the caller's array: the part's caller ids (fleet_part_ids - the table device I/O keeps
// on the device) are the kernel's row table.  Nothing is staged and nothing is allocated once device I/O is prepared; the rows of the parts are
// disjoint, so the parts' streams need no order among themselves.
#pragma once

extern "C" int shc_fleet_get_observations_device(shc_fleet *f, const shc_obs_spec *spec, void *out) {
  RowLayout lay;
  int rc = fleet_rows_begin<ObsRows>(f, spec, out, "out", lay, [&](const shc_engine *e) { return observe_check(e, spec, lay); });
  if (rc != SHC_OK) return rc;
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const int rc = fleet_part_join(p);
    return rc != SHC_OK ? rc : observe_launch(p.engine, spec, lay, out, stride, p.d_ids, 0, int64_t(p.ids.size()));
  });
}
