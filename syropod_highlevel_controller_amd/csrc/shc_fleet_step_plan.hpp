// shc_fleet_step_plan.hpp — shc_fleet_get_step_plan_device: the step plan pass (shc_step_plan.hpp) for a mixed fleet, straight into the caller's
// device array in the caller's instance order.  Included by shc_fleet.hpp, beside shc_fleet_observe.hpp, whose pattern it follows: the readiness
// check, ids and ordering calls are those of shc_fleet_io.hpp.
//
// One launch of step_plan_kernel per part (one per run of fields where a row is too wide for the tile, see step_plan_launch), on the part's own
// stream, reads the part's state and writes the selected columns of robot r of the part into row ids[r] of the caller's array.  Nothing is staged
// and nothing is allocated once device I/O is prepared; the rows of the parts are disjoint, so the parts' streams need no order among
// themselves.  No part's state is written.
#pragma once

extern "C" int shc_fleet_get_step_plan_device(shc_fleet *f, const shc_plan_spec *spec, void *out) {
  RowLayout lay;
  int rc = fleet_rows_begin<PlanRows>(f, spec, out, "out", lay, [&](const shc_engine *e) { return step_plan_check(e, spec); });
  if (rc != SHC_OK) return rc;
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const int rc = fleet_part_join(p);
    return rc != SHC_OK ? rc : step_plan_launch(p.engine, spec, lay, out, stride, p.d_ids, 0, int64_t(p.ids.size()));
  });
}
