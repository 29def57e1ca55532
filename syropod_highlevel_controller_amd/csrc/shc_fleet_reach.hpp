// shc_fleet_reach.hpp — shc_fleet_probe_reach_device: the reach probe (shc_reach.hpp) for a mixed fleet, straight from and into the caller's
// device arrays in the caller's instance order.  Included by shc_fleet.hpp, beside shc_fleet_footholds.hpp; uses the readiness check, ids and
// ordering calls of shc_fleet_io.hpp.
//
// One launch of reach_probe_kernel per part, on the part's own stream, reads the targets of robot r of the part from row ids[r] of the caller's
// array and writes its blocks into row ids[r] of the caller's output - the part's caller ids (fleet_part_ids, the table device I/O keeps on the
// device) are the kernel's row table.  Nothing is staged and nothing is allocated once device I/O is prepared; the rows of the parts are
// disjoint, so the parts' streams need no order among themselves.  No part's state is written.
#pragma once

extern "C" int shc_fleet_probe_reach_device(shc_fleet *f, const shc_reach_spec *spec, const void *targets, void *out) {
  if (!f || !spec || !targets || !out) return fail(SHC_ERR_INVALID_ARG, "fleet, spec, targets or out NULL");
  RowLayout lay;
  if (const int bad = reach_resolve(spec, lay)) return bad;
  if (spec->legs < f->max_legs || spec->dof < f->max_dof) return fail(SHC_ERR_INVALID_ARG, "shc_reach_spec.legs / dof are below the fleet's shape (shc_fleet_shape)");
  int rc = reach_arrays_check(spec, targets, out);
  if (rc == SHC_OK) rc = fleet_io_ready(f);
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i) rc = reach_check(f->parts[i].engine, spec);
  if (rc == SHC_OK) rc = fleet_io_prepare(f);
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i) {
    FleetPart &p = f->parts[i];
    if ((rc = fleet_part_join(p)) == SHC_OK) rc = reach_launch(p.engine, spec, lay, targets, out, p.d_ids, 0, int64_t(p.ids.size()));
  }
  return rc;
}
