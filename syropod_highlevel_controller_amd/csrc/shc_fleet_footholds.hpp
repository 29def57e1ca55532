// shc_fleet_footholds.hpp — shc_fleet_set_footholds_device / shc_fleet_get_footholds_device: the foothold pass (shc_footholds.hpp) for a mixed
// fleet, straight from / into the caller's device array in the caller's instance order.  Included by shc_fleet.hpp, beside
// shc_fleet_actions.hpp; uses the readiness check, ids and ordering calls of shc_fleet_io.hpp.
//
// The host calls have no fleet form: a caller walks shc_fleet_part / shc_fleet_part_instances and regroups its rows.  Here one launch of
// footholds_set_kernel / footholds_get_kernel per part, on the part's own stream, serves robot r of the part from row ids[r] of the caller's
// array - the part's caller ids (fleet_part_ids, the table device I/O keeps on the device) are the kernel's row table; every part adds its
// dropped rows to the caller's one device word.  A part's first call allocates its records (and the sequence state for targets), as the
// engine's host calls do; after that nothing is staged and nothing is allocated.
#pragma once

extern "C" int shc_fleet_set_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, const void *rows, int64_t *ignored_device) {
  RowLayout lay;
  int rc = fleet_rows_begin<FhRows>(f, spec, rows, "rows", lay, [&](const shc_engine *e) { return footholds_check(e, spec); });
  if (rc != SHC_OK) return rc;
  if (const char *why = fh_set_fields(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  if (reinterpret_cast<uintptr_t>(ignored_device) & 7) return fail(SHC_ERR_INVALID_ARG, "ignored must be aligned to 8 bytes");
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const int rc = fleet_part_join(p);
    return rc != SHC_OK ? rc : footholds_apply(p.engine, spec, lay, rows, stride, p.d_ids, ignored_device);
  });
}

extern "C" int shc_fleet_get_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, void *rows) {
  RowLayout lay;
  int rc = fleet_rows_begin<FhRows>(f, spec, rows, "rows", lay, [&](const shc_engine *e) { return footholds_check(e, spec); });
  if (rc != SHC_OK) return rc;
  if (spec->mode != SHC_FH_REQUEST) return fail(SHC_ERR_INVALID_ARG, "shc_foothold_spec.mode must be 0 for shc_fleet_get_footholds_device");
  return fleet_rows_each(f, spec, lay, [&](FleetPart &p, int64_t stride) {
    const int rc = fleet_part_join(p);
    return rc != SHC_OK ? rc : footholds_read(p.engine, spec, lay, rows, stride, p.d_ids);
  });
}
