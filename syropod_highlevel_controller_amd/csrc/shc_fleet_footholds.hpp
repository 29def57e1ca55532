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

// What both calls ask before anything changes: the spec, the fleet's shape, the array, one device, every part
static int fleet_footholds_check(const shc_fleet *f, const shc_foothold_spec *spec, const void *rows, FhLayout &lay) {
  if (!f || !spec || !rows) return fail(SHC_ERR_INVALID_ARG, "fleet, spec or rows NULL");
  if (const char *why = fh_layout(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  if (spec->legs < f->max_legs) return fail(SHC_ERR_INVALID_ARG, "shc_foothold_spec.legs is below the fleet's shape (shc_fleet_shape)");
  if (reinterpret_cast<uintptr_t>(rows) & (fh_element_bytes(spec) - 1)) return fail(SHC_ERR_INVALID_ARG, "rows must be aligned to its element size");
  int rc = fleet_io_ready(f);
  if (rc != SHC_OK) return rc;
  for (const auto &p : f->parts) // every part is asked before the first launch
    if ((rc = footholds_check(p.engine, spec)) != SHC_OK) return rc;
  return SHC_OK;
}

extern "C" int shc_fleet_set_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, const void *rows, int64_t *ignored_device) {
  FhLayout lay;
  int rc = fleet_footholds_check(f, spec, rows, lay);
  if (rc != SHC_OK) return rc;
  if (const char *why = fh_set_fields(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  if (reinterpret_cast<uintptr_t>(ignored_device) & 7) return fail(SHC_ERR_INVALID_ARG, "ignored must be aligned to 8 bytes");
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  const int64_t stride = spec->row_stride ? spec->row_stride : lay.width;
  for (auto &p : f->parts) {
    HIP_TRY(hipSetDevice(p.device));
    if ((rc = shc_engine_join(p.engine)) != SHC_OK) return rc; // split steps in flight: the part's stream follows both halves first
    if ((rc = footholds_apply(p.engine, spec, lay, rows, stride, p.d_ids, ignored_device)) != SHC_OK) return rc;
  }
  return SHC_OK;
}

extern "C" int shc_fleet_get_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, void *rows) {
  FhLayout lay;
  int rc = fleet_footholds_check(f, spec, rows, lay);
  if (rc != SHC_OK) return rc;
  if (spec->mode != SHC_FH_REQUEST) return fail(SHC_ERR_INVALID_ARG, "shc_foothold_spec.mode must be 0 for shc_fleet_get_footholds_device");
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  const int64_t stride = spec->row_stride ? spec->row_stride : lay.width;
  for (auto &p : f->parts) {
    HIP_TRY(hipSetDevice(p.device));
    if ((rc = shc_engine_join(p.engine)) != SHC_OK) return rc;
    if ((rc = footholds_read(p.engine, spec, lay, rows, stride, p.d_ids)) != SHC_OK) return rc;
  }
  return SHC_OK;
}
