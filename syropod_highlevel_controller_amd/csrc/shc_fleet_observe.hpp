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
  if (!f || !spec || !out) return fail(SHC_ERR_INVALID_ARG, "fleet, spec or out NULL");
  ObsLayout lay;
  if (const char *why = obs_layout(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  if (spec->legs < f->max_legs || spec->dof < f->max_dof) return fail(SHC_ERR_INVALID_ARG, "shc_obs_spec.legs / dof are below the fleet's shape (shc_fleet_shape)");
  if (reinterpret_cast<uintptr_t>(out) & (obs_element_bytes(spec) - 1)) return fail(SHC_ERR_INVALID_ARG, "out must be aligned to its element size");
  int rc = fleet_io_ready(f);
  if (rc != SHC_OK) return rc;
  for (const auto &p : f->parts) // every part is asked before the first launch
    if ((rc = observe_check(p.engine, spec, lay)) != SHC_OK) return rc;
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  const int64_t stride = spec->row_stride ? spec->row_stride : lay.width;
  for (auto &p : f->parts) {
    HIP_TRY(hipSetDevice(p.device));
    if ((rc = shc_engine_join(p.engine)) != SHC_OK) return rc; // split steps in flight: the part's stream follows both halves first
    if ((rc = observe_launch(p.engine, spec, lay, out, stride, p.d_ids, 0, int64_t(p.ids.size()))) != SHC_OK) return rc;
  }
  return SHC_OK;
}
