// shc_fleet_checkpoint.hpp — fleet checkpoints: shc_fleet_checkpoint_*, shc_fleet_restore_instances, shc_fleet_scan_and_restore.  The fleet layer
// over the engines' device checkpoints (shc_checkpoint.hpp) and health scan (shc_health.hpp): one handle for a mixed fleet, maps in the CALLER's
// instance order, one call.  Included by shc_fleet.hpp.
//
// A fleet checkpoint is one shc_checkpoint per part, made and used through the engine entry points on the part's own stream; what is new here
// is the translation between the caller's order and a part's order.  A host map is validated and split into the parts' maps on the host and
// goes through the engine's host form (a fleet that spans devices has no device every part could read one map from); a device map is
// translated by fleet_translate_map_kernel on each part's stream, directly before the part's restore, and goes through the engine's device
// form - the only device path.  shc_fleet_scan_and_restore needs no translation: each part's scan writes the part's own map.
#pragma once

// the block a part keeps on its own device (FleetPart::ck_block), every piece at a multiple of 16 bytes
struct FleetCkBlock {
  size_t health, map, count, bytes; // [rows] shc_robot_health, [rows] int64 restore map, [1] int64 selected count (the caller's ids: FleetPart::d_ids)
};
static FleetCkBlock fleet_ck_block(size_t rows) {
  const size_t r16 = (rows * 8 + 15) & ~size_t(15);
  FleetCkBlock b;
  b.health = 0;
  b.map = rows * sizeof(shc_robot_health);
  b.count = b.map + r16;
  b.bytes = b.count + 16;
  return b;
}

// Device form: the part's map from the caller's.  One thread per destination slot j of part k, grid-stride; ids (the part's caller ids,
// ascending) makes the loads of `source` a gather over neighbouring or nearby lines.  A source outside [0, n), of another morphology or of
// another part of the same morphology becomes -1: the guard is on the value, before it indexes anything.
__global__ void fleet_translate_map_kernel(int64_t *__restrict__ local, const int64_t *__restrict__ source, const int64_t *__restrict__ ids,
                                           const int32_t *__restrict__ part_of, const int64_t *__restrict__ local_of, int64_t rows, int64_t n, int32_t k) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < rows; j += stride) {
    const int64_t s = source[ids[j]];
    int64_t out = -1;
    if (s >= 0 && s < n && part_of[s] == k) out = local_of[s];
    local[j] = out;
  }
}

// A fleet checkpoint sits in its fleet's registry (shc_fleet::checkpoints).  shc_fleet_destroy orphans the handles (fleet == nullptr) while its
// engines release the device arrays of the parts' checkpoints: an orphan answers every use with SHC_ERR_INVALID_ARG, and
// shc_fleet_checkpoint_destroy frees what is left of it - no call ever follows a pointer into a destroyed fleet.
struct shc_fleet_checkpoint {
  shc_fleet *fleet;
  shc_fleet_checkpoint *next;
  std::vector<shc_checkpoint *> parts; // parts[k] belongs to fleet->parts[k].engine
};

static void fleet_release_checkpoints(shc_fleet *f) {
  for (shc_fleet_checkpoint *ck = f->checkpoints; ck;) {
    shc_fleet_checkpoint *next = ck->next;
    ck->fleet = nullptr, ck->next = nullptr;
    ck = next;
  }
  f->checkpoints = nullptr;
}

// The first checkpoint call of a fleet: the inverse tables on the host, every part's block on its device and - when one device holds every
// part - the tables on that device.  Allocates and copies synchronously; later calls find everything in place.
static int fleet_ck_prepare(shc_fleet *f) {
  if (f->ck_ready) return SHC_OK;
  if (f->ck_part_of.empty()) {
    f->ck_part_of.assign(size_t(f->n), 0);
    f->ck_local_of.assign(size_t(f->n), 0);
    for (size_t k = 0; k < f->parts.size(); ++k)
      for (size_t j = 0; j < f->parts[k].ids.size(); ++j) {
        f->ck_part_of[size_t(f->parts[k].ids[j])] = int32_t(k);
        f->ck_local_of[size_t(f->parts[k].ids[j])] = int64_t(j);
      }
  }
  bool one_device = true;
  for (auto &p : f->parts) {
    one_device = one_device && p.device == f->parts[0].device;
    if (const int rc = fleet_part_ids(p); rc != SHC_OK) return rc;
    if (p.ck_block) continue;
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipMalloc(&p.ck_block, fleet_ck_block(p.ids.size()).bytes));
  }
  if (one_device && !f->ck_tables) {
    const size_t n = size_t(f->n);
    HIP_TRY(hipSetDevice(f->parts[0].device));
    HIP_TRY(hipMalloc(&f->ck_tables, n * 12));
    HIP_TRY(hipMemcpy(f->ck_tables, f->ck_local_of.data(), n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f->ck_tables + n * 8, f->ck_part_of.data(), n * 4, hipMemcpyHostToDevice));
  }
  f->ck_ready = true;
  return SHC_OK;
}

static int fleet_checkpoint_of(const shc_fleet *f, const shc_fleet_checkpoint *ck) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  if (!ck) return fail(SHC_ERR_INVALID_ARG, "checkpoint is NULL");
  if (!ck->fleet) return fail(SHC_ERR_INVALID_ARG, "the checkpoint's fleet has been destroyed");
  if (ck->fleet != f) return fail(SHC_ERR_INVALID_ARG, "the checkpoint belongs to another fleet");
  return SHC_OK;
}
// What every part would answer, asked of all of them before the first launch so that a refusal leaves every part as it was: the conditions
// shc_engine_checkpoint_update (restore = false) and shc_engine_restore_instances (restore = true) test at their entry, in their order.
static int fleet_parts_ready(const shc_fleet *f, const shc_fleet_checkpoint *ck, bool restore) {
  for (size_t k = 0; k < f->parts.size(); ++k) {
    const shc_engine *e = f->parts[k].engine;
    if (resident_active(e)) return fail(SHC_ERR_BUSY, "a part of the fleet is in resident mode: only shc_engine_resident_* calls are valid until shc_engine_resident_end");
    const int rc = checkpoint_of(e, ck->parts[k]);
    if (rc != SHC_OK) return rc;
    if (!restore) continue;
    if (adjust_pending(e)) return fail(SHC_ERR_UNSUPPORTED, "a shc_engine_adjust_parameter waits for its loop on a part: step once, then shc_fleet_checkpoint_update");
    if (ck->parts[k]->generation != adjust_generation(e))
      return fail(SHC_ERR_UNSUPPORTED, "the gait or a parameter of a part has changed since the checkpoint was captured: shc_fleet_checkpoint_update");
  }
  return SHC_OK;
}

extern "C" int shc_fleet_checkpoint_create(shc_fleet *f, shc_fleet_checkpoint **out) {
  if (!out) return fail(SHC_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  int rc = fleet_ck_prepare(f);
  if (rc != SHC_OK) return rc;
  shc_fleet_checkpoint *ck = new shc_fleet_checkpoint();
  for (auto &p : f->parts) {
    shc_checkpoint *part = nullptr;
    if ((rc = shc_engine_checkpoint_create(p.engine, &part)) != SHC_OK) break;
    ck->parts.push_back(part);
  }
  if (rc != SHC_OK) {
    for (shc_checkpoint *part : ck->parts) (void)shc_checkpoint_destroy(part);
    delete ck;
    return rc;
  }
  ck->fleet = f;
  ck->next = f->checkpoints;
  f->checkpoints = ck;
  *out = ck;
  return SHC_OK;
}
extern "C" int shc_fleet_checkpoint_update(shc_fleet *f, shc_fleet_checkpoint *ck) {
  int rc = fleet_checkpoint_of(f, ck);
  if (rc == SHC_OK) rc = fleet_parts_ready(f, ck, false);
  if (rc != SHC_OK) return rc;
  for (size_t k = 0; k < f->parts.size() && rc == SHC_OK; ++k) rc = shc_engine_checkpoint_update(f->parts[k].engine, ck->parts[k]);
  return rc;
}
extern "C" int shc_fleet_checkpoint_destroy(shc_fleet_checkpoint *ck) {
  if (!ck) return fail(SHC_ERR_INVALID_ARG, "checkpoint is NULL");
  if (shc_fleet *f = ck->fleet)
    for (shc_fleet_checkpoint **p = &f->checkpoints; *p; p = &(*p)->next)
      if (*p == ck) {
        *p = ck->next;
        break;
      }
  for (shc_checkpoint *part : ck->parts) (void)shc_checkpoint_destroy(part); // (waits for the part's stream while its engine lives)
  delete ck;
  return SHC_OK;
}
extern "C" int64_t shc_fleet_checkpoint_bytes(const shc_fleet_checkpoint *ck) {
  int64_t bytes = 0;
  if (ck)
    for (const shc_checkpoint *part : ck->parts) bytes += shc_checkpoint_bytes(part);
  return bytes;
}

extern "C" int shc_fleet_restore_instances(shc_fleet *f, const shc_fleet_checkpoint *ck, const int64_t *source, int on_device) {
  int rc = fleet_checkpoint_of(f, ck);
  if (rc == SHC_OK) rc = fleet_parts_ready(f, ck, true);
  if (rc != SHC_OK) return rc;
  const size_t np = f->parts.size();
  if (!source) { // the identity, in either form: every part restores everything
    for (size_t k = 0; k < np && rc == SHC_OK; ++k) rc = shc_engine_restore_instances(f->parts[k].engine, ck->parts[k], nullptr, 0);
    return rc;
  }
  if (on_device) {
    if (!f->ck_tables) return fail(SHC_ERR_UNSUPPORTED, "a device map needs one device that holds every part of the fleet: use the host form");
    const int64_t *local_of = reinterpret_cast<const int64_t *>(f->ck_tables);
    const int32_t *part_of = reinterpret_cast<const int32_t *>(f->ck_tables + size_t(f->n) * 8);
    HIP_TRY(hipSetDevice(f->parts[0].device));
    for (size_t k = 0; k < np; ++k) {
      FleetPart &p = f->parts[k];
      const int64_t rows = int64_t(p.ids.size());
      const FleetCkBlock b = fleet_ck_block(size_t(rows));
      int64_t *map = reinterpret_cast<int64_t *>(p.ck_block + b.map);
      const unsigned grid = unsigned(std::min<int64_t>((rows + 255) / 256, 2048));
      fleet_translate_map_kernel<<<dim3(grid), dim3(256), 0, p.engine->stream>>>(map, source, p.d_ids, part_of, local_of, rows,
                                                                                 f->n, int32_t(k));
      HIP_TRY(hipGetLastError());
      if ((rc = shc_engine_restore_instances(p.engine, ck->parts[k], map, 1)) != SHC_OK) return rc;
    }
    return SHC_OK;
  }
  // host form: the whole map is validated before anything is launched
  bool crosses_parts = false;
  for (int64_t i = 0; i < f->n; ++i) {
    const int64_t s = source[i];
    if (s < 0) continue;
    if (s >= f->n) return fail(SHC_ERR_INVALID_ARG, "source entry >= n");
    const int ks = f->ck_part_of[size_t(s)], ki = f->ck_part_of[size_t(i)];
    if (f->parts[ks].morph != f->parts[ki].morph) return fail(SHC_ERR_INVALID_ARG, "source entry of another morphology than its destination");
    crosses_parts = crosses_parts || ks != ki;
  }
  if (crosses_parts)
    return fail(SHC_ERR_UNSUPPORTED, "source entry in another part (another device's shard of the morphology): a clone across parts is not implemented");
  std::vector<int64_t> local;
  for (size_t k = 0; k < np; ++k) {
    const FleetPart &p = f->parts[k];
    local.resize(p.ids.size());
    bool any = false;
    for (size_t j = 0; j < p.ids.size(); ++j) {
      const int64_t s = source[p.ids[j]];
      local[j] = s < 0 ? int64_t(-1) : f->ck_local_of[size_t(s)];
      any = any || s >= 0;
    }
    if (!any) continue; // a part the map does not name is not touched, nor is its stream waited for
    if ((rc = shc_engine_restore_instances(p.engine, ck->parts[k], local.data(), 0)) != SHC_OK) return rc;
  }
  return SHC_OK;
}

extern "C" int shc_fleet_scan_and_restore(shc_fleet *f, const shc_fleet_checkpoint *ck, const shc_health_criteria *criteria, shc_robot_health *health,
                                          int64_t *n_restored) {
  int rc = fleet_checkpoint_of(f, ck);
  if (rc == SHC_OK) rc = fleet_parts_ready(f, ck, true);
  if (rc != SHC_OK) return rc;
  const shc_health_criteria crit = health_criteria(criteria); // (what shc_engine_scan_health would refuse, before the first part has run)
  if (crit.reserved != 0) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.reserved must be 0");
  if (crit.select & ~kHealthAllFlags) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.select has bits outside SHC_HEALTH_*");
  for (size_t k = 0; k < f->parts.size(); ++k) {
    FleetPart &p = f->parts[k];
    const int64_t rows = int64_t(p.ids.size());
    const FleetCkBlock b = fleet_ck_block(size_t(rows));
    int64_t *map = reinterpret_cast<int64_t *>(p.ck_block + b.map);
    rc = shc_engine_scan_health(p.engine, 0, rows, criteria, health ? reinterpret_cast<shc_robot_health *>(p.ck_block + b.health) : nullptr, map, nullptr,
                                n_restored ? reinterpret_cast<int64_t *>(p.ck_block + b.count) : nullptr, 1);
    // select = 0 (or no criteria) selects nobody: a scan and nothing else
    if (rc == SHC_OK && crit.select != 0) rc = shc_engine_restore_instances(p.engine, ck->parts[k], map, 1);
    if (rc != SHC_OK) return rc;
  }
  if (!health && !n_restored) return SHC_OK;
  // the records and the counts come back on each part's stream, behind its scan; one wait per part
  shc_robot_health *rows = reinterpret_cast<shc_robot_health *>(f->scratch.room(health ? size_t(f->n) * sizeof(shc_robot_health) : 0)); // part by part, dense
  std::vector<int64_t> counts(f->parts.size(), 0);
  size_t at = 0;
  for (size_t k = 0; k < f->parts.size(); ++k) {
    FleetPart &p = f->parts[k];
    const FleetCkBlock b = fleet_ck_block(p.ids.size());
    HIP_TRY(hipSetDevice(p.device));
    if (health) HIP_TRY(hipMemcpyAsync(rows + at, p.ck_block + b.health, p.ids.size() * sizeof(shc_robot_health), hipMemcpyDeviceToHost, p.engine->stream));
    if (n_restored) HIP_TRY(hipMemcpyAsync(&counts[k], p.ck_block + b.count, 8, hipMemcpyDeviceToHost, p.engine->stream));
    at += p.ids.size();
  }
  at = 0;
  int64_t total = 0;
  for (size_t k = 0; k < f->parts.size(); ++k) {
    FleetPart &p = f->parts[k];
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipStreamSynchronize(p.engine->stream));
    if (health) // (a record is four 8-byte words: shc_health.hpp)
      fleet_place_host(reinterpret_cast<uint64_t *>(health), reinterpret_cast<const uint64_t *>(rows + at), p.ids.data(), int64_t(p.ids.size()), 1, 4, 1, 4, uint64_t(0));
    at += p.ids.size();
    total += counts[k];
  }
  if (n_restored) *n_restored = total;
  return SHC_OK;
}
