// shc_fleet.hpp — shc_fleet_*: mixed-morphology batches and multi-device sharding behind one handle (C ABI, host side).
//
// BASELINE.json configs[3] / configs[4]: robots are independent (nothing in the reference couples two robots), so a batch
// shards by contiguous instance ranges with no data-path exchange while stepping, and a mixed-morphology batch is binned by
// morphology: the cycle kernel keeps ONE morphology's DH / limit tables in LDS and maps one leg to one lane, so every
// (morphology bin, device) pair gets its own engine on its own HIP stream.  The fleet keeps the caller's instance order at
// the boundary whatever the interleaving pattern.  The only exchange is the all-gather of the final joint-state buffer:
// every device ends up with every instance's joints, copied device to device (hipMemcpyPeerAsync: xGMI on an MI355X node).
// One-process-per-GPU hosts (bench.py under torch.distributed) do the same exchange with RCCL instead.
// What crosses that boundary is translated in one place: shc_fleet_order.hpp states pick (the caller's padded rows -> a part's dense rows) and
// place (back, padding written) on the host, shc_fleet_io.hpp holds the same two as kernels and the one walk over the inputs and the one over
// the outputs that every setter and getter, host or device form, runs through.  This file creates the fleet, steps it and exchanges the joints.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "shc_fleet_order.hpp" // pick and place between the caller's rows and a part's, on the host

struct FleetPart {
  shc_engine *engine = nullptr;
  int morph = 0, device = 0, device_slot = 0;
  hipStream_t stream = nullptr;
  std::vector<int64_t> ids; // caller's instance ids, ascending
  int64_t *d_ids = nullptr;           // ... and on the part's device (fleet_part_ids): the one copy the exchange step, the checkpoints and the device I/O read
  // the exchange step's buffers, allocated by the first shc_fleet_all_gather_joints and kept
  double *g_joints = nullptr;         // this part's joints [rows][L][D] on its own device
  hipEvent_t g_ready = nullptr;       // recorded on `stream` once g_joints is complete
  std::vector<double *> r_joints;     // per device slot (other devices only): the landing buffer of the peer copy ...
  std::vector<int64_t *> r_ids;       // ... and the ids over there
  // fleet checkpoints (shc_fleet_checkpoint.hpp): one block on the part's device, allocated by the first shc_fleet_checkpoint_create and kept
  char *ck_block = nullptr;           // [health records][restore map][selected count], FleetCkBlock gives the offsets
  // device I/O (shc_fleet_io.hpp): staging and the two ordering events, made by the first device I/O call and kept
  char *io_stage = nullptr;
  size_t io_stage_bytes = 0;
  hipEvent_t io_after = nullptr, io_before = nullptr; // the part's stream after the caller's / the caller's stream after the part's
  // shc_fleet_step_k (shc_fleet_step_k.hpp): the part's rows of the K-deep input arrays, dense [K][rows][..] group by group; grows on demand, kept
  char *k_stage = nullptr;
  size_t k_stage_bytes = 0;
};

struct shc_fleet {
  std::vector<shc_params> params;
  std::vector<FleetPart> parts;
  std::vector<int> devices;
  int64_t n = 0;
  int max_legs = 0, max_dof = 0;
  std::vector<double *> gather; // per device: [n][max_legs][max_dof], NaN padded
  std::vector<hipStream_t> gather_stream; // per device: incoming peer copies + their placement
  FleetScratch scratch; // the host route's dense rows of one part (shc_fleet_order.hpp)
  // fleet checkpoints (shc_fleet_checkpoint.hpp)
  struct shc_fleet_checkpoint *checkpoints = nullptr; // the registry of this fleet's checkpoint handles: orphaned with the fleet
  std::vector<int32_t> ck_part_of;   // caller's id -> its part ...
  std::vector<int64_t> ck_local_of;  // ... and its instance id inside that part
  char *ck_tables = nullptr;         // the two tables on the device, when one device holds every part: local_of [n] int64, then part_of [n] int32
  bool ck_ready = false;
  // device I/O (shc_fleet_io.hpp)
  int64_t io_chunk = 0; // robots per part and staging pass of the record outputs; 0 = the default
  bool io_ready = false;
  int k_cycles = 0;     // K of the latest shc_fleet_step_k (0: none yet): what shc_fleet_get_step_k_joints_device may be asked for
};
static void fleet_release_checkpoints(shc_fleet *f); // orphan the fleet's checkpoint handles (shc_fleet_destroy)

static void fleet_free(shc_fleet *f) {
  if (!f) return;
  fleet_release_checkpoints(f); // (the parts' engines release the device arrays of their own checkpoints below)
  const int ck_device = f->parts.empty() ? 0 : f->parts[0].device;
  for (auto &p : f->parts) {
    if (p.engine) shc_engine_destroy(p.engine);
    if (p.stream) {
      (void)hipSetDevice(p.device);
      (void)hipStreamDestroy(p.stream);
    }
  }
  for (auto &p : f->parts) {
    (void)hipSetDevice(p.device);
    (void)hipFree(p.g_joints);
    (void)hipFree(p.d_ids);
    (void)hipFree(p.ck_block);
    (void)hipFree(p.io_stage);
    (void)hipFree(p.k_stage);
    if (p.io_after) (void)hipEventDestroy(p.io_after);
    if (p.io_before) (void)hipEventDestroy(p.io_before);
    if (p.g_ready) (void)hipEventDestroy(p.g_ready);
    for (size_t d = 0; d < p.r_joints.size(); ++d) {
      (void)hipSetDevice(f->devices[d]);
      (void)hipFree(p.r_joints[d]);
      (void)hipFree(p.r_ids[d]);
    }
  }
  if (f->ck_tables) { // (every part's stream has drained: shc_engine_destroy waits for it)
    (void)hipSetDevice(ck_device);
    (void)hipFree(f->ck_tables);
  }
  for (size_t d = 0; d < f->gather.size(); ++d) {
    (void)hipSetDevice(f->devices[d]);
    if (f->gather[d]) (void)hipFree(f->gather[d]);
    if (d < f->gather_stream.size() && f->gather_stream[d]) (void)hipStreamDestroy(f->gather_stream[d]);
  }
  delete f;
}

static int f_parts_on_device(const shc_fleet *f, int device) {
  int k = 0;
  for (const auto &p : f->parts) k += p.device == device ? 1 : 0;
  return k;
}
extern "C" int shc_fleet_create(const shc_params *params, int n_morphologies, const int32_t *morph_id, int64_t n_instances, const int *device_ids,
                                int n_devices, shc_fleet **out) {
  if (!params || !out || n_morphologies < 1 || n_instances < 1) return fail(SHC_ERR_INVALID_ARG, "params / out NULL, or no morphology / instance");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(SHC_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
  const int one = 0;
  if (!device_ids || n_devices < 1) {
    device_ids = &one;
    n_devices = 1;
  }
  for (int d = 0; d < n_devices; ++d)
    if (device_ids[d] < 0 || device_ids[d] >= ndev) return fail(SHC_ERR_INVALID_ARG, "device id out of range");
  shc_fleet *f = new shc_fleet();
  f->params.assign(params, params + n_morphologies);
  f->devices.assign(device_ids, device_ids + n_devices);
  f->n = n_instances;
  std::vector<std::vector<int64_t>> bins(n_morphologies);
  for (int64_t i = 0; i < n_instances; ++i) {
    const int m = morph_id ? morph_id[i] : 0;
    if (m < 0 || m >= n_morphologies) {
      fleet_free(f);
      return fail(SHC_ERR_INVALID_ARG, "morph_id out of range");
    }
    bins[m].push_back(i);
  }
  for (int m = 0; m < n_morphologies; ++m) {
    if (bins[m].empty()) continue;
    int L, NJ;
    const int rc = validate_params(&params[m], &L, &NJ);
    if (rc != SHC_OK) {
      fleet_free(f);
      return rc;
    }
    f->max_legs = std::max(f->max_legs, L);
    f->max_dof = std::max(f->max_dof, NJ);
  }
  // one init chain per morphology, shared by its shards
  for (int m = 0; m < n_morphologies; ++m) {
    if (bins[m].empty()) continue;
    shc_tables tables;
    int rc = shc_generate_tables(&params[m], &tables);
    const int64_t nb = int64_t(bins[m].size());
    for (int d = 0; d < n_devices && rc == SHC_OK; ++d) { // contiguous shards of the bin, sizes differing by at most one
      const int64_t base = nb / n_devices, rem = nb % n_devices;
      const int64_t lo = d * base + std::min<int64_t>(d, rem), hi = lo + base + (d < rem ? 1 : 0);
      if (hi == lo) continue;
      FleetPart part;
      part.morph = m;
      part.device = device_ids[d];
      part.device_slot = d;
      part.ids.assign(bins[m].begin() + lo, bins[m].begin() + hi);
      if (hipSetDevice(part.device) != hipSuccess || hipStreamCreateWithFlags(&part.stream, hipStreamNonBlocking) != hipSuccess) {
        rc = fail(SHC_ERR_HIP, "stream creation failed");
        break;
      }
      rc = shc_engine_create_with_tables(&params[m], &tables, hi - lo, part.device, part.stream, &part.engine);
      f->parts.push_back(part); // (also on failure: fleet_free releases the stream)
    }
    if (rc != SHC_OK) {
      fleet_free(f);
      return rc;
    }
  }
  // parts that share a device already run concurrently, one stream each: no two-stream split inside such a part (shc_engine_step)
  for (auto &part : f->parts)
    if (f_parts_on_device(f, part.device) > 1) {
      const int rc = shc_engine_set_features(part.engine, part.engine->features | SHC_FEAT_SINGLE_STREAM);
      if (rc != SHC_OK) {
        fleet_free(f);
        return rc;
      }
    }
  f->gather.assign(n_devices, nullptr);
  *out = f;
  return SHC_OK;
}

extern "C" int shc_fleet_destroy(shc_fleet *f) {
  fleet_free(f);
  return SHC_OK;
}
extern "C" int64_t shc_fleet_instances(const shc_fleet *f) { return f ? f->n : 0; }
extern "C" int shc_fleet_part_count(const shc_fleet *f) { return f ? int(f->parts.size()) : 0; }
extern "C" int shc_fleet_part(const shc_fleet *f, int k, shc_engine **engine, int *morphology, int *device, int64_t *n_instances) {
  if (!f || k < 0 || k >= int(f->parts.size())) return fail(SHC_ERR_INVALID_ARG, "part index out of range");
  const FleetPart &p = f->parts[k];
  if (engine) *engine = p.engine;
  if (morphology) *morphology = p.morph;
  if (device) *device = p.device;
  if (n_instances) *n_instances = int64_t(p.ids.size());
  return SHC_OK;
}
extern "C" int shc_fleet_part_instances(const shc_fleet *f, int k, int64_t *ids) {
  if (!f || !ids || k < 0 || k >= int(f->parts.size())) return fail(SHC_ERR_INVALID_ARG, "part index out of range / ids NULL");
  std::copy(f->parts[k].ids.begin(), f->parts[k].ids.end(), ids);
  return SHC_OK;
}

// The part's caller ids on its own device, uploaded (synchronously) by the first user and kept.
static int fleet_part_ids(FleetPart &p) {
  if (p.d_ids) return SHC_OK;
  HIP_TRY(hipSetDevice(p.device));
  HIP_TRY(hipMalloc(&p.d_ids, p.ids.size() * 8));
  HIP_TRY(hipMemcpy(p.d_ids, p.ids.data(), p.ids.size() * 8, hipMemcpyHostToDevice));
  return SHC_OK;
}

extern "C" int shc_fleet_shape(const shc_fleet *f, int *max_legs, int *max_dof) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  if (max_legs) *max_legs = f->max_legs;
  if (max_dof) *max_dof = f->max_dof;
  return SHC_OK;
}

// every part advances on its own stream; nothing orders one part against another
extern "C" int shc_fleet_step(shc_fleet *f, int n_cycles) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  for (auto &p : f->parts) {
    const int rc = shc_engine_step(p.engine, n_cycles);
    if (rc != SHC_OK) return rc;
  }
  return SHC_OK;
}
extern "C" int shc_fleet_synchronize(shc_fleet *f) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  for (auto &p : f->parts) {
    const int rc = shc_engine_synchronize(p.engine);
    if (rc != SHC_OK) return rc;
  }
  return SHC_OK;
}

#include "shc_fleet_io.hpp" // the setters and getters, host and device forms: one walk over the inputs, one over the outputs, two routes

// The exchange step: every device ends up with the desired joint positions of ALL instances ([n][max_legs][max_dof], NaN
// padded, caller's order) in its own HBM; device_buffers[d] receives device d's buffer (owned by the fleet).  Each part
// gathers its joints on its own device and stream, places them in the local buffer, and every other device pulls the part's
// rows with one peer copy on its own gather stream (ordered behind the part by an event) and places them on its side - the
// place of the device I/O (fleet_place), which writes the NaN padding of its rows with every exchange.
// Direct peer copies rather than a ring collective: xGMI is point to point (7 links per GPU), so the (device, device) pairs use
// their own links concurrently - 1/8 of the data per link instead of the 7/8 a ring all-gather pushes through each - and a
// single-process host needs no communicator; the one-process-per-GPU host (bench.py, parallel.py) exchanges the same buffer
// with RCCL's all-gather.  Every buffer is allocated once (first call) and kept; nothing synchronises device-wide.
extern "C" int shc_fleet_all_gather_joints(shc_fleet *f, double **device_buffers) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  const size_t row = size_t(f->max_legs) * f->max_dof, total = size_t(f->n) * row;
  const int nd = int(f->devices.size());
  if (f->gather_stream.size() != size_t(nd)) f->gather_stream.assign(nd, nullptr);
  for (int d = 0; d < nd; ++d) {
    HIP_TRY(hipSetDevice(f->devices[d]));
    if (!f->gather_stream[d]) HIP_TRY(hipStreamCreateWithFlags(&f->gather_stream[d], hipStreamNonBlocking));
    if (!f->gather[d]) HIP_TRY(hipMalloc(&f->gather[d], total * 8)); // (every word is written by every exchange: the parts' ids partition [0, n), and place writes the padding)
  }
  for (auto &p : f->parts) { // first call: the part's own buffers, the landing buffers on the other devices, the ids everywhere
    if (p.g_joints) continue;
    const shc_params &pp = f->params[p.morph];
    const size_t rows = p.ids.size(), elems = rows * pp.leg_count * max_dof(pp);
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipMalloc(&p.g_joints, elems * 8));
    HIP_TRY(hipEventCreateWithFlags(&p.g_ready, hipEventDisableTiming));
    if (const int rc = fleet_part_ids(p); rc != SHC_OK) return rc;
    p.r_joints.assign(nd, nullptr);
    p.r_ids.assign(nd, nullptr);
    for (int d = 0; d < nd; ++d) {
      if (f->devices[d] == p.device) continue;
      HIP_TRY(hipSetDevice(f->devices[d]));
      HIP_TRY(hipMalloc(&p.r_joints[d], elems * 8));
      HIP_TRY(hipMalloc(&p.r_ids[d], rows * 8));
      HIP_TRY(hipMemcpy(p.r_ids[d], p.ids.data(), rows * 8, hipMemcpyHostToDevice));
    }
  }
  for (auto &p : f->parts) { // every part: joints -> its buffer -> the local gather buffer(s), on its own stream
    const shc_params &pp = f->params[p.morph];
    const int L = pp.leg_count, D = max_dof(pp);
    const int64_t rows = int64_t(p.ids.size());
    HIP_TRY(hipSetDevice(p.device));
    int rc = shc_engine_get_joint_state(p.engine, p.g_joints, nullptr, 1);
    if (rc != SHC_OK) return rc;
    HIP_TRY(hipEventRecord(p.g_ready, p.stream));
    for (int d = 0; d < nd; ++d) // (also covers several device slots naming one device)
      if (f->devices[d] == p.device && (rc = fleet_place(p.stream, f->gather[d], p.g_joints, p.d_ids, rows, L, D, f->max_legs, f->max_dof, nan_word())) != SHC_OK) return rc;
  }
  for (auto &p : f->parts) { // every other device pulls the part's rows and places them
    const shc_params &pp = f->params[p.morph];
    const int L = pp.leg_count, D = max_dof(pp);
    const int64_t rows = int64_t(p.ids.size()), threads = rows * L * D;
    for (int d = 0; d < nd; ++d) {
      if (f->devices[d] == p.device) continue;
      HIP_TRY(hipSetDevice(f->devices[d]));
      HIP_TRY(hipStreamWaitEvent(f->gather_stream[d], p.g_ready, 0));
      HIP_TRY(hipMemcpyPeerAsync(p.r_joints[d], f->devices[d], p.g_joints, p.device, size_t(threads) * 8, f->gather_stream[d]));
      if (const int rc = fleet_place(f->gather_stream[d], f->gather[d], p.r_joints[d], p.r_ids[d], rows, L, D, f->max_legs, f->max_dof, nan_word())) return rc;
    }
  }
  for (auto &p : f->parts) {
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipStreamSynchronize(p.stream));
  }
  for (int d = 0; d < nd; ++d) {
    HIP_TRY(hipSetDevice(f->devices[d]));
    HIP_TRY(hipStreamSynchronize(f->gather_stream[d]));
  }
  if (device_buffers)
    for (int d = 0; d < nd; ++d) device_buffers[d] = f->gather[d];
  return SHC_OK;
}

#include "shc_fleet_checkpoint.hpp" // shc_fleet_checkpoint_*, shc_fleet_restore_instances, shc_fleet_scan_and_restore
#include "shc_fleet_step_k.hpp" // shc_fleet_step_k, shc_fleet_get_step_k_joints_device: K cycles per launch from K-deep device arrays
#include "shc_fleet_observe.hpp" // shc_fleet_get_observations_device: chosen fields of every robot straight into the caller's rows
#include "shc_fleet_actions.hpp" // shc_fleet_set_actions_device: chosen input groups of every robot straight from the caller's rows
#include "shc_fleet_rollout.hpp" // shc_fleet_step_k_actions_device / _get_step_k_observations_device: K cycles per launch from / into the caller's dense tensors
#include "shc_fleet_footholds.hpp" // shc_fleet_set_footholds_device / _get_footholds_device: every robot's tip-target requests from / into the caller's rows
#include "shc_fleet_reach.hpp" // shc_fleet_probe_reach_device: the reach probe from / into the caller's rows
#include "shc_fleet_step_plan.hpp" // shc_fleet_get_step_plan_device: the step plan pass into the caller's rows

// ================================================================================================ one process per GPU: the exchange over peer copies
// The all-gather of the final joint buffer (BASELINE.json north_star) without a collective library, for the one-process-per-GPU host (bench.py
// --gather peer, parallel.PeerAllGather): every rank allocates its gathered buffer here, exports it (hipIpcGetMemHandle), opens its peers'
// and writes its own shard into EVERY peer's buffer at its own offset - N - 1 copies on N - 1 streams, i.e. over the N - 1 xGMI links of the GPU
// at once (41.9 MB per link, ~0.27 ms at 2^20 octopods, against ~1.9 ms for a ring that is bound by one link).  The
// copies are ordered after the caller's stream and the caller's stream after them; a barrier of the caller's (every rank has written) closes
// the exchange.  Same boundary as shc_fleet_all_gather_joints, which does this inside one process with hipMemcpyPeerAsync.
struct PeerPool {
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> done;
  hipEvent_t start = nullptr;
};
static PeerPool g_peer_pool[64];
static std::mutex g_peer_mutex;

extern "C" int shc_peer_alloc(int device, int64_t bytes, void **device_ptr, unsigned char *handle64) {
  if (!device_ptr || !handle64 || bytes < 1) return fail(SHC_ERR_INVALID_ARG, "shc_peer_alloc: device_ptr, handle (64 bytes) and a size");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "the exported handle is 64 bytes");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(device_ptr, size_t(bytes)));
  hipIpcMemHandle_t h;
  const hipError_t err = hipIpcGetMemHandle(&h, *device_ptr);
  if (err != hipSuccess) {
    (void)hipFree(*device_ptr);
    *device_ptr = nullptr;
    return fail(SHC_ERR_HIP, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(err) + " (HSA_ENABLE_IPC_MODE_LEGACY=0 must be set before the first HIP call)");
  }
  memcpy(handle64, &h, 64);
  return SHC_OK;
}
extern "C" int shc_peer_open(int device, const unsigned char *handle64, void **device_ptr) {
  if (!device_ptr || !handle64) return fail(SHC_ERR_INVALID_ARG, "shc_peer_open: handle and device_ptr");
  HIP_TRY(hipSetDevice(device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, 64);
  HIP_TRY(hipIpcOpenMemHandle(device_ptr, h, hipIpcMemLazyEnablePeerAccess));
  return SHC_OK;
}
// the copy streams / events shc_peer_scatter keeps per device: released when the rank frees its own gathered buffer (the exchange's lifetime)
static void peer_pool_release(int device) {
  if (device < 0 || device >= 64) return;
  std::lock_guard<std::mutex> lock(g_peer_mutex);
  PeerPool &pool = g_peer_pool[device];
  for (size_t k = 0; k < pool.streams.size(); ++k) {
    (void)hipStreamSynchronize(pool.streams[k]);
    (void)hipEventDestroy(pool.done[k]);
    (void)hipStreamDestroy(pool.streams[k]);
  }
  pool.streams.clear();
  pool.done.clear();
  if (pool.start) (void)hipEventDestroy(pool.start);
  pool.start = nullptr;
}
extern "C" int shc_peer_close(int device, void *device_ptr, int opened) {
  if (!device_ptr) return SHC_OK;
  HIP_TRY(hipSetDevice(device));
  if (opened) {
    HIP_TRY(hipIpcCloseMemHandle(device_ptr));
  } else {
    peer_pool_release(device);
    HIP_TRY(hipFree(device_ptr));
  }
  return SHC_OK;
}
// src (this device) -> dst[k] for k < n_dst, each copy on a stream of its own; ordered after `stream`, and `stream` is ordered after all of them
extern "C" int shc_peer_scatter(int device, const void *src, int64_t bytes, void *const *dst, int n_dst, void *stream) {
  if (!src || !dst || n_dst < 1 || bytes < 1) return fail(SHC_ERR_INVALID_ARG, "shc_peer_scatter: src, destinations and a size");
  if (device < 0 || device >= 64) return fail(SHC_ERR_INVALID_ARG, "device index");
  HIP_TRY(hipSetDevice(device));
  std::lock_guard<std::mutex> lock(g_peer_mutex);
  PeerPool &pool = g_peer_pool[device];
  if (!pool.start) HIP_TRY(hipEventCreateWithFlags(&pool.start, hipEventDisableTiming));
  while (int(pool.streams.size()) < n_dst) {
    hipStream_t s;
    hipEvent_t ev;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (const hipError_t err = hipEventCreateWithFlags(&ev, hipEventDisableTiming); err != hipSuccess) {
      (void)hipStreamDestroy(s);
      return fail(SHC_ERR_HIP, std::string("shc_peer_scatter: hipEventCreateWithFlags: ") + hipGetErrorString(err));
    }
    pool.streams.push_back(s);
    pool.done.push_back(ev);
  }
  hipStream_t main = (hipStream_t)stream;
  HIP_TRY(hipEventRecord(pool.start, main));
  for (int k = 0; k < n_dst; ++k) {
    HIP_TRY(hipStreamWaitEvent(pool.streams[k], pool.start, 0));
    HIP_TRY(hipMemcpyAsync(dst[k], src, size_t(bytes), hipMemcpyDeviceToDevice, pool.streams[k]));
    HIP_TRY(hipEventRecord(pool.done[k], pool.streams[k]));
    HIP_TRY(hipStreamWaitEvent(main, pool.done[k], 0));
  }
  return SHC_OK;
}
