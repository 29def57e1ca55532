// shc_fleet_io.hpp — fleet I/O, host and device forms: the five host setters (shc_fleet_set_velocity .. _set_joint_effort) and
// shc_fleet_set_inputs_device, the five host getters (shc_fleet_get_joint_state .. shc_fleet_scan_health) and shc_fleet_get_outputs_device,
// shc_fleet_order_after_stream, shc_fleet_order_stream_after, shc_fleet_set_io_chunk, shc_fleet_io_bytes.  Included by shc_fleet.hpp.  (K cycles
// per launch from K-deep device arrays - shc_fleet_step_k, shc_fleet_get_step_k_joints_device - is shc_fleet_step_k.hpp, built on what is here.)
//
// Every one of them translates between the caller's padded order and a part's dense order (shc_fleet_order.hpp: pick and place) and does nothing
// else: between a part's dense rows and its state stand the engine's own setters and getters, so every side effect of one - RT_TOUCHDOWN and
// touchdown detection, the first-effort switch, RT_MANUAL_LIVE, quaternion normalisation, the derived-tip refresh, inputs riding the two half
// streams of split steps - is the engine's, written once.  There is ONE walk over the inputs (fleet_inputs_walk: which engine setter is entered
// for which groups) and ONE over the outputs (fleet_outputs_walk: every output's engine getter, word size and padding), and two routes through
// each:
//   host route    the dense rows are the fleet's host scratch buffer, pick and place are the loops of shc_fleet_order.hpp, the engine calls are
//                 given on_device = 0 and a part is read in one piece.  Needs no single device and allocates nothing on one.
//   device route  the dense rows are the part's staging on the device, PACK and PLACE below are kernels on the part's own stream, the engine
//                 calls are given on_device = 1 and the record outputs walk a part in chunks.
//
// The device route's staging: one buffer per part, allocated by the fleet's first device I/O call and kept.  Every use of it is ordered on the part's stream: the
// engine getters join split steps before they write it, and a setter that scatters on the half streams orders the part's stream behind those
// reads (split_inputs_end), so the next pack cannot overwrite rows a half has not read yet.  Its size is the largest of
//   inputs:   rows x (16 + 3 L + L D) doubles   (all eight groups of one call - input_plan of shc_inputs.hpp -, packed by one launch),
//   joints:   rows x L x D doubles              (shc_engine_get_joint_state has no range: q, then qd, through the same rows),
//   records:  chunk x L x 512 bytes             (leg messages; leg frames + body frames of the same chunk need less, health 32 bytes a robot),
// with rows, L, D the part's own and chunk = min(rows, shc_fleet_set_io_chunk).  Record outputs walk the part in chunks through the engine
// calls' (first, count).  Default chunk: 8 192 robots - 32 MiB of octopod leg messages, which the place kernel reads back out of the 256 MiB
// last-level cache while six parts run side by side, and 64 chunks (two launches each) for a part of 2^19 robots.  A choice from that
// trade-off; the record outputs have not been timed (DESIGN 4.6 has the figures of the joint route).
#pragma once

static_assert(sizeof(shc_fleet_outputs) == 72 && offsetof(shc_fleet_outputs, frame) == 48 && offsetof(shc_fleet_outputs, health) == 56,
              "shc_fleet_outputs is six pointers, two int32, two pointers");
constexpr int64_t kFleetIoDefaultChunk = 8192;

// PACK: one launch per part, for one cycle or K.  Group g is an input array of the caller, [K][n][src_robot] doubles, of which a part's robot takes
// legs x k entries: entry (l, j) of part row r in cycle c is src[(c * n + ids[r]) * src_robot + l * src_leg + j] and lands at
// stage[dst + (c * rows + r) * legs * k + l * k + j], so that each staged group is a dense [K][rows][..] array (input_plan of shc_inputs.hpp).  The
// group is blockIdx.y and the cycle blockIdx.z, so both are wave-uniform (scalar loads of the kernel arguments), the stores of a group are one
// contiguous run, and - ids ascending - the loads walk the caller's array forwards, skipping the rows of other parts and the padding.  Bytes are
// copied as they are.
// Both kernels number their threads word by word in 64 bits, but divide in 32: a workgroup's first word is split into (row, column) once,
// wave-uniformly, and a thread adds its lane to the column - at most one row length plus 255, far inside 32 bits.
struct FleetPackGroup {
  const double *src;
  int64_t dst;       // doubles from the start of staging
  int32_t legs, k;   // per robot of the part
  int32_t src_robot; // doubles per robot in the caller's array
  int32_t src_leg;   // doubles per leg there (per-robot inputs: legs = 1)
};
struct FleetPackArgs {
  FleetPackGroup g[kInputGroups];
  int32_t n_groups;
};
// (the rows of one group: `dst` the group's staged rows, `src` the caller's array - both of ONE cycle)
__device__ __forceinline__ void fleet_pack_rows(double *__restrict__ dst, const double *__restrict__ src, const int64_t *__restrict__ ids, int64_t rows,
                                                const FleetPackGroup &g) {
  const uint32_t w = uint32_t(g.legs * g.k), gk = uint32_t(g.k);
  const int64_t total = rows * w, stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t0 = int64_t(blockIdx.x) * blockDim.x; t0 < total; t0 += stride) {
    const int64_t r0 = t0 / w; // uniform over the workgroup
    const uint32_t u = uint32_t(t0 - r0 * w) + threadIdx.x, dr = u / w, c = u - dr * w, l = c / gk, j = c - l * gk;
    const int64_t r = r0 + dr;
    if (r < rows) dst[r * w + c] = src[ids[r] * g.src_robot + int64_t(l) * g.src_leg + j];
  }
}
__global__ void fleet_pack_inputs_kernel(double *__restrict__ stage, const int64_t *__restrict__ ids, int64_t rows, int64_t n, FleetPackArgs a) {
  const FleetPackGroup &g = a.g[blockIdx.y];
  const int64_t cycle = blockIdx.z;
  fleet_pack_rows(stage + g.dst + cycle * rows * (g.legs * g.k), g.src + cycle * n * g.src_robot, ids, rows, g);
}

// PLACE: `count` rows of a part ([count][legs][k] words, dense, in staging) into the caller's buffer ([n][dst_legs][dst_k] words) at the rows
// ids[0 .. count).  One thread per word of a DESTINATION row, so that the stores of a robot are one contiguous run and every word of the row is
// written: a thread of a leg or joint the part's morphology lacks stores `pad` (the NaN of the joint arrays, zero for records).  Words are 8
// bytes (doubles, the 64 / 42 / 20 doubles of the leg message, leg frame and body frame records, the four words of a health record) or 4 (walk
// state).  Records are placed whole: legs = 1 .. L of k = dst_k words each.
template <class Word>
__global__ void fleet_place_kernel(Word *__restrict__ dst, const Word *__restrict__ part, const int64_t *__restrict__ ids, int64_t count, int legs, int k,
                                   int dst_legs, int dst_k, Word pad) {
  const uint32_t row = uint32_t(dst_legs * dst_k), dk = uint32_t(dst_k);
  const int64_t total = count * row, stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t0 = int64_t(blockIdx.x) * blockDim.x; t0 < total; t0 += stride) {
    const int64_t r0 = t0 / row; // uniform over the workgroup
    const uint32_t u = uint32_t(t0 - r0 * row) + threadIdx.x, dr = u / row, c = u - dr * row, l = c / dk, j = c - l * dk;
    const int64_t r = r0 + dr;
    if (r >= count) continue;
    Word v = pad;
    if (l < uint32_t(legs) && j < uint32_t(k)) v = part[(r * legs + l) * k + j];
    dst[ids[r] * row + c] = v;
  }
}
// one word per thread: at most 2 048 workgroups along x - shared among the cycles of a launch that has `cycles` of them along another grid
// dimension -, the rest by the grid stride
static unsigned fleet_io_grid(int64_t threads, int cycles = 1) { return unsigned(std::max<int64_t>(1, std::min<int64_t>((threads + 255) / 256, 2048 / cycles))); }
// the bit pattern shc_fleet_get_joint_state fills the padding with
static uint64_t nan_word() {
  const double nan_value = std::nan("");
  uint64_t word;
  memcpy(&word, &nan_value, 8);
  return word;
}

// PLACE on `stream`: the dense `rows` of a part into dst at `ids` (Word: that of the padding)
template <class Word>
static int fleet_place(hipStream_t stream, void *dst, const void *rows, const int64_t *ids, int64_t count, int legs, int k, int dst_legs, int dst_k, Word pad) {
  fleet_place_kernel<Word><<<dim3(fleet_io_grid(count * dst_legs * dst_k)), dim3(256), 0, stream>>>(static_cast<Word *>(dst), static_cast<const Word *>(rows), ids, count, legs, k,
                                                                                                 dst_legs, dst_k, pad);
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

// The rows of input group g for a part - the group table's entry at the part's (legs, dof) on the dense side and the fleet's padded (max_legs,
// max_dof) on the caller's: what the pack kernel and the host pick both read
static FleetRows fleet_input_rows(const shc_fleet *f, const FleetPart &p, int g) {
  const shc_params &pp = f->params[p.morph];
  return fleet_rows(input_per_leg(g), input_group(g).width, pp.leg_count, max_dof(pp), f->max_legs, f->max_dof);
}
// The K-deep staging of the groups of `mask` for a part (K = 1: the inputs of one set call), and the pack launch that fills it at `stage` from the
// caller's arrays on the part's stream: every selected group of the table
static InputPlan fleet_input_plan(const shc_fleet *f, const FleetPart &p, unsigned mask, int K) {
  const shc_params &pp = f->params[p.morph];
  return input_plan(mask, int64_t(p.ids.size()), pp.leg_count, max_dof(pp), K);
}
static int fleet_pack(const shc_fleet *f, const FleetPart &p, const shc_fleet_inputs *in, const InputPlan &plan, int K, double *stage) {
  const int64_t rows = int64_t(p.ids.size());
  FleetPackArgs a{};
  int64_t widest = 0;
  for (int g = 0; g < kInputGroups; ++g) {
    if (plan.at[g] < 0) continue;
    FleetPackGroup &pg = a.g[a.n_groups++];
    const FleetRows r = fleet_input_rows(f, p, g);
    pg.src = in->*kFleetInput[g], pg.dst = plan.at[g];
    pg.legs = r.legs, pg.k = r.k, pg.src_robot = r.src_robot, pg.src_leg = r.src_leg;
    widest = std::max<int64_t>(widest, rows * pg.legs * pg.k);
  }
  HIP_TRY(hipSetDevice(p.device));
  fleet_pack_inputs_kernel<<<dim3(fleet_io_grid(widest, K), unsigned(a.n_groups), unsigned(K)), dim3(256), 0, p.engine->stream>>>(stage, p.d_ids, rows, f->n, a);
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

static int64_t fleet_io_chunk_of(const shc_fleet *f, const FleetPart &p) {
  return std::min<int64_t>(int64_t(p.ids.size()), f->io_chunk > 0 ? f->io_chunk : kFleetIoDefaultChunk);
}
static size_t fleet_io_stage_bytes(const shc_fleet *f, const FleetPart &p) {
  const shc_params &pp = f->params[p.morph];
  const size_t rows = p.ids.size(), L = size_t(pp.leg_count), D = size_t(max_dof(pp));
  const size_t inputs = size_t(fleet_input_plan(f, p, kAllInputs, 1).doubles) * 8, joints = rows * L * D * 8;
  const size_t records = size_t(fleet_io_chunk_of(f, p)) * L * sizeof(shc_leg_state_msg);
  static_assert(sizeof(shc_leg_frames) + sizeof(shc_body_frames) <= sizeof(shc_leg_state_msg), "a chunk of leg messages is the largest record output");
  return (std::max(inputs, std::max(joints, records)) + 15) & ~size_t(15);
}

// What all four device entry points ask before they do anything: one device, nobody in resident mode.
static int fleet_io_ready(const shc_fleet *f) {
  for (const auto &p : f->parts) {
    if (p.device != f->parts[0].device)
      return fail(SHC_ERR_UNSUPPORTED, "device I/O needs one device that holds every part of the fleet (the caller's arrays live on one): use the host forms");
    if (resident_active(p.engine))
      return fail(SHC_ERR_BUSY, "a part of the fleet is in resident mode: only shc_engine_resident_* calls are valid until shc_engine_resident_end");
  }
  return SHC_OK;
}
// The first device I/O call of a fleet (and the first after shc_fleet_set_io_chunk): ids, staging and events of every part.  Allocates and
// uploads synchronously; later calls find everything in place.
static int fleet_io_prepare(shc_fleet *f) {
  if (f->io_ready) return SHC_OK;
  for (auto &p : f->parts) {
    int rc = fleet_part_ids(p);
    if (rc != SHC_OK) return rc;
    HIP_TRY(hipSetDevice(p.device));
    if (!p.io_stage) {
      const size_t bytes = fleet_io_stage_bytes(f, p);
      HIP_TRY(hipMalloc(&p.io_stage, bytes));
      p.io_stage_bytes = bytes;
    }
    if (!p.io_after) HIP_TRY(hipEventCreateWithFlags(&p.io_after, hipEventDisableTiming));
    if (!p.io_before) HIP_TRY(hipEventCreateWithFlags(&p.io_before, hipEventDisableTiming));
  }
  f->io_ready = true;
  return SHC_OK;
}

// The fleet forms of the row passes (shc_rows.hpp; shc_fleet_observe.hpp, shc_fleet_actions.hpp, shc_fleet_footholds.hpp), straight between the
// caller's device array and the parts' states.  What every one asks before anything changes: the spec (P: its description for row_layout), the
// fleet's shape, the array `rows` (named `what` in the messages), one device, and every part - check(engine) - before the first launch.
template <class P, class Check>
static int fleet_rows_begin(const shc_fleet *f, const typename P::Spec *spec, const void *rows, const char *what, RowLayout &lay, Check &&check) {
  if (!f || !spec || !rows) return fail(SHC_ERR_INVALID_ARG, std::string("fleet, spec or ") + what + " NULL");
  if (const int bad = row_resolve<P>(spec, lay)) return bad;
  bool below = spec->legs < f->max_legs;
  if constexpr (P::has_dof) below = below || spec->dof < f->max_dof;
  if (below) return fail(SHC_ERR_INVALID_ARG, std::string(P::name) + (P::has_dof ? ".legs / dof are" : ".legs is") + " below the fleet's shape (shc_fleet_shape)");
  int rc = row_aligned(rows, spec->dtype, what);
  if (rc == SHC_OK) rc = fleet_io_ready(f);
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i) rc = check(f->parts[i].engine);
  return rc;
}
// ... and then: device I/O prepared, part(p, row stride) for every part - its caller ids (p.d_ids) are the kernels' row table.  Nothing is staged;
// the rows of the parts are disjoint, so the parts' streams need no order among themselves.
template <class Spec, class Part>
static int fleet_rows_each(shc_fleet *f, const Spec *spec, const RowLayout &lay, Part &&part) {
  int rc = fleet_io_prepare(f);
  const int64_t stride = row_stride_of(spec, lay);
  for (size_t i = 0; rc == SHC_OK && i < f->parts.size(); ++i) rc = part(f->parts[i], stride);
  return rc;
}
// (a part's stream follows both halves of split steps in flight first)
static int fleet_part_join(FleetPart &p) {
  HIP_TRY(hipSetDevice(p.device));
  return shc_engine_join(p.engine);
}

extern "C" int shc_fleet_set_io_chunk(shc_fleet *f, int64_t robots) {
  if (!f || robots < 0) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL or a negative chunk");
  if (robots == f->io_chunk) return SHC_OK;
  for (auto &p : f->parts) { // staging is sized by the chunk: drain the part, release it, and let the next device I/O call allocate it again
    if (!p.io_stage) continue; // (the K-deep staging of shc_fleet_step_k does not depend on the chunk: it stays)
    HIP_TRY(hipSetDevice(p.device));
    if (p.engine->side_busy) HIP_TRY(hipDeviceSynchronize()); // (a half stream may still read staged inputs)
    HIP_TRY(hipStreamSynchronize(p.engine->stream));
    HIP_TRY(hipFree(p.io_stage));
    p.io_stage = nullptr, p.io_stage_bytes = 0;
  }
  f->io_chunk = robots;
  f->io_ready = false;
  return SHC_OK;
}
extern "C" int64_t shc_fleet_io_bytes(const shc_fleet *f) {
  int64_t bytes = 0;
  if (f)
    for (const auto &p : f->parts)
      bytes += int64_t(p.io_stage_bytes) + int64_t(p.k_stage_bytes) + (p.d_ids ? int64_t(p.ids.size()) * 8 : 0); // (the ids stay when shc_fleet_set_io_chunk releases the staging)
  return bytes;
}

extern "C" int shc_fleet_order_after_stream(shc_fleet *f, void *stream) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  int rc = fleet_io_ready(f);
  if (rc == SHC_OK) rc = fleet_io_prepare(f);
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipSetDevice(f->parts[0].device));
  for (auto &p : f->parts) { // (inputs that ride the half streams of split steps follow the part's stream: split_inputs_begin)
    HIP_TRY(hipEventRecord(p.io_after, hipStream_t(stream)));
    HIP_TRY(hipStreamWaitEvent(p.engine->stream, p.io_after, 0));
  }
  return SHC_OK;
}
extern "C" int shc_fleet_order_stream_after(shc_fleet *f, void *stream) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  int rc = fleet_io_ready(f);
  if (rc == SHC_OK) rc = fleet_io_prepare(f);
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipSetDevice(f->parts[0].device));
  for (auto &p : f->parts) {
    if ((rc = shc_engine_join(p.engine)) != SHC_OK) return rc; // split steps in flight: the part's stream follows both halves first
    HIP_TRY(hipEventRecord(p.io_before, p.engine->stream));
    HIP_TRY(hipStreamWaitEvent(hipStream_t(stream), p.io_before, 0));
  }
  return SHC_OK;
}


// ================================================================================================ the two routes, the two walks
// What a walk asks of a route: on_device, handed to the engine's calls; rows(f, p, bytes), where a part's dense rows go; chunk(f, p), the
// robots per pass of the record outputs; pick, the part's rows of the groups of `plan` out of the caller's arrays into `rows`; place, `count`
// dense rows into the caller's buffer at the part's ids from `first` on.
struct FleetHostRoute {
  static constexpr int on_device = 0;
  static char *rows(shc_fleet *f, const FleetPart &, size_t bytes) { return f->scratch.room(bytes); }
  static int64_t chunk(const shc_fleet *, const FleetPart &p) { return int64_t(p.ids.size()); }
  static int pick(const shc_fleet *f, const FleetPart &p, const shc_fleet_inputs *in, const InputPlan &plan, double *rows) {
    for (int g = 0; g < kInputGroups; ++g)
      if (plan.at[g] >= 0) fleet_pick_host(rows + plan.at[g], in->*kFleetInput[g], p.ids.data(), int64_t(p.ids.size()), fleet_input_rows(f, p, g));
    return SHC_OK;
  }
  template <class Word>
  static int place(const FleetPart &p, void *dst, const void *rows, int64_t first, int64_t count, int legs, int k, int dst_legs, int dst_k, Word pad) {
    fleet_place_host(static_cast<Word *>(dst), static_cast<const Word *>(rows), p.ids.data() + first, count, legs, k, dst_legs, dst_k, pad);
    return SHC_OK;
  }
};
struct FleetDeviceRoute {
  static constexpr int on_device = 1;
  static char *rows(shc_fleet *, const FleetPart &p, size_t) { return p.io_stage; } // (fleet_io_prepare has sized it: fleet_io_stage_bytes)
  static int64_t chunk(const shc_fleet *f, const FleetPart &p) { return fleet_io_chunk_of(f, p); }
  static int pick(const shc_fleet *f, const FleetPart &p, const shc_fleet_inputs *in, const InputPlan &plan, double *rows) { return fleet_pack(f, p, in, plan, 1, rows); }
  template <class Word>
  static int place(const FleetPart &p, void *dst, const void *rows, int64_t first, int64_t count, int legs, int k, int dst_legs, int dst_k, Word pad) {
    return fleet_place(p.engine->stream, dst, rows, p.d_ids + first, count, legs, k, dst_legs, dst_k, pad);
  }
};

// The walk over the inputs: per part, the rows of the groups given are picked into one dense block (input_plan) and handed to the engine's
// setters.  `enter` names groups whose setter is entered on every part although no array is given; with the groups given they decide which
// setters run.  A setter none of whose groups is named is not called: with nothing to set it would still enter the engine, and some of them
// join split steps - a caller who sends velocity alone never joins them through the effort or force setter.
template <class Route>
static int fleet_inputs_walk(shc_fleet *f, const shc_fleet_inputs *in, unsigned enter) {
  const unsigned mask = input_mask(in);
  enter |= mask;
  if (enter == 0) return SHC_OK; // every input is held
  auto entered = [enter](int g) { return ((enter >> g) | (enter >> input_group(g).with)) & 1u; };
  constexpr int dev = Route::on_device;
  for (auto &p : f->parts) {
    const InputPlan plan = fleet_input_plan(f, p, mask, 1);
    double *rows = reinterpret_cast<double *>(Route::rows(f, p, size_t(plan.doubles) * 8));
    int rc = Route::pick(f, p, in, plan, rows);
    if (rc != SHC_OK) return rc;
    const shc_cycle_inputs s = input_plan_arrays(plan, rows);
    if (entered(SHC_ACT_LINEAR_XY) && (rc = shc_engine_set_velocity(p.engine, s.linear_xy, s.angular, dev)) != SHC_OK) return rc;
    if (entered(SHC_ACT_IMU_ORIENTATION) && (rc = shc_engine_set_imu(p.engine, s.imu_orientation_wxyz, s.imu_angular_velocity, dev)) != SHC_OK) return rc;
    if (entered(SHC_ACT_POSE_TRANSLATION_VELOCITY) && (rc = shc_engine_set_pose_input(p.engine, s.pose_translation_velocity, s.pose_rotation_velocity, dev)) != SHC_OK) return rc;
    if (entered(SHC_ACT_TIP_FORCE) && (rc = shc_engine_set_tip_force(p.engine, s.tip_force, dev)) != SHC_OK) return rc;
    if (entered(SHC_ACT_JOINT_EFFORT) && (rc = shc_engine_set_joint_effort(p.engine, s.joint_effort, dev)) != SHC_OK) return rc;
  }
  return SHC_OK;
}

// The walk over the outputs: per part q, qd and the walk state in one piece, then chunk by chunk the leg messages, leg and body frames from one
// engine pass, and health - each read densely by the engine's getter and placed.  q / qd: [n][max_legs][max_dof], the bits of std::nan("")
// where a morphology has no such leg or joint; records: [n][max_legs] or [n], those of legs a robot does not have all zero.  Every word of
// every buffer given is written.
template <class Route>
static int fleet_outputs_walk(shc_fleet *f, const shc_fleet_outputs *out) {
  constexpr int dev = Route::on_device, kMsgWords = int(sizeof(shc_leg_state_msg) / 8), kLegWords = int(sizeof(shc_leg_frames) / 8),
                kBodyWords = int(sizeof(shc_body_frames) / 8), kHealthWords = int(sizeof(shc_robot_health) / 8);
  const bool frames = out->leg_frames || out->body_frames;
  const uint64_t zero = 0;
  int rc;
  for (auto &p : f->parts) {
    const shc_params &pp = f->params[p.morph];
    const int L = pp.leg_count, D = max_dof(pp);
    const int64_t rows = int64_t(p.ids.size()), chunk = Route::chunk(f, p);
    HIP_TRY(hipSetDevice(p.device));
    // q, then qd, through the same dense rows: the device staging holds one joint array of a part.  The host route follows - two engine calls
    // (two enters, two copies back with their waits) where one call with both arrays would do; the bytes are the same, and what the walk
    // saves the host route elsewhere is far more (profiles/bench/fleet_order_ab.json)
    for (int which = 0; which < 2; ++which) {
      double *dst = which == 0 ? out->q : out->qd;
      if (!dst) continue;
      double *dense = reinterpret_cast<double *>(Route::rows(f, p, size_t(rows) * L * D * 8));
      if ((rc = shc_engine_get_joint_state(p.engine, which == 0 ? dense : nullptr, which == 0 ? nullptr : dense, dev)) != SHC_OK) return rc;
      if ((rc = Route::place(p, dst, dense, 0, rows, L, D, f->max_legs, f->max_dof, nan_word())) != SHC_OK) return rc;
    }
    if (out->walk_state) {
      int32_t *dense = reinterpret_cast<int32_t *>(Route::rows(f, p, size_t(rows) * 4));
      if ((rc = shc_engine_get_body_state(p.engine, nullptr, nullptr, dense, dev)) != SHC_OK) return rc;
      if ((rc = Route::place(p, out->walk_state, dense, 0, rows, 1, 1, 1, 1, int32_t(0))) != SHC_OK) return rc;
    }
    for (int64_t first = 0; first < rows; first += chunk) {
      const int64_t count = std::min(chunk, rows - first);
      if (out->leg_state_msgs) {
        auto *dense = reinterpret_cast<shc_leg_state_msg *>(Route::rows(f, p, size_t(count) * L * sizeof(shc_leg_state_msg)));
        if ((rc = shc_engine_get_leg_state_msgs(p.engine, first, count, dense, dev)) != SHC_OK) return rc;
        if ((rc = Route::place(p, out->leg_state_msgs, dense, first, count, L, kMsgWords, f->max_legs, kMsgWords, zero)) != SHC_OK) return rc;
      }
      if (frames) { // one engine pass for both; the body records sit behind the chunk's leg records
        const size_t leg_bytes = out->leg_frames ? size_t(count) * L * sizeof(shc_leg_frames) : 0;
        char *legs = Route::rows(f, p, leg_bytes + size_t(count) * sizeof(shc_body_frames)), *body = legs + leg_bytes;
        rc = shc_engine_get_frame_transforms(p.engine, first, count, out->frame, out->leg_frames ? reinterpret_cast<shc_leg_frames *>(legs) : nullptr,
                                             out->body_frames ? reinterpret_cast<shc_body_frames *>(body) : nullptr, dev);
        if (rc != SHC_OK) return rc;
        if (out->leg_frames && (rc = Route::place(p, out->leg_frames, legs, first, count, L, kLegWords, f->max_legs, kLegWords, zero)) != SHC_OK) return rc;
        if (out->body_frames && (rc = Route::place(p, out->body_frames, body, first, count, 1, kBodyWords, 1, kBodyWords, zero)) != SHC_OK) return rc;
      }
      if (out->health) {
        auto *dense = reinterpret_cast<shc_robot_health *>(Route::rows(f, p, size_t(count) * sizeof(shc_robot_health)));
        if ((rc = shc_engine_scan_health(p.engine, first, count, out->criteria, dense, nullptr, nullptr, nullptr, dev)) != SHC_OK) return rc;
        if ((rc = Route::place(p, out->health, dense, first, count, 1, kHealthWords, 1, kHealthWords, zero)) != SHC_OK) return rc;
      }
    }
  }
  return SHC_OK;
}

// ================================================================================================ the host forms
// A setter of per-robot groups enters its engine setter on every part even when both arrays are NULL (a part in resident mode answers
// SHC_ERR_BUSY, split steps are joined); a per-leg setter given NULL returns without entering an engine.  Per-leg inputs arrive padded,
// [n][max_legs][max_k]: entries beyond a morphology's (legs, k) are ignored.
static int fleet_set_host(shc_fleet *f, int g, const double *a, const double *b = nullptr) { // group g, and for a per-robot group the one it is given with
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  shc_fleet_inputs in{};
  in.*kFleetInput[input_group(g).with] = b, in.*kFleetInput[g] = a;
  return fleet_inputs_walk<FleetHostRoute>(f, &in, input_per_leg(g) ? 0 : 1u << g);
}
extern "C" int shc_fleet_set_velocity(shc_fleet *f, const double *linear_xy, const double *angular) { return fleet_set_host(f, SHC_ACT_LINEAR_XY, linear_xy, angular); }
extern "C" int shc_fleet_set_imu(shc_fleet *f, const double *orientation_wxyz, const double *angular_velocity) {
  return fleet_set_host(f, SHC_ACT_IMU_ORIENTATION, orientation_wxyz, angular_velocity);
}
extern "C" int shc_fleet_set_pose_input(shc_fleet *f, const double *translation_velocity, const double *rotation_velocity) {
  return fleet_set_host(f, SHC_ACT_POSE_TRANSLATION_VELOCITY, translation_velocity, rotation_velocity);
}
extern "C" int shc_fleet_set_tip_force(shc_fleet *f, const double *tip_force) { return fleet_set_host(f, SHC_ACT_TIP_FORCE, tip_force); }
extern "C" int shc_fleet_set_joint_effort(shc_fleet *f, const double *joint_effort) { return fleet_set_host(f, SHC_ACT_JOINT_EFFORT, joint_effort); }

// The getters: an argument check, the outputs asked for, the walk.  What an engine refuses (a part in resident mode, an unknown frame,
// odometry off, criteria) is refused by the first part that objects.
extern "C" int shc_fleet_get_joint_state(shc_fleet *f, double *q, double *qd) {
  if (!f) return fail(SHC_ERR_INVALID_ARG, "fleet is NULL");
  shc_fleet_outputs out{};
  out.q = q, out.qd = qd;
  if (q || qd) return fleet_outputs_walk<FleetHostRoute>(f, &out);
  // nothing to read, so nothing for the walk to do - but shc_engine_get_joint_state(NULL, NULL) still entered every part (SHC_ENTER_JOINED: a
  // part in resident mode answers SHC_ERR_BUSY, split steps are joined), and shc_engine_join is exactly that entry
  for (auto &p : f->parts)
    if (const int rc = shc_engine_join(p.engine)) return rc;
  return SHC_OK;
}
extern "C" int shc_fleet_get_walk_state(shc_fleet *f, int32_t *walk_state) {
  if (!f || !walk_state) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  shc_fleet_outputs out{};
  out.walk_state = walk_state;
  return fleet_outputs_walk<FleetHostRoute>(f, &out);
}
// publishLegState of every robot: msgs[i * max_legs + l]
extern "C" int shc_fleet_get_leg_state_msgs(shc_fleet *f, shc_leg_state_msg *msgs) {
  if (!f || !msgs) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  shc_fleet_outputs out{};
  out.leg_state_msgs = msgs;
  return fleet_outputs_walk<FleetHostRoute>(f, &out);
}
// publishFrameTransforms of every robot: legs[i * max_legs + l] and body[i] (either may be NULL)
extern "C" int shc_fleet_get_frame_transforms(shc_fleet *f, int frame, shc_leg_frames *legs, shc_body_frames *body) {
  if (!f || (!legs && !body)) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  shc_fleet_outputs out{};
  out.leg_frames = legs, out.body_frames = body, out.frame = frame;
  return fleet_outputs_walk<FleetHostRoute>(f, &out);
}
// shc_engine_scan_health of every part: the records
extern "C" int shc_fleet_scan_health(shc_fleet *f, const shc_health_criteria *criteria, shc_robot_health *health) {
  if (!f || !health) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  shc_fleet_outputs out{};
  out.health = health, out.criteria = criteria;
  return fleet_outputs_walk<FleetHostRoute>(f, &out);
}

// ================================================================================================ the device forms
extern "C" int shc_fleet_set_inputs_device(shc_fleet *f, const shc_fleet_inputs *in) {
  if (!f || !in) return fail(SHC_ERR_INVALID_ARG, "fleet or inputs NULL");
  int rc = fleet_io_ready(f);
  if (rc == SHC_OK) rc = fleet_io_prepare(f);
  return rc != SHC_OK ? rc : fleet_inputs_walk<FleetDeviceRoute>(f, in, 0);
}

extern "C" int shc_fleet_get_outputs_device(shc_fleet *f, const shc_fleet_outputs *out) {
  if (!f || !out) return fail(SHC_ERR_INVALID_ARG, "fleet or outputs NULL");
  const bool frames = out->leg_frames || out->body_frames;
  if (!out->q && !out->qd && !out->walk_state && !out->leg_state_msgs && !frames && !out->health) return fail(SHC_ERR_INVALID_ARG, "every output is NULL");
  if (out->reserved != 0) return fail(SHC_ERR_INVALID_ARG, "shc_fleet_outputs.reserved must be 0");
  if (frames && out->frame != SHC_FRAME_BASE_LINK && out->frame != SHC_FRAME_ODOM_IDEAL) return fail(SHC_ERR_INVALID_ARG, "unknown frame");
  if ((reinterpret_cast<uintptr_t>(out->leg_state_msgs) | reinterpret_cast<uintptr_t>(out->leg_frames) | reinterpret_cast<uintptr_t>(out->body_frames) |
       reinterpret_cast<uintptr_t>(out->health)) & 15)
    return fail(SHC_ERR_INVALID_ARG, "record buffers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(out->q) | reinterpret_cast<uintptr_t>(out->qd)) & 7 || reinterpret_cast<uintptr_t>(out->walk_state) & 3)
    return fail(SHC_ERR_INVALID_ARG, "q / qd must be 8-byte aligned, walk_state 4-byte aligned");
  if (out->health) { // (what shc_engine_scan_health would refuse, before the first part has run)
    const shc_health_criteria crit = health_criteria(out->criteria);
    if (crit.reserved != 0) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.reserved must be 0");
    if (crit.select & ~kHealthAllFlags) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.select has bits outside SHC_HEALTH_*");
  }
  int rc = fleet_io_ready(f);
  if (rc != SHC_OK) return rc;
  if (out->body_frames || (out->leg_frames && out->frame == SHC_FRAME_ODOM_IDEAL))
    for (const auto &p : f->parts)
      if (!p.engine->cp.odometry) return fail(SHC_ERR_UNSUPPORTED, "SHC_FEAT_ODOMETRY is off on a part: odom_to_base_link needs the ideal odometry");
  if ((rc = fleet_io_prepare(f)) != SHC_OK) return rc;
  return fleet_outputs_walk<FleetDeviceRoute>(f, out);
}
