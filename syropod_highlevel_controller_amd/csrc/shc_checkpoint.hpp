// shc_checkpoint.hpp — device checkpoints: shc_engine_checkpoint_create / update, shc_engine_restore_instances.  The state of every
// instance, copied plane by plane into device memory of its own, and an indexed restore from it: instance i <- the checkpoint's instance
// source[i], for any subset of the batch, in one kernel on the engine's stream.  Included by shc_engine.hip below shc_snapshot.hpp.
//
// The host route (shc_engine_get_state / set_state + get_aux_state / set_aux_state, shc_snapshot.hpp) defines the result: a restored
// instance reads back, and walks on, as if its source's records had been read at capture time and injected at restore time.  What that
// route moves is what the tables below call state or output; the held inputs stay with the destination ("inputs are inputs: the caller
// applies them again"), and the robot tile's LDS-only fields have no meaning in HBM.
#pragma once

#include "shc_cycle.hpp"

namespace shc {

// ---- the one classification of every field index.  The restore kernel's plane / field lists are generated from these tables.
enum : int { CK_STATE = 0, CK_INPUT = 1, CK_OUTPUT = 2, CK_LDS_ONLY = 3 };
struct CkRange {
  int begin, end, cls; // fields [begin, end)
};
template <int NJ>
struct LegFieldClasses {
  using F = Fields<NJ>;
  static constexpr int kRanges = 4;
  static constexpr CkRange range[kRanges] = {
      {F::Q, F::FORCE_IN, CK_STATE},          // joints, the stepper's tips / origins / stride, admittance state, tip-force filter state
      {F::FORCE_IN, F::POSER_TIP, CK_INPUT},  // FORCE_IN, EFFORT_IN
      {F::POSER_TIP, F::ORG_DIR, CK_OUTPUT},  // POSER_TIP (state while the LegPoser tips of a plan call are current), MODEL_TIP, ADM_DELTA (+ the published stiffness)
      {F::ORG_DIR, F::COUNT, CK_STATE}};      // tip directions, DES_TIP / DES_DIR, the LegPoser sequence state, STEP_PLANE, MEAS_Q
  static constexpr int count = F::COUNT;
};
struct RobotFieldClasses {
  using R = RobotFields;
  static constexpr int kRanges = 10;
  static constexpr CkRange range[kRanges] = {
      {R::VLIN, R::VIN, CK_STATE},       // desired velocity, walk planes, origin walk-plane pose
      {R::VIN, R::CORE_END, CK_INPUT},   // VIN, WIN
      {R::MPOSE, R::GYRO, CK_STATE},     // manual pose and its velocity inputs (part of the state record), IMU PID state
      {R::GYRO, R::APREV, CK_INPUT},     // GYRO, IMUQ
      {R::APREV, R::CPOSE, CK_STATE},    // previous auto-pose rotation
      {R::CPOSE, R::WPP, CK_OUTPUT},     // Model::current_pose_
      {R::WPP, R::ODOM, CK_LDS_ONLY},    // walk_plane_pose_ of the current cycle
      {R::ODOM, R::INCL, CK_STATE},      // ideal odometry
      {R::INCL, R::TALIGN, CK_OUTPUT},   // inclination pose
      {R::TALIGN, R::COUNT, CK_STATE}};  // tip-align poses
  static constexpr int count = R::COUNT;
};
// the class of field f, -1 where no range or more than one range holds it
template <class T>
constexpr int ck_field_class(int f) {
  int cls = -1, hits = 0;
  for (int k = 0; k < T::kRanges; ++k)
    if (f >= T::range[k].begin && f < T::range[k].end) cls = T::range[k].cls, ++hits;
  return hits == 1 ? cls : -1;
}
template <class T>
constexpr bool ck_classified_once() {
  for (int f = 0; f < T::count; ++f)
    if (ck_field_class<T>(f) < 0) return false;
  return true;
}
constexpr bool ck_copied(int cls) { return cls == CK_STATE || cls == CK_OUTPUT; }
static_assert(ck_classified_once<LegFieldClasses<3>>() && ck_classified_once<LegFieldClasses<4>>() && ck_classified_once<LegFieldClasses<5>>() &&
                  ck_classified_once<RobotFieldClasses>(),
              "every field index belongs to exactly one class");

// The 16-byte planes of the leg fields a restore moves (a plane holds fields 2p and 2p + 1).  The two POSER_TIP planes are left out: they
// move only while they are state (CK_LIVE_POSER_TIPS), as in the auxiliary blob.
template <int NJ>
struct LegCopyPlanes {
  int n;
  int p[Fields<NJ>::COUNT / 2];
};
template <int NJ>
constexpr LegCopyPlanes<NJ> leg_copy_planes() {
  using F = Fields<NJ>;
  LegCopyPlanes<NJ> r{};
  for (int p = 0; p < F::COUNT / 2; ++p)
    if (ck_copied(ck_field_class<LegFieldClasses<NJ>>(2 * p)) && !(2 * p >= F::POSER_TIP && 2 * p < F::POSER_TIP + 4)) r.p[r.n++] = p;
  return r;
}
template <int NJ>
constexpr bool ck_planes_whole() { // both fields of a plane move, or neither
  for (int p = 0; p < Fields<NJ>::COUNT / 2; ++p)
    if (ck_copied(ck_field_class<LegFieldClasses<NJ>>(2 * p)) != ck_copied(ck_field_class<LegFieldClasses<NJ>>(2 * p + 1))) return false;
  return Fields<NJ>::POSER_TIP % 2 == 0;
}
static_assert(ck_planes_whole<3>() && ck_planes_whole<4>() && ck_planes_whole<5>(), "a class boundary cuts a 16-byte plane");
// bit f of word f / 64: robot field f moves
struct RobotCopyMask {
  uint64_t w[2];
};
constexpr RobotCopyMask robot_copy_mask() {
  RobotCopyMask m{};
  for (int f = 0; f < RobotFields::COUNT; ++f)
    if (ck_copied(ck_field_class<RobotFieldClasses>(f))) m.w[f >> 6] |= uint64_t(1) << (f & 63);
  return m;
}
static_assert(RobotFields::COUNT <= 128, "robot_copy_mask holds 128 fields");

// the records an engine holds at capture time, as the header of an auxiliary blob names them (AuxHeader::flags)
enum : uint32_t { CK_LIVE_MANUAL = 1, CK_LIVE_EXT = 2, CK_LIVE_SEQ = 4, CK_LIVE_POSER_TIPS = 8 };

// the checkpoint's arrays, in the engine's own layouts
struct CheckpointView {
  const double2 *legd;
  const int32_t *legi;
  const double *robd;
  const int32_t *robi;
  const double2 *ext;
  const ManualRobot *manual;
  const SeqRobotState *seq;
  uint32_t live; // CK_LIVE_*
};

constexpr int kRestoreBatch = 8; // independent 16-byte loads in flight per lane before the first store

// planes[p[k]] of slot `src` -> the same planes of slot `dst`, kRestoreBatch loads ahead of their stores
template <int N, class PlaneOf>
__device__ __forceinline__ void restore_planes(double2 *__restrict__ to, const double2 *__restrict__ from, int64_t n_slots, int64_t dst, int64_t src, PlaneOf plane_of) {
#pragma unroll
  for (int b = 0; b < N; b += kRestoreBatch) {
    double2 v[kRestoreBatch];
#pragma unroll
    for (int k = 0; k < kRestoreBatch; ++k)
      if (b + k < N) v[k] = from[int64_t(plane_of(b + k)) * n_slots + src];
#pragma unroll
    for (int k = 0; k < kRestoreBatch; ++k)
      if (b + k < N) to[int64_t(plane_of(b + k)) * n_slots + dst] = v[k];
  }
}
// 4-byte words [0, words) of a per-robot record, spread over the L lanes of the robot's group; from == nullptr clears them
template <int L>
__device__ __forceinline__ void restore_words(int32_t *__restrict__ to, const int32_t *__restrict__ from, int words, int leg) {
#pragma unroll 4
  for (int i = leg; i < words; i += L) to[i] = from ? from[i] : 0;
}

// One leg per lane, floor(64 / L) robots per wavefront (the cycle's slot mapping), one wavefront per workgroup: block w serves the robots
// of wavefront w.  Every lane of a robot's group reads the same source[rob] (one request); a source that is the robot itself, or any
// source at the same place in its wavefront, makes each plane one contiguous 16 B-per-lane load and store, any other source costs a
// gather on the load side only.  The stores always go to the lane's own slot.  A source outside [0, n) leaves the robot alone - the
// guard is on the value, so a bad entry of a device map cannot address anything.  No LDS, no atomics: a map names no destination twice,
// and the checkpoint is never written here.
template <int L, int NJ>
__global__ __launch_bounds__(64) void restore_instances_kernel(DevState st, SeqRobotState *__restrict__ seq, const CheckpointView ck,
                                                               const int64_t *__restrict__ source) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  const int lane = threadIdx.x;
  const int gi = lane / L, leg = lane - gi * L;
  const int64_t w = blockIdx.x, rob = w * rpw + gi, n = st.n_robots;
  if (gi >= rpw || rob >= n) return;
  const int64_t src = source ? source[rob] : rob;
  if (src < 0 || src >= n) return;
  const int64_t sw = src / rpw;
  const int sgi = int(src - sw * rpw);
  const int64_t dst_slot = w * 64 + lane, src_slot = sw * 64 + sgi * L + leg; // slot_of(rob, leg, L), slot_of(src, leg, L)
  const int64_t ns = st.n_slots;

  // ---- leg planes
  constexpr LegCopyPlanes<NJ> planes = leg_copy_planes<NJ>();
  restore_planes<planes.n>(reinterpret_cast<double2 *>(st.legd), ck.legd, ns, dst_slot, src_slot, [&](int k) { return planes.p[k]; });
  if (ck.live & CK_LIVE_POSER_TIPS)
    restore_planes<2>(reinterpret_cast<double2 *>(st.legd), ck.legd, ns, dst_slot, src_slot, [](int k) { return FD::POSER_TIP / 2 + k; });
  st.legi[dst_slot] = ck.legi[src_slot];
  if (st.ext) {
    double2 *ext = reinterpret_cast<double2 *>(st.ext);
    if (ck.live & CK_LIVE_EXT) restore_planes<ExtFields::COUNT / 2>(ext, ck.ext, ns, dst_slot, src_slot, [](int k) { return k; });
    else
      for (int p = 0; p < ExtFields::COUNT / 2; ++p) ext[int64_t(p) * ns + dst_slot] = double2{0.0, 0.0};
  }

  // ---- robot tile (rob_index layout: [wavefront][field][rpw]): lane `leg` of the group moves fields leg, leg + L, ...
  constexpr RobotCopyMask mask = robot_copy_mask();
  constexpr int per_lane = (R::COUNT + L - 1) / L;
  const double *rs = ck.robd + sw * (R::COUNT * rpw) + sgi;
  double *rd = st.robd + w * (R::COUNT * rpw) + gi;
  double rv[per_lane];
#pragma unroll
  for (int k = 0; k < per_lane; ++k) {
    const int f = leg + k * L;
    const bool moves = f < R::COUNT && ((mask.w[(f >> 6) & 1] >> (f & 63)) & 1);
    rv[k] = moves ? rs[f * rpw] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < per_lane; ++k) {
    const int f = leg + k * L;
    const bool moves = f < R::COUNT && ((mask.w[(f >> 6) & 1] >> (f & 63)) & 1);
    if (moves) rd[f * rpw] = rv[k];
  }
  for (int f = leg; f < R::I_COUNT; f += L) st.robi[(w * R::I_COUNT + f) * rpw + gi] = ck.robi[(sw * R::I_COUNT + f) * rpw + sgi];

  // ---- lazily allocated per-robot records: a record the checkpoint does not hold is cleared (as aux_state_kernel does for a blob without the flag)
  if (st.manual)
    restore_words<L>(reinterpret_cast<int32_t *>(st.manual + rob), (ck.live & CK_LIVE_MANUAL) ? reinterpret_cast<const int32_t *>(ck.manual + src) : nullptr,
                     int(sizeof(ManualRobot) / 4), leg);
  if (seq)
    restore_words<L>(reinterpret_cast<int32_t *>(seq + rob), (ck.live & CK_LIVE_SEQ) ? reinterpret_cast<const int32_t *>(ck.seq + src) : nullptr,
                     int(sizeof(SeqRobotState) / 4), leg);
}
static_assert(sizeof(ManualRobot) % 4 == 0 && sizeof(SeqRobotState) % 4 == 0, "the per-robot records are copied as 4-byte words");

} // namespace shc

// ---- host side (included by shc_engine.hip below shc_snapshot.hpp)
extern "C" int shc_debug_checkpoint_field_class(int nj, int is_robot, int field) {
  if (field < 0) return -1;
  if (is_robot) return field < RobotFields::COUNT ? ck_field_class<RobotFieldClasses>(field) : -1;
  if (nj < 3 || nj > 5) return -1;
  return dispatch_nj(nj, [&](auto j) { return field < Fields<decltype(j)::value>::COUNT ? ck_field_class<LegFieldClasses<decltype(j)::value>>(field) : -1; });
}

// A checkpoint belongs to the engine that made it and sits in that engine's registry (shc_engine::checkpoints).  shc_engine_destroy releases
// the device arrays of every registered checkpoint and leaves the handles behind as orphans (engine == nullptr): an orphan answers every use
// with SHC_ERR_INVALID_ARG, and shc_checkpoint_destroy frees what is left of it - no call ever follows a pointer into a destroyed engine.
struct shc_checkpoint {
  shc_engine *engine;
  shc_checkpoint *next;
  double *legd;
  int32_t *legi;
  double *robd;
  int32_t *robi;
  double *ext;
  ManualRobot *manual;
  SeqRobotState *seq;
  int64_t bytes;       // device bytes held
  uint32_t rt_flags;   // the engine's RT_* facts at capture time
  uint32_t live;       // CK_LIVE_* at capture time
  uint64_t generation; // adjust_generation at capture time
};

static size_t ck_legd_bytes(const shc_engine *e) { return size_t(e->n_leg_fields) * e->n_slots * 8; }
static size_t ck_legi_bytes(const shc_engine *e) { return size_t(e->n_slots) * 4; }
static size_t ck_robd_bytes(const shc_engine *e) { return size_t(RobotFields::COUNT) * e->n_rob_pad * 8; }
static size_t ck_robi_bytes(const shc_engine *e) { return size_t(RobotFields::I_COUNT) * e->n_rob_pad * 4; }
static size_t ck_ext_bytes(const shc_engine *e) { return size_t(ExtFields::COUNT) * e->n_slots * 8; }
static size_t ck_manual_bytes(const shc_engine *e) { return sizeof(ManualRobot) * size_t(e->n_rob_pad); }
static size_t ck_seq_bytes(const shc_engine *e) { return sizeof(SeqRobotState) * size_t(e->n); }

static void checkpoint_free_arrays(shc_checkpoint *ck) {
  (void)hipFree(ck->legd);
  (void)hipFree(ck->legi);
  (void)hipFree(ck->robd);
  (void)hipFree(ck->robi);
  (void)hipFree(ck->ext);
  (void)hipFree(ck->manual);
  (void)hipFree(ck->seq);
  ck->legd = ck->robd = ck->ext = nullptr;
  ck->legi = ck->robi = nullptr;
  ck->manual = nullptr;
  ck->seq = nullptr;
  ck->bytes = 0;
}
static void release_checkpoints(shc_engine *e) { // shc_engine_destroy, after the engine's streams have drained
  for (shc_checkpoint *ck = e->checkpoints; ck;) {
    shc_checkpoint *next = ck->next;
    checkpoint_free_arrays(ck);
    ck->engine = nullptr, ck->next = nullptr;
    ck = next;
  }
  e->checkpoints = nullptr;
}
template <class T>
static int checkpoint_alloc(shc_checkpoint *ck, T **p, size_t bytes) {
  if (*p) return SHC_OK;
  HIP_TRY(hipMalloc(p, bytes));
  ck->bytes += int64_t(bytes);
  return SHC_OK;
}
// Device-to-device copies of the whole arrays on the engine's stream; the only allocation is for a record array the engine has grown since
// the checkpoint last saw it.  Neither waits for the device.
static int checkpoint_capture(shc_engine *e, shc_checkpoint *ck) {
  HIP_TRY(hipSetDevice(e->device));
  int rc = SHC_OK;
  if (e->st.ext && (rc = checkpoint_alloc(ck, &ck->ext, ck_ext_bytes(e))) != SHC_OK) return rc;
  if (e->st.manual && (rc = checkpoint_alloc(ck, &ck->manual, ck_manual_bytes(e))) != SHC_OK) return rc;
  if (e->d_seq && (rc = checkpoint_alloc(ck, &ck->seq, ck_seq_bytes(e))) != SHC_OK) return rc;
  HIP_TRY(hipMemcpyAsync(ck->legd, e->st.legd, ck_legd_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(ck->legi, e->st.legi, ck_legi_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(ck->robd, e->st.robd, ck_robd_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(ck->robi, e->st.robi, ck_robi_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  if (e->st.ext) HIP_TRY(hipMemcpyAsync(ck->ext, e->st.ext, ck_ext_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  if (e->st.manual) HIP_TRY(hipMemcpyAsync(ck->manual, e->st.manual, ck_manual_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  if (e->d_seq) HIP_TRY(hipMemcpyAsync(ck->seq, e->d_seq, ck_seq_bytes(e), hipMemcpyDeviceToDevice, e->stream));
  ck->rt_flags = e->rt_flags;
  ck->live = aux_live_flags(e);
  ck->generation = adjust_generation(e);
  return SHC_OK;
}

extern "C" int shc_engine_checkpoint_create(shc_engine *e, shc_checkpoint **out) {
  if (!out) return fail(SHC_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  SHC_ENTER_JOINED(e);
  HIP_TRY(hipSetDevice(e->device));
  shc_checkpoint *ck = new shc_checkpoint();
  int rc = checkpoint_alloc(ck, &ck->legd, ck_legd_bytes(e));
  if (rc == SHC_OK) rc = checkpoint_alloc(ck, &ck->legi, ck_legi_bytes(e));
  if (rc == SHC_OK) rc = checkpoint_alloc(ck, &ck->robd, ck_robd_bytes(e));
  if (rc == SHC_OK) rc = checkpoint_alloc(ck, &ck->robi, ck_robi_bytes(e));
  if (rc == SHC_OK) rc = checkpoint_capture(e, ck);
  if (rc != SHC_OK) {
    checkpoint_free_arrays(ck);
    delete ck;
    return rc;
  }
  ck->engine = e;
  ck->next = e->checkpoints;
  e->checkpoints = ck;
  *out = ck;
  return SHC_OK;
}
static int checkpoint_of(const shc_engine *e, const shc_checkpoint *ck) {
  if (!ck) return fail(SHC_ERR_INVALID_ARG, "checkpoint is NULL");
  if (!ck->engine) return fail(SHC_ERR_INVALID_ARG, "the checkpoint's engine has been destroyed");
  if (ck->engine != e) return fail(SHC_ERR_INVALID_ARG, "the checkpoint belongs to another engine");
  return SHC_OK;
}
extern "C" int shc_engine_checkpoint_update(shc_engine *e, shc_checkpoint *ck) {
  SHC_ENTER_JOINED(e);
  const int rc = checkpoint_of(e, ck);
  return rc == SHC_OK ? checkpoint_capture(e, ck) : rc;
}
extern "C" int shc_checkpoint_destroy(shc_checkpoint *ck) {
  if (!ck) return fail(SHC_ERR_INVALID_ARG, "checkpoint is NULL");
  if (shc_engine *e = ck->engine) { // (an orphan holds nothing on the device any more)
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream); // a capture or a restore may still be reading / writing the arrays
    for (shc_checkpoint **p = &e->checkpoints; *p; p = &(*p)->next)
      if (*p == ck) {
        *p = ck->next;
        break;
      }
    checkpoint_free_arrays(ck);
  }
  delete ck;
  return SHC_OK;
}
extern "C" int64_t shc_checkpoint_bytes(const shc_checkpoint *ck) { return ck ? ck->bytes : 0; }

extern "C" int shc_engine_restore_instances(shc_engine *e, const shc_checkpoint *ck, const int64_t *source, int on_device) {
  SHC_ENTER_JOINED(e);
  int rc = checkpoint_of(e, ck);
  if (rc != SHC_OK) return rc;
  // Phases count in the step cycle of capture time, and the parameters a restored state was produced under are not part of it
  if (adjust_pending(e)) return fail(SHC_ERR_UNSUPPORTED, "a shc_engine_adjust_parameter waits for its loop: step once, then shc_engine_checkpoint_update");
  if (ck->generation != adjust_generation(e))
    return fail(SHC_ERR_UNSUPPORTED, "the gait or a parameter has changed since the checkpoint was captured: shc_engine_checkpoint_update");
  bool whole = source == nullptr; // every instance is restored (known for a host map only)
  if (source && !on_device) {
    whole = true;
    for (int64_t i = 0; i < e->n; ++i) {
      if (source[i] >= e->n) return fail(SHC_ERR_INVALID_ARG, "source entry >= n");
      whole = whole && source[i] >= 0;
    }
  }
  HIP_TRY(hipSetDevice(e->device));
  // ---- the engine-wide facts, by the rules state_transfer and aux_state apply to injected records; the values are the checkpoint's, captured on the host
  if ((ck->live & CK_LIVE_MANUAL) && !e->st.manual && (rc = ensure_manual(e)) != SHC_OK) return rc; // (cannot happen on the same engine: records are never freed)
  if ((ck->live & CK_LIVE_SEQ) && !e->d_seq && (rc = ensure_seq(e)) != SHC_OK) return rc;
  if ((ck->rt_flags & RT_EFFORT_LIVE) && (rc = effort_live(e)) != SHC_OK) return rc; // (already on: the flag is never taken back)
  e->rt_flags |= RT_MANUAL_LIVE | (ck->rt_flags & RT_TOUCHDOWN);
  if (ck->live & CK_LIVE_MANUAL) e->rt_flags |= RT_MANUAL_LEGS | RT_MANUAL_LIVE;
  if (ck->live & CK_LIVE_EXT) e->rt_flags |= RT_EXTERNAL;
  const bool tips = (ck->live & CK_LIVE_POSER_TIPS) != 0; // as aux_state: only a restore of the whole batch can raise it
  e->plan_poser_tips_current = whole ? tips : (e->plan_poser_tips_current && tips);
  HostCall hc(e);
  const int64_t *d_source = hc.in(source, size_t(e->n), on_device);
  if ((rc = hc.status()) != SHC_OK) return rc;
  const CheckpointView view{reinterpret_cast<const double2 *>(ck->legd), ck->legi, ck->robd, ck->robi, reinterpret_cast<const double2 *>(ck->ext), ck->manual, ck->seq, ck->live};
  rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    restore_instances_kernel<L, NJ><<<dim3((unsigned)e->n_waves), dim3(64), 0, e->stream>>>(e->st, e->d_seq, view, d_source);
    return SHC_OK;
  });
  return rc != SHC_OK ? rc : hc.finish();
}
