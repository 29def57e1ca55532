// shc_resident_rows.hpp — resident tensors: the two dense-tensor ends of the resident loop.  shc_engine_resident_post_actions posts the inputs of
// the next cycle from one dense [n][A] array of float64 or float32 - what a policy emits per tick -, shc_engine_resident_get_observations_async
// hands q / qd / model_tip = FK(q) of a cycle back as one dense [n][D] array, stream-ordered.  Included by shc_engine.hip behind shc_resident.hpp
// and the row passes (uses the host route of a post, the read wait and the post kernel's device pieces of shc_resident.hpp, the specs and checks
// of shc_actions.hpp / shc_observe.hpp / shc_rollout.hpp, the group table of shc_inputs.hpp and the joints launch of shc_rollout.hpp).
//
// Neither end touches a cycle kernel, a loop kernel or the relay.
//   POST   one launch reads the caller's tensor with consecutive lanes on consecutive elements and stores every element, converted, straight into
//          the loop's input rings (rin, force, effort) with the ordinary post kernel's write-through stores; thread 0 writes the cycle's header
//          and, with publish, the last block rings the doorbell - resident_post_kernel's own pieces.  Nothing is staged.  A column table in the
//          kernel arguments says where a column goes; the host builds it per call (at most 88 entries) with the ring positions folded in.
//   READ   a slot of the loop's output ring has the layout of a slot of the K-cycle launches' ring (NJ planes of n_slots double2): the read kernel
//          is rollout_joints_kernel, one cycle, behind resident_wait_done_kernel on the engine's stream.
// Every kernel launched while a loop is alive must find room beside a loop that fills the chip: the post kernel has no LDS, no scratch and a
// handful of registers (DESIGN §4.6g has the figures); the read kernel's LDS tile fits the compute unit per XCD the loop leaves free.
#pragma once

// ---- device side
// Where a column of the caller's row goes: bits 0-2 kind, 3-7 field, 8-10 leg, 11-18 ring position of the column's group
enum : uint32_t {
  RROW_IGNORED = 0, // a leg or a joint the morphology lacks
  RROW_ROBOT = 1,   // rin record `field` (RIN_*) of the robot
  RROW_QUAT = 2,    // ... RIN_IMU + `field` of the quaternion normalised in double: the lane re-reads the four columns from `imuq_col`
  RROW_FORCE = 3,   // plane `field` (0 .. 2) of the force ring at the slot of (robot, leg)
  RROW_EFFORT = 4,  // plane `field` (joint) of the effort ring
};
constexpr int kResidentRowColumns = 16 + SHC_MAX_LEGS * 3 + SHC_MAX_LEGS * SHC_MAX_JOINTS; // every field in the largest row geometry
constexpr uint32_t resident_row_entry(uint32_t kind, int field, int leg, int pos) { return kind | uint32_t(field) << 3 | uint32_t(leg) << 8 | uint32_t(pos) << 11; }

struct ResidentRowsArgs : ResidentPostSlot {
  int64_t elements;   // n x width: one thread each
  int64_t row_stride; // elements between the rows of the caller's array
  int64_t n_slots;
  int32_t width, imuq_col;
  int32_t L, rpw, nje; // legs, robots per wavefront, joint planes of the effort ring (NJ rounded up to even)
  int32_t n_waves;
  uint32_t col[kResidentRowColumns];
};

// Thread t takes element (robot t / width, column t mod width): a wavefront reads 64 consecutive elements of a dense array (two runs at most per
// row seam of a wider one) and each lane stores its own element where the loop reads it - L and NJ are run-time values, as in resident_post_kernel:
// one instance per element type.  No LDS (a loop that fills the chip leaves none), no cross-lane exchange: the four lanes of a robot's quaternion
// each read all four columns and compute the same norm.
template <class T>
__global__ __launch_bounds__(64) void resident_post_rows_kernel(const T *__restrict__ in, const ResidentRowsArgs a, ResidentHeader *headers, double *rin, double *force,
                                                                double *effort) {
  const int64_t t = int64_t(blockIdx.x) * 64 + threadIdx.x;
  if (t < a.elements) {
    const int64_t rob = t / a.width;
    const int c = int(t - rob * a.width);
    const uint32_t entry = a.col[c];
    const uint32_t kind = entry & 7u;
    const int field = int(entry >> 3 & 31u), leg = int(entry >> 8 & 7u);
    const int64_t pos = entry >> 11 & 255u;
    if (kind != RROW_IGNORED) {
      const T *row = in + rob * a.row_stride;
      double v = static_cast<double>(row[c]);
      if (kind == RROW_ROBOT || kind == RROW_QUAT) {
        int rfield = field;
        if (kind == RROW_QUAT) { // Model::setImuData input as shc_engine_set_imu stores it: the orientation normalised (as resident_post_kernel)
          const T *s = row + a.imuq_col;
          const Quat qn = normalized(Quat{static_cast<double>(s[0]), static_cast<double>(s[1]), static_cast<double>(s[2]), static_cast<double>(s[3])});
          v = field == 0 ? qn.w : field == 1 ? qn.x : field == 2 ? qn.y : qn.z;
          rfield = RIN_IMU + field;
        }
        const int64_t w = rob / a.rpw;
        const int r = int(rob - w * a.rpw);
        resident_put(rin + ((pos * a.n_waves + w) * RIN_COUNT + rfield) * a.rpw + r, v);
      } else {
        const int64_t slot = slot_of(rob, leg, a.L);
        double *base = kind == RROW_FORCE ? force + pos * 2 * a.n_slots * 2 : effort + pos * (a.nje / 2) * a.n_slots * 2;
        resident_put(base + leg_field_index(field, slot, a.n_slots), v);
      }
    }
  }
  if (t == 0) resident_post_header(a, headers);
  resident_post_doorbell(a);
}

// ---- host side
// The column table of a resolved spec for an engine, the ring positions already in `a` (resident_post_place) folded in
static void resident_rows_columns(const shc_engine *e, const shc_act_spec *spec, const RowLayout &lay, ResidentRowsArgs &a) {
  for (int g = 0; g < kInputGroups; ++g) {
    if (!(lay.mask >> g & 1u)) continue;
    const int pos = a.pos[input_group(g).rg], first = lay.col[g];
    if (!input_per_leg(g)) {
      // (the record of a robot group: v(2) w(1) | quat(4) gyro(3) | tvi(3) rvi(3), the components of a group one behind the other)
      if (g == SHC_ACT_IMU_ORIENTATION) { // (RIN_IMU + 0 .. 3, through the normalisation)
        for (int k = 0; k < 4; ++k) a.col[first + k] = resident_row_entry(RROW_QUAT, k, 0, pos);
        a.imuq_col = first;
        continue;
      }
      const int rin0 = g == SHC_ACT_LINEAR_XY ? RIN_VEL : g == SHC_ACT_ANGULAR ? RIN_VEL + 2 : g == SHC_ACT_IMU_ANGULAR_VELOCITY ? RIN_IMU + 4
                       : g == SHC_ACT_POSE_TRANSLATION_VELOCITY ? RIN_POSE : RIN_POSE + 3;
      for (int k = 0; k < input_group(g).width; ++k) a.col[first + k] = resident_row_entry(RROW_ROBOT, rin0 + k, 0, pos);
      continue;
    }
    // per leg, leg-major: all NJ entries of every leg the robot has (a shorter leg's surplus joints hold what the caller put there, as the ordinary post)
    const int per_leg = input_k(g, spec->dof), live = g == SHC_ACT_TIP_FORCE ? 3 : e->NJ;
    for (int leg = 0; leg < e->L; ++leg)
      for (int k = 0; k < live; ++k) a.col[first + leg * per_leg + k] = resident_row_entry(g == SHC_ACT_TIP_FORCE ? RROW_FORCE : RROW_EFFORT, k, leg, pos);
  }
}

extern "C" int shc_engine_resident_post_actions(shc_engine *e, const shc_act_spec *spec, const void *actions, int publish, int64_t *cycle) {
  int rc = resident_require(e, true);
  if (rc != SHC_OK) return rc;
  Resident *r = e->res;
  if ((rc = resident_alive(r)) != SHC_OK) return rc;
  if (!spec || !actions) return fail(SHC_ERR_INVALID_ARG, "spec or actions is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ActRows>(spec, lay)) return bad;
  if ((rc = actions_check(e, spec)) != SHC_OK) return rc;
  if ((rc = input_pairs_check(lay.mask, kAllInputs, "posted")) != SHC_OK) return rc;
  if ((rc = row_aligned(actions, spec->dtype, "actions")) != SHC_OK) return rc;
  // The post kernel follows the engine's stream (where the tensor is ready).  A stream-ordered read parks that stream until its cycle has run:
  // behind a read of a cycle nobody has released, this post - and whatever would release the cycle behind it - would wait for the read to give up.
  if (r->read_queued >= 0 && (unsigned long long)r->read_queued >= r->published)
    return fail(SHC_ERR_INVALID_ARG, "resident mode: a stream-ordered read of an unpublished cycle is pending: publish or post first");
  const unsigned mask = input_resident_groups(lay.mask);
  unsigned long long c = 0;
  if ((rc = resident_post_admit(e, mask, c)) != SHC_OK) return rc;
  ResidentRowsArgs a{};
  if ((rc = resident_post_place(r, mask, c, a)) != SHC_OK) return rc;
  if (publish != 0 && (rc = resident_post_release(r, a)) != SHC_OK) return rc;
  a.width = int32_t(lay.width);
  a.elements = e->n * lay.width;
  a.row_stride = row_stride_of(spec, lay);
  a.n_slots = e->n_slots;
  a.L = e->L, a.rpw = 64 / e->L, a.nje = (e->NJ + 1) & ~1;
  a.n_waves = int32_t(e->n_waves);
  resident_rows_columns(e, spec, lay, a);
  const dim3 grid((unsigned)((a.elements + 63) / 64));
  HIP_TRY(hipEventRecord(r->rows_ev[0], e->stream)); // the tensor is ready on the engine's stream ...
  HIP_TRY(hipStreamWaitEvent(r->in_stream, r->rows_ev[0], 0));
  if (spec->dtype == SHC_OBS_F32)
    resident_post_rows_kernel<float><<<grid, dim3(64), 0, r->in_stream>>>(static_cast<const float *>(actions), a, r->headers, r->rin, r->force, r->effort);
  else
    resident_post_rows_kernel<double><<<grid, dim3(64), 0, r->in_stream>>>(static_cast<const double *>(actions), a, r->headers, r->rin, r->force, r->effort);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(r->rows_ev[1], r->in_stream)); // ... and free again for what that stream is given behind this call
  HIP_TRY(hipStreamWaitEvent(e->stream, r->rows_ev[1], 0));
  resident_post_commit(r, a, cycle);
  return SHC_OK;
}

extern "C" int shc_engine_resident_get_observations_async(shc_engine *e, int64_t cycle, const shc_obs_spec *spec, void *out, int timeout_ms) {
  int rc = resident_require(e, true);
  if (rc != SHC_OK) return rc;
  Resident *r = e->res;
  if ((rc = resident_alive(r)) != SHC_OK) return rc;
  if (!spec || !out) return fail(SHC_ERR_INVALID_ARG, "spec or out is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ObsRows>(spec, lay)) return bad;
  if ((rc = rollout_joints_check(e, spec, lay, kRingKinematics)) != SHC_OK) return rc;
  if ((rc = row_aligned(out, spec->dtype, "out")) != SHC_OK) return rc;
  if ((rc = resident_read_wait(e, cycle, timeout_ms)) != SHC_OK) return rc;
  const double2 *slot = reinterpret_cast<const double2 *>(r->out) + int64_t(cycle % r->depth) * e->NJ * e->n_slots;
  const int64_t stride = row_stride_of(spec, lay);
  return rollout_joints_launch_at(e, spec, lay, out, stride, e->n * stride, nullptr, slot, 1);
}
