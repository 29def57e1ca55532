// shc_actions.hpp — the action pass: chosen input groups of every instance taken from one dense [n][A] array of float64 or float32 in one device
// pass: shc_act_width, shc_act_column, shc_engine_set_actions.  Included by shc_engine.hip beside shc_observe.hpp, whose pass it turns round (uses
// rob_index, leg_field_index, the split-input calls, effort_live and touchdown_detection_kernel of the setters, and the entry-point macros).  The
// fleet form (shc_fleet_actions.hpp) launches the same kernel with a part's caller ids as the row table.
//
// The definition is the device setters': the pass leaves what shc_engine_set_velocity / _set_imu / _set_pose_input / _set_tip_force /
// _set_joint_effort leave when they are given the columns as float64 arrays.  Nothing is computed here but the conversion to double and the
// normalisation of the IMU quaternion, by the normalized() scatter_rob_kernel calls; every host-side effect is the setters' own code path
// (effort_live, the flags, touchdown_detection_kernel).  The field list is launch-uniform: a bit per selected field and the field's first column.
#pragma once

constexpr int kActFields = SHC_ACT_FIELD_COUNT;
constexpr int kActRobotFields = SHC_ACT_TIP_FORCE; // the per-robot fields come first in the enum
static_assert(sizeof(shc_act_spec) == 64 && offsetof(shc_act_spec, row_stride) == 56, "shc_act_spec: 13 int32, 4 bytes of alignment, row_stride");
static_assert(kActRobotFields == 6 && SHC_ACT_JOINT_EFFORT == 7 && kActFields == 8, "six per-robot fields, then tip force and joint effort");

// columns of a per-robot field, and the robot field its first component is stored at
__host__ __device__ constexpr int act_robot_width(int field) {
  return field == SHC_ACT_LINEAR_XY ? 2 : field == SHC_ACT_ANGULAR ? 1 : field == SHC_ACT_IMU_ORIENTATION ? 4 : 3;
}
__host__ __device__ constexpr int act_robot_field(int field) {
  using R = RobotFields;
  return field == SHC_ACT_LINEAR_XY                   ? R::VIN
         : field == SHC_ACT_ANGULAR                   ? R::WIN
         : field == SHC_ACT_IMU_ORIENTATION           ? R::IMUQ
         : field == SHC_ACT_IMU_ANGULAR_VELOCITY      ? R::GYRO
         : field == SHC_ACT_POSE_TRANSLATION_VELOCITY ? R::TVI
                                                      : R::RVI;
}
static bool act_per_leg(int field) { return field >= kActRobotFields; }
// columns per leg (per-leg fields) or per robot
static int act_field_width(int field, int dof) { return field == SHC_ACT_JOINT_EFFORT ? dof : field == SHC_ACT_TIP_FORCE ? 3 : act_robot_width(field); }

// A spec resolved: the first column of every field (-1: not selected), the selected fields as a mask, the columns of a row.
struct ActLayout {
  int32_t col[kActFields];
  uint32_t mask;
  int64_t width;
};
// nullptr when the spec is valid on its own (no engine asked yet), else what is wrong with it
static const char *act_layout(const shc_act_spec *s, ActLayout &lay) {
  if (!s) return "spec is NULL";
  if (s->n_fields < 1 || s->n_fields > kActFields) return "shc_act_spec.n_fields outside 1 .. SHC_ACT_FIELD_COUNT";
  if (s->dtype != SHC_OBS_F64 && s->dtype != SHC_OBS_F32) return "shc_act_spec.dtype is neither SHC_OBS_F64 nor SHC_OBS_F32";
  if (s->reserved != 0) return "shc_act_spec.reserved must be 0";
  if (s->legs < 1 || s->legs > SHC_MAX_LEGS || s->dof < 1 || s->dof > SHC_MAX_JOINTS) return "shc_act_spec.legs / dof outside 1 .. SHC_MAX_LEGS / SHC_MAX_JOINTS";
  for (int f = 0; f < kActFields; ++f) lay.col[f] = -1;
  lay.mask = 0, lay.width = 0;
  for (int i = 0; i < s->n_fields; ++i) {
    const int f = s->fields[i];
    if (f < 0 || f >= kActFields) return "shc_act_spec.fields names an unknown field";
    if (lay.mask & (1u << f)) return "shc_act_spec.fields names a field twice";
    lay.mask |= 1u << f;
    lay.col[f] = int32_t(lay.width);
    lay.width += act_field_width(f, s->dof) * (act_per_leg(f) ? s->legs : 1);
  }
  if (s->row_stride != 0 && s->row_stride < lay.width) return "shc_act_spec.row_stride is below the width of a row";
  return nullptr;
}

extern "C" int64_t shc_act_width(const shc_act_spec *spec) {
  ActLayout lay;
  const char *why = act_layout(spec, lay);
  if (why) return -int64_t(fail(SHC_ERR_INVALID_ARG, why));
  return lay.width;
}
extern "C" int shc_act_column(const shc_act_spec *spec, int field, int leg, int k) {
  ActLayout lay;
  if (act_layout(spec, lay) || field < 0 || field >= kActFields || lay.col[field] < 0) return -1;
  const int w = act_field_width(field, spec->dof);
  if (k < 0 || k >= w) return -1;
  if (!act_per_leg(field)) return lay.col[field] + k;
  if (leg < 0 || leg >= spec->legs) return -1;
  return lay.col[field] + leg * w + k;
}

// The kernel's view of a spec (launch-uniform: scalar loads of the kernel arguments)
struct ActArgs {
  uint32_t mask;
  int32_t col[kActFields];
  int32_t dof;          // columns per leg of the joint efforts
  int32_t width, pitch; // columns of a row; elements between the rows of the LDS tile
  int64_t row_stride;
};

// observe_kernel turned round.  One leg per lane, floor(64 / L) robots per wavefront, one wavefront per workgroup: block b serves the robot
// group first / rpw + b, clipped to [first, end).  Rows come from in[row * row_stride]: row = ids[robot] (the caller's instance id of a fleet
// part's robot) or the robot's own index.
//
// Copy-in.  A robot's row is contiguous in `in`, but its columns belong to different lanes (leg l of a per-leg field at l * width + k).  The
// wavefront therefore first copies its rows into LDS - `tile`, rpw rows of `pitch` elements of T - with consecutive lanes on consecutive
// elements of a row: the lanes run through the rows one after the other, so a 64-lane load covers 64 consecutive elements of one row or the end
// of one and the start of the next (two contiguous runs), and the LDS stores (ds_write_b32 / _b64) hit consecutive banks - conflict-free but for
// the seam between two rows.  All `width` columns are copied, those of legs or joints the morphology lacks included: they stay in the tile.
// Scatter.  Lane (robot, leg) reads its own columns back (ds_read_b32 / _b64): within a robot the lanes are 3 or dof elements apart, robots
// `pitch` elements; pitch is odd, so the robots of a lane group start on distinct banks and the reads meet 2-way at most for 4-byte elements,
// 2- to 4-way for 8-byte ones (a read replays once per extra address: a handful of LDS cycles against the 3 + NJ plane stores that follow).  The
// values go to the leg planes at the lane's slot - consecutive lanes on consecutive slots, as the cycle kernels read them.
// The per-robot fields are six groups (velocity 2 + 1, IMU 4 + 3, pose 3 + 3): group g is served by the robot's lane g mod L, so a hexapod's
// six lanes take one group each; the quaternion is one lane's, which normalises it.  Their stores go to rob_index: consecutive robots on
// consecutive elements.
// The tile is at most 21 rows x 89 x 8 B = 15 KiB (3 legs, every field, 8 x 6 row geometry); a hexapod's 46-column float32 row 10 x 47 x 4 B.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void actions_kernel(const T *__restrict__ in, DevState st, const ActArgs a, const int64_t *__restrict__ ids, int64_t first, int64_t end) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  extern __shared__ double2 act_tile[];
  T *tile = reinterpret_cast<T *>(act_tile);
  const int lane = threadIdx.x;
  const int64_t w = first / rpw + blockIdx.x;
  const int gi = lane / L, leg = lane - gi * L;
  const int64_t rob = w * rpw + gi;
  const bool live = gi < rpw && rob >= first && rob < end;
  // groups [g0, g0 + n_rob) hold the rows of robots rob_lo .. of this block
  const int64_t rob_lo = w * rpw > first ? w * rpw : first, rob_hi = (w + 1) * rpw < end ? (w + 1) * rpw : end;
  const int g0 = int(rob_lo - w * rpw), n_rob = int(rob_hi - rob_lo);

  // copy-in: element e = lane, lane + 64, .. of the block's n_rob x width elements; (r, c) follow by addition - 64 = dq * width + dr
  const int total = n_rob * a.width, dq = 64 / a.width, dr = 64 - dq * a.width;
  int r = lane / a.width, c = lane - r * a.width;
  for (int e = lane; e < total; e += 64) {
    const int64_t rr = rob_lo + r;
    const int64_t irow = ids ? ids[rr] : rr;
    tile[(g0 + r) * a.pitch + c] = in[irow * a.row_stride + c];
    r += dq, c += dr;
    if (c >= a.width) c -= a.width, ++r;
  }
  __syncthreads();
  if (!live) return;

  const T *row = tile + gi * a.pitch;
  auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
  const int64_t slot = w * 64 + lane;
  if (sel(SHC_ACT_TIP_FORCE)) {
    const T *s = row + a.col[SHC_ACT_TIP_FORCE] + leg * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) st.legd[leg_field_index(FD::FORCE_IN + k, slot, st.n_slots)] = static_cast<double>(s[k]);
  }
  if (sel(SHC_ACT_JOINT_EFFORT)) { // all NJ entries of every leg, as scatter_leg_kernel: a shorter leg's surplus joints hold what the caller put there
    const T *s = row + a.col[SHC_ACT_JOINT_EFFORT] + leg * a.dof;
#pragma unroll
    for (int j = 0; j < NJ; ++j) st.legd[leg_field_index(FD::EFFORT_IN + j, slot, st.n_slots)] = static_cast<double>(s[j]);
  }
  if (a.mask & ((1u << kActRobotFields) - 1u)) {
#pragma unroll
    for (int g = 0; g < kActRobotFields; ++g) {
      if (g % L != leg || !sel(g)) continue;
      const T *s = row + a.col[g];
      if (g == SHC_ACT_IMU_ORIENTATION) { // Model::setImuData normalises the orientation (model.h:150): the call scatter_rob_kernel makes, on the converted values
        const Quat q = normalized(Quat{static_cast<double>(s[0]), static_cast<double>(s[1]), static_cast<double>(s[2]), static_cast<double>(s[3])});
        st.robd[rob_index(rob, R::IMUQ + 0, rpw, R::COUNT)] = q.w;
        st.robd[rob_index(rob, R::IMUQ + 1, rpw, R::COUNT)] = q.x;
        st.robd[rob_index(rob, R::IMUQ + 2, rpw, R::COUNT)] = q.y;
        st.robd[rob_index(rob, R::IMUQ + 3, rpw, R::COUNT)] = q.z;
      } else {
#pragma unroll
        for (int k = 0; k < act_robot_width(g); ++k) st.robd[rob_index(rob, act_robot_field(g) + k, rpw, R::COUNT)] = static_cast<double>(s[k]);
      }
    }
  }
}

// What an engine refuses of a spec that is valid on its own
static int actions_check(const shc_engine *e, const shc_act_spec *spec) {
  if (spec->legs < e->L || spec->dof < e->NJ) return fail(SHC_ERR_INVALID_ARG, "shc_act_spec.legs / dof are below the engine's legs / longest leg's DOF");
  return SHC_OK;
}
static size_t act_element_bytes(const shc_act_spec *spec) { return spec->dtype == SHC_OBS_F32 ? 4 : 8; }
// Every group of the spec could ride the half streams of split steps, as its own setter decides it
static bool actions_ride(const shc_engine *e, const ActLayout &lay, int on_device) {
  if ((lay.mask & (1u << SHC_ACT_TIP_FORCE)) && e->params.rough_terrain_mode) return false; // touchdown detection runs on the engine's stream
  if ((lay.mask & (1u << SHC_ACT_JOINT_EFFORT)) && !(e->rt_flags & RT_EFFORT_LIVE)) return false; // the parameter block is about to be re-uploaded
  return split_inputs(e, on_device);
}

// One launch: instances [r0, r1) from rows ids[instance] (ids != NULL, a device table) or instance of the device array `in`
static int actions_launch(shc_engine *e, const ActArgs &a, const void *in, int f32, const int64_t *ids, int64_t r0, int64_t r1, hipStream_t stream) {
  const int rpw = 64 / e->L;
  const unsigned grid = (unsigned)((r1 - 1) / rpw - r0 / rpw + 1);
  const size_t lds = size_t(rpw) * a.pitch * (f32 ? 4 : 8);
  return dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    if (f32)
      actions_kernel<L, NJ, float><<<dim3(grid), dim3(64), lds, stream>>>(static_cast<const float *>(in), e->st, a, ids, r0, r1);
    else
      actions_kernel<L, NJ, double><<<dim3(grid), dim3(64), lds, stream>>>(static_cast<const double *>(in), e->st, a, ids, r0, r1);
    return SHC_OK;
  });
}

// The pass over every instance of an engine, with the setters' host-side effects.  `in` is a device array ready on the engine's stream; the
// caller has checked everything and - unless `ride` (actions_ride) - joined split steps.
static int actions_apply(shc_engine *e, const shc_act_spec *spec, const ActLayout &lay, const void *in, int64_t row_stride, const int64_t *ids, bool ride) {
  HIP_TRY(hipSetDevice(e->device));
  if (lay.mask & (1u << SHC_ACT_POSE_TRANSLATION_VELOCITY | 1u << SHC_ACT_POSE_ROTATION_VELOCITY)) e->rt_flags |= RT_MANUAL_LIVE; // as shc_engine_set_pose_input
  int rc;
  if ((lay.mask & (1u << SHC_ACT_JOINT_EFFORT)) && (rc = effort_live(e)) != SHC_OK) return rc; // as shc_engine_set_joint_effort
  ActArgs a{};
  a.mask = lay.mask;
  for (int f = 0; f < kActFields; ++f) a.col[f] = lay.col[f];
  a.dof = spec->dof;
  a.width = int32_t(lay.width), a.pitch = int32_t(lay.width) | 1;
  a.row_stride = row_stride;
  const int f32 = spec->dtype == SHC_OBS_F32;
  if (ride) {
    if ((rc = split_inputs_begin(e)) != SHC_OK) return rc;
    const int64_t mid = split_first_instance_of_second_half(e);
    if (mid > 0 && (rc = actions_launch(e, a, in, f32, ids, 0, mid, e->half_stream[0])) != SHC_OK) return rc;
    if (e->n > mid && (rc = actions_launch(e, a, in, f32, ids, mid, e->n, e->half_stream[1])) != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    if ((rc = split_inputs_end(e)) != SHC_OK) return rc;
  } else {
    if ((rc = actions_launch(e, a, in, f32, ids, 0, e->n, e->stream)) != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
  }
  if (lay.mask & (1u << SHC_ACT_TIP_FORCE)) {
    e->rt_flags |= RT_TOUCHDOWN; // LegStepper::setTouchdownDetection(true) (state_controller.cpp:1642)
    if (e->params.rough_terrain_mode) { // Leg::touchdownDetection behind the stored forces, as shc_engine_set_tip_force (never riding: actions_ride)
      const int64_t threads = e->n * e->L;
      rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
        constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
        touchdown_detection_kernel<L, NJ><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, e->stream>>>(
            e->st, (const SharedConsts<L, NJ> *)e->d_consts, e->params.touchdown_threshold, e->params.liftoff_threshold);
        return SHC_OK;
      });
      if (rc != SHC_OK) return rc;
      HIP_TRY(hipGetLastError());
    }
  }
  return SHC_OK;
}

extern "C" int shc_engine_set_actions(shc_engine *e, const shc_act_spec *spec, const void *actions, int on_device) {
  SHC_ENTER(e);
  if (!spec || !actions) return fail(SHC_ERR_INVALID_ARG, "spec or actions is NULL");
  ActLayout lay;
  if (const char *why = act_layout(spec, lay)) return fail(SHC_ERR_INVALID_ARG, why);
  int rc = actions_check(e, spec);
  if (rc != SHC_OK) return rc;
  const size_t es = act_element_bytes(spec);
  if (reinterpret_cast<uintptr_t>(actions) & (es - 1)) return fail(SHC_ERR_INVALID_ARG, "actions must be aligned to its element size");
  const bool ride = actions_ride(e, lay, on_device);
  if (!ride && (rc = join_side(e)) != SHC_OK) return rc;
  const int64_t stride = spec->row_stride ? spec->row_stride : lay.width;
  if (on_device) return actions_apply(e, spec, lay, actions, stride, nullptr, ride);
  // host form: the columns [0, width) of every row of the caller's array as dense rows on the device, then the pass
  HIP_TRY(hipSetDevice(e->device));
  void *d = nullptr;
  const size_t row_bytes = size_t(lay.width) * es;
  HIP_TRY(hipMalloc(&d, size_t(e->n) * row_bytes));
  hipError_t err = hipMemcpy2DAsync(d, row_bytes, actions, size_t(stride) * es, row_bytes, size_t(e->n), hipMemcpyHostToDevice, e->stream);
  if (err == hipSuccess) rc = actions_apply(e, spec, lay, d, lay.width, nullptr, false);
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  (void)hipFree(d);
  if (err != hipSuccess) return fail(SHC_ERR_HIP, std::string("actions: ") + hipGetErrorString(err));
  return rc;
}
