// shc_actions.hpp — the action pass: chosen input groups of every instance taken from one dense [n][A] array of float64 or float32 in one device
// pass: shc_act_width, shc_act_column, shc_engine_set_actions.  Included by shc_engine.hip beside shc_observe.hpp (uses the row pattern of shc_rows.hpp,
// the group table of shc_inputs.hpp - a field of a spec IS an input group: its width, its robot field -, rob_index, leg_field_index, the split-input
// calls, effort_live and tip_force_given of the setters, and the entry-point macros).  The fleet form (shc_fleet_actions.hpp) launches the same
// kernel with a part's caller ids as the row table.
//
// The definition is the device setters': the pass leaves what shc_engine_set_velocity / _set_imu / _set_pose_input / _set_tip_force /
// _set_joint_effort leave when they are given the columns as float64 arrays.  Nothing is computed here but the conversion to double and the
// normalisation of the IMU quaternion, by the normalized() scatter_rob_kernel calls; every host-side effect is the setters' own code path
// (effort_live, the flags, touchdown_detection_kernel).  The field list is launch-uniform: a bit per selected field and the field's first column.
#pragma once

constexpr int kActFields = kInputGroups, kActRobotFields = kRobotInputGroups; // the fields are the input groups of shc_inputs.hpp
static_assert(sizeof(shc_act_spec) == 64 && offsetof(shc_act_spec, row_stride) == 56, "shc_act_spec: 13 int32, 4 bytes of alignment, row_stride");

// shc_act_spec for row_layout (shc_rows.hpp)
struct ActRows {
  using Spec = shc_act_spec;
  static constexpr const char *name = "shc_act_spec", *n_fields_why = ".n_fields outside 1 .. SHC_ACT_FIELD_COUNT";
  static constexpr int fields = kActFields, most_fields = kActFields;
  static constexpr bool has_dof = true;
  static bool per_leg(int field) { return input_per_leg(field); }
  static int width(int field, int dof) { return input_k(field, dof); }
  static const char *own(const Spec *) { return nullptr; }
};

extern "C" int64_t shc_act_width(const shc_act_spec *spec) { return row_width<ActRows>(spec); }
extern "C" int shc_act_column(const shc_act_spec *spec, int field, int leg, int k) { return row_column<ActRows>(spec, field, leg, k); }

// The kernel's view of a spec
struct ActArgs : RowArgs<kActFields> {
  int32_t dof; // columns per leg of the joint efforts
};

// The geometry and the tile of shc_rows.hpp, copy-in: the rows in[row * row_stride], row = ids[robot] or the robot's own index, come into the
// tile with consecutive lanes on consecutive elements; lane (robot, leg) then reads its own columns back and stores them to the leg planes at
// the lane's slot - consecutive lanes on consecutive slots, as the cycle kernels read them (a bank conflict of the read is a handful of LDS
// cycles against the 3 + NJ plane stores that follow).
// The per-robot fields are six groups (velocity 2 + 1, IMU 4 + 3, pose 3 + 3): group g is served by the robot's lane g mod L, so a hexapod's
// six lanes take one group each; the quaternion is one lane's, which normalises it.  Their stores go to rob_index: consecutive robots on
// consecutive elements.
// The tile is at most 21 rows x 89 x 8 B = 15 KiB (3 legs, every field, 8 x 6 row geometry); a hexapod's 46-column float32 row 10 x 47 x 4 B.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void actions_kernel(const T *__restrict__ in, DevState st, const ActArgs a, const int64_t *__restrict__ ids, int64_t first, int64_t end) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  const RowGroup<L> rg(first, end);
  const int gi = rg.gi, leg = rg.leg;
  const int64_t rob = rg.rob;
  T *tile = row_tile<T>();

  row_tile_in(tile, in, rg, a, ids, 0);
  __syncthreads();
  if (!rg.live) return;

  const T *row = tile + gi * a.pitch;
  auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
  const int64_t slot = rg.slot;
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
// Every group of the spec could ride the half streams of split steps, as its own setter decides it
static bool actions_ride(const shc_engine *e, const RowLayout &lay, int on_device) {
  if ((lay.mask & (1u << SHC_ACT_TIP_FORCE)) && e->params.rough_terrain_mode) return false; // touchdown detection runs on the engine's stream
  if ((lay.mask & (1u << SHC_ACT_JOINT_EFFORT)) && !(e->rt_flags & RT_EFFORT_LIVE)) return false; // the parameter block is about to be re-uploaded
  return split_inputs(e, on_device);
}

// One launch: instances [r0, r1) from rows ids[instance] (ids != NULL, a device table) or instance of the device array `in`
static int actions_launch(shc_engine *e, const ActArgs &a, const void *in, int f32, const int64_t *ids, int64_t r0, int64_t r1, hipStream_t stream) {
  const unsigned grid = row_grid(e->L, r0, r1);
  const size_t lds = row_tile_bytes(e->L, a.pitch, f32 ? SHC_OBS_F32 : SHC_OBS_F64);
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
static int actions_apply(shc_engine *e, const shc_act_spec *spec, const RowLayout &lay, const void *in, int64_t row_stride, const int64_t *ids, bool ride) {
  HIP_TRY(hipSetDevice(e->device));
  if (lay.mask & kPoseInputs) e->rt_flags |= RT_MANUAL_LIVE; // as shc_engine_set_pose_input
  int rc;
  if ((lay.mask & (1u << SHC_ACT_JOINT_EFFORT)) && (rc = effort_live(e)) != SHC_OK) return rc; // as shc_engine_set_joint_effort
  ActArgs a{};
  row_args(a, lay, spec->dtype, row_stride, false, 0.0);
  a.dof = spec->dof;
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
  // Leg::touchdownDetection behind the stored forces, as shc_engine_set_tip_force (in rough terrain mode never riding: actions_ride)
  return (lay.mask & (1u << SHC_ACT_TIP_FORCE)) ? tip_force_given(e) : SHC_OK;
}

extern "C" int shc_engine_set_actions(shc_engine *e, const shc_act_spec *spec, const void *actions, int on_device) {
  SHC_ENTER(e);
  if (!spec || !actions) return fail(SHC_ERR_INVALID_ARG, "spec or actions is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ActRows>(spec, lay)) return bad;
  int rc = actions_check(e, spec);
  if (rc != SHC_OK) return rc;
  if ((rc = row_aligned(actions, spec->dtype, "actions")) != SHC_OK) return rc;
  const bool ride = actions_ride(e, lay, on_device);
  if (!ride && (rc = join_side(e)) != SHC_OK) return rc;
  const int64_t stride = row_stride_of(spec, lay);
  if (on_device) return actions_apply(e, spec, lay, actions, stride, nullptr, ride);
  HIP_TRY(hipSetDevice(e->device));
  return rows_from_host(e, actions, e->n, lay.width, stride, spec->dtype, nullptr,
                        [&](const void *d, int64_t *) { return actions_apply(e, spec, lay, d, lay.width, nullptr, false); });
}
