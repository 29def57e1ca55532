// shc_observe.hpp — the observation pass: chosen fields of a range of instances as one dense [rows][D] array of float64 or float32 in one device
// pass: shc_obs_width, shc_obs_column, shc_engine_get_observations.  Included by shc_engine.hip (uses its rob_index, the derived-tip functions,
// leg_status_of / walk_state_of, load_leg_fields / leg_msg_progress of shc_leg_msgs.hpp, the body-frame functions of shc_frames.hpp and the
// entry-point macros).  The fleet form (shc_fleet_observe.hpp) launches the same kernel with a part's caller ids as the row table.
//
// Every value comes from the function the record getters call: nothing is computed here that is not computed there.  The field list is
// launch-uniform: the host resolves it into ObsArgs - a bit per selected field and the field's first column - which travels as a kernel argument;
// a field that is not selected costs neither loads nor arithmetic (scalar branches on the mask), FK runs only for SHC_OBS_MODEL_TIP and
// leg_msg_progress only for the three progress fields.
#pragma once

constexpr int kObsFields = SHC_OBS_FIELD_COUNT;
static_assert(kObsFields <= 32, "the selected fields are one 32-bit mask");
static_assert(sizeof(shc_obs_spec) == 4 * (1 + SHC_OBS_MAX_FIELDS + 4) + 4 + 16, "shc_obs_spec: 37 int32, 4 bytes of alignment, row_stride, pad");

// shc_obs_spec for row_layout (shc_rows.hpp)
struct ObsRows {
  using Spec = shc_obs_spec;
  static constexpr const char *name = "shc_obs_spec", *n_fields_why = ".n_fields outside 1 .. SHC_OBS_MAX_FIELDS";
  static constexpr int fields = kObsFields, most_fields = SHC_OBS_MAX_FIELDS;
  static constexpr bool has_dof = true;
  static bool per_leg(int field) { return field < SHC_OBS_BODY_POSE; }
  static int width(int field, int dof) {
    switch (field) {
      case SHC_OBS_Q: case SHC_OBS_QD: case SHC_OBS_JOINT_EFFORT: return dof;
      case SHC_OBS_WALKER_TIP: case SHC_OBS_TARGET_TIP: case SHC_OBS_POSER_TIP: case SHC_OBS_MODEL_TIP: case SHC_OBS_TIP_FORCE: case SHC_OBS_ADMITTANCE_DELTA: return 3;
      case SHC_OBS_BODY_POSE: case SHC_OBS_ODOM_TO_BASE_LINK: return 7;
      case SHC_OBS_DESIRED_VELOCITY: case SHC_OBS_POSE_EULER: return 3;
      default: return 1;
    }
  }
  static const char *own(const Spec *) { return nullptr; }
};

extern "C" int64_t shc_obs_width(const shc_obs_spec *spec) { return row_width<ObsRows>(spec); }
extern "C" int shc_obs_column(const shc_obs_spec *spec, int field, int leg, int k) { return row_column<ObsRows>(spec, field, leg, k); }

// The kernel's view of a spec
struct ObsArgs : RowArgs<kObsFields> {
  int32_t dof;                       // columns per leg of the joint fields
  int32_t derive_poser, keep_marked; // derive_tips' two facts
  int32_t have_odom;
};

// The geometry and the tile of shc_rows.hpp, copy-out: the lanes build their robots' rows in the tile (filled with `pad` first where the row has
// columns no lane owns), and the rows leave with consecutive lanes on consecutive elements, for out[row * row_stride]: row = ids[robot] or
// robot - first.  The tile is at most 21 rows x 349 x 8 B = 57 KiB (3 legs, every field, 8 x 6 row geometry); the learner-sized selection of a
// hexapod is 10 x 77 x 4 B = 3.0 KiB.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void observe_kernel(T *__restrict__ out, DevState st, const SharedConsts<L, NJ> *__restrict__ gc, const LegMsgArgs a,
                                                     const ObsArgs o, const int64_t *__restrict__ ids, int64_t first, int64_t count) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  const RowGroup<L> rg(first, first + count);
  const int gi = rg.gi, leg = rg.leg;
  const int64_t rob = rg.rob;
  T *tile = row_tile<T>();

  row_tile_pad(tile, rg, o);
  if (rg.live) {
    T *row = tile + gi * o.pitch;
    auto sel = [&](int f) { return (o.mask >> f & 1u) != 0; };
    const double2 *planes = reinterpret_cast<const double2 *>(st.legd);
    const int64_t slot = rg.slot;
    if (sel(SHC_OBS_Q) || sel(SHC_OBS_MODEL_TIP)) {
      double q[NJ]; // Joint::desired_position_
      load_leg_fields<FD::Q, NJ>(planes, st.n_slots, slot, q);
      if (sel(SHC_OBS_Q)) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) row[o.col[SHC_OBS_Q] + leg * o.dof + j] = static_cast<T>(q[j]);
      }
      if (sel(SHC_OBS_MODEL_TIP)) {
        const V3 tip = derived_model_tip<NJ>(gc->leg[leg], q);
        T *d = row + o.col[SHC_OBS_MODEL_TIP] + leg * 3;
        d[0] = static_cast<T>(tip.x), d[1] = static_cast<T>(tip.y), d[2] = static_cast<T>(tip.z);
      }
    }
    if (sel(SHC_OBS_QD)) {
      double v[NJ];
      load_leg_fields<FD::QD, NJ>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int j = 0; j < NJ; ++j) row[o.col[SHC_OBS_QD] + leg * o.dof + j] = static_cast<T>(v[j]);
    }
    if (sel(SHC_OBS_JOINT_EFFORT)) {
      double v[NJ];
      load_leg_fields<FD::EFFORT_IN, NJ>(planes, st.n_slots, slot, v); // desired_effort_ = current_effort_ (state_controller.cpp:1590)
#pragma unroll
      for (int j = 0; j < NJ; ++j) row[o.col[SHC_OBS_JOINT_EFFORT] + leg * o.dof + j] = static_cast<T>(v[j]);
    }
    auto put3 = [&](int f, const double (&v)[3]) {
      T *d = row + o.col[f] + leg * 3;
      d[0] = static_cast<T>(v[0]), d[1] = static_cast<T>(v[1]), d[2] = static_cast<T>(v[2]);
    };
    if (sel(SHC_OBS_WALKER_TIP) || sel(SHC_OBS_POSER_TIP)) {
      double tip[3];
      load_leg_fields<FD::TIP, 3>(planes, st.n_slots, slot, tip);
      if (sel(SHC_OBS_WALKER_TIP)) put3(SHC_OBS_WALKER_TIP, tip);
      if (sel(SHC_OBS_POSER_TIP)) {
        double v[3];
        if (poser_tip_is_derived(st, rob, o.derive_poser, o.keep_marked)) {
          double c[7];
#pragma unroll
          for (int k = 0; k < 7; ++k) c[k] = st.robd[rob_index(rob, R::CPOSE + k, rpw, R::COUNT)];
          const V3 pt = derived_poser_tip(c, V3{tip[0], tip[1], tip[2]});
          v[0] = pt.x, v[1] = pt.y, v[2] = pt.z;
        } else {
          load_leg_fields<FD::POSER_TIP, 3>(planes, st.n_slots, slot, v);
        }
        put3(SHC_OBS_POSER_TIP, v);
      }
    }
    if (sel(SHC_OBS_TARGET_TIP)) {
      double v[3];
      load_leg_fields<FD::TARG, 3>(planes, st.n_slots, slot, v);
      put3(SHC_OBS_TARGET_TIP, v);
    }
    if (sel(SHC_OBS_TIP_FORCE)) {
      double v[3];
      load_leg_fields<FD::TF, 3>(planes, st.n_slots, slot, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = leg_msg_tip_force(a, v[k]);
      put3(SHC_OBS_TIP_FORCE, v);
    }
    if (sel(SHC_OBS_ADMITTANCE_DELTA) || sel(SHC_OBS_VIRTUAL_STIFFNESS)) {
      double v[4] = {0.0, 0.0, 0.0, 0.0}; // (zero without admittance control, as the record)
      if (a.admittance_control) load_leg_fields<FD::ADM_DELTA, 4>(planes, st.n_slots, slot, v);
      if (sel(SHC_OBS_ADMITTANCE_DELTA)) {
        const double d[3] = {v[0], v[1], v[2]};
        put3(SHC_OBS_ADMITTANCE_DELTA, d);
      }
      if (sel(SHC_OBS_VIRTUAL_STIFFNESS)) row[o.col[SHC_OBS_VIRTUAL_STIFFNESS] + leg] = static_cast<T>(v[3]);
    }
    constexpr uint32_t kProgress = 1u << SHC_OBS_STANCE_PROGRESS | 1u << SHC_OBS_SWING_PROGRESS | 1u << SHC_OBS_TIME_TO_SWING_END;
    if (o.mask & (kProgress | 1u << SHC_OBS_STEP_STATE)) {
      const int word = st.legi[slot];
      if (sel(SHC_OBS_STEP_STATE)) row[o.col[SHC_OBS_STEP_STATE] + leg] = static_cast<T>(double(leg_status_of(word) & 3));
      if (o.mask & kProgress) {
        const V3 vel = frames_desired_velocity(st, rob, rpw);
        const LegMsgProgress pr = leg_msg_progress(a, word, vel.x, vel.y, vel.z);
        if (sel(SHC_OBS_STANCE_PROGRESS)) row[o.col[SHC_OBS_STANCE_PROGRESS] + leg] = static_cast<T>(pr.stance_progress);
        if (sel(SHC_OBS_SWING_PROGRESS)) row[o.col[SHC_OBS_SWING_PROGRESS] + leg] = static_cast<T>(pr.swing_progress);
        if (sel(SHC_OBS_TIME_TO_SWING_END)) row[o.col[SHC_OBS_TIME_TO_SWING_END] + leg] = static_cast<T>(pr.time_to_swing_end);
      }
    }
    // the per-robot fields: the group's first lane
    constexpr uint32_t kRobot = 1u << SHC_OBS_BODY_POSE | 1u << SHC_OBS_DESIRED_VELOCITY | 1u << SHC_OBS_POSE_EULER | 1u << SHC_OBS_ODOM_TO_BASE_LINK | 1u << SHC_OBS_WALK_STATE;
    if (leg == 0 && (o.mask & kRobot)) {
      if (sel(SHC_OBS_DESIRED_VELOCITY)) {
        const V3 vel = frames_desired_velocity(st, rob, rpw);
        T *d = row + o.col[SHC_OBS_DESIRED_VELOCITY];
        d[0] = static_cast<T>(vel.x), d[1] = static_cast<T>(vel.y), d[2] = static_cast<T>(vel.z);
      }
      if (sel(SHC_OBS_WALK_STATE)) row[o.col[SHC_OBS_WALK_STATE]] = static_cast<T>(double(walk_state_of(st.robi, rob, rpw)));
      if (o.mask & (1u << SHC_OBS_BODY_POSE | 1u << SHC_OBS_POSE_EULER | 1u << SHC_OBS_ODOM_TO_BASE_LINK)) {
        // The odometry is read before the current pose, as frame_transforms_kernel's call of body_frames does: the compiler orders the operands of
        // the commutative sums of the quaternion product by where their inputs are defined, and contracts a.w * b.z + a.z * b.w into an fma
        // around the first of them - read the other way round, the last bit of odom_to_base_link's qz differs from that kernel's.
        const Pose odometry = frames_odometry(st, rob, rpw, sel(SHC_OBS_ODOM_TO_BASE_LINK) ? o.have_odom : 0);
        const Pose current = frames_current_pose(st, rob, rpw);
        double v[7];
        if (sel(SHC_OBS_BODY_POSE)) {
          put_pose(v, current);
#pragma unroll
          for (int k = 0; k < 7; ++k) row[o.col[SHC_OBS_BODY_POSE] + k] = static_cast<T>(v[k]);
        }
        if (sel(SHC_OBS_POSE_EULER)) {
          const V3 e = body_pose_euler(current);
          T *d = row + o.col[SHC_OBS_POSE_EULER];
          d[0] = static_cast<T>(e.x), d[1] = static_cast<T>(e.y), d[2] = static_cast<T>(e.z);
        }
        if (sel(SHC_OBS_ODOM_TO_BASE_LINK)) {
          put_pose(v, body_odom_to_base_link(odometry, current));
#pragma unroll
          for (int k = 0; k < 7; ++k) row[o.col[SHC_OBS_ODOM_TO_BASE_LINK] + k] = static_cast<T>(v[k]);
        }
      }
    }
  }
  __syncthreads();
  row_tile_out(out, tile, rg, o, ids, first);
}

// What an engine refuses of a spec that is valid on its own
static int observe_check(const shc_engine *e, const shc_obs_spec *spec, const RowLayout &lay) {
  if (spec->legs < e->L || spec->dof < e->NJ) return fail(SHC_ERR_INVALID_ARG, "shc_obs_spec.legs / dof are below the engine's legs / longest leg's DOF");
  if ((lay.mask & (1u << SHC_OBS_ODOM_TO_BASE_LINK)) && !e->cp.odometry)
    return fail(SHC_ERR_UNSUPPORTED, "SHC_FEAT_ODOMETRY is off: odom_to_base_link needs the ideal odometry");
  if ((lay.mask & (1u << SHC_OBS_VIRTUAL_STIFFNESS)) && !e->params.admittance_control)
    return fail(SHC_ERR_UNSUPPORTED, "admittance_control is off: updateStiffness never runs");
  return SHC_OK;
}

// The launch on the engine's stream: instances [first, first + count) into rows ids[instance] (ids != NULL, a device table) or instance - first
// of the device array `out`.  The caller has checked everything and joined split steps.
static int observe_launch(shc_engine *e, const shc_obs_spec *spec, const RowLayout &lay, void *out, int64_t row_stride, const int64_t *ids, int64_t first, int64_t count) {
  ObsArgs o{};
  row_args(o, lay, spec->dtype, row_stride, spec->legs > e->L || spec->dof > e->NJ, spec->pad);
  o.dof = spec->dof;
  o.derive_poser = derive_poser_tips(e), o.keep_marked = keep_marked_poser_tips(e);
  o.have_odom = e->cp.odometry ? 1 : 0;
  const LegMsgArgs args = leg_msg_args(e->params, e->tables);
  const unsigned grid = row_grid(e->L, first, first + count);
  const size_t lds = row_tile_bytes(e->L, o.pitch, spec->dtype);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    const SharedConsts<L, NJ> *gc = (const SharedConsts<L, NJ> *)e->d_consts;
    if (spec->dtype == SHC_OBS_F32)
      observe_kernel<L, NJ, float><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<float *>(out), e->st, gc, args, o, ids, first, count);
    else
      observe_kernel<L, NJ, double><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<double *>(out), e->st, gc, args, o, ids, first, count);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

extern "C" int shc_engine_get_observations(shc_engine *e, int64_t first, int64_t count, const shc_obs_spec *spec, void *out, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!spec || !out) return fail(SHC_ERR_INVALID_ARG, "spec or out is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<ObsRows>(spec, lay)) return bad;
  int rc = observe_check(e, spec, lay);
  if (rc != SHC_OK) return rc;
  if (first < 0 || count < 0 || first > e->n || count > e->n - first) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if ((rc = row_aligned(out, spec->dtype, "out")) != SHC_OK) return rc;
  if (count == 0) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t stride = row_stride_of(spec, lay);
  if (on_device) return observe_launch(e, spec, lay, out, stride, nullptr, first, count);
  return rows_to_host(e, out, count, lay.width, stride, spec->dtype,
                      [&](void *d) { return observe_launch(e, spec, lay, d, lay.width, nullptr, first, count); });
}
