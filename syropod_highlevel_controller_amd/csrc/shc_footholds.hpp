// shc_footholds.hpp — the foothold pass: the externally requested tip targets / default stance poses of every instance (struct ExternalTarget)
// taken from, or read back into, one dense [n][F] array of float64 or float32 in one device pass: shc_foothold_width, shc_foothold_column,
// shc_engine_set_footholds, shc_engine_get_footholds.  Included by shc_engine.hip behind the three host calls it is defined against
// (shc_engine_set_external_target / _set_external_transform / _get_external_target), whose record table (ext_record), checks and lazy
// allocations (external_select) it uses; the row geometry and the LDS tile are those of shc_rows.hpp.  The fleet form
// (shc_fleet_footholds.hpp) launches the same kernels with a part's caller ids as the row table.
//
// The definition is the host calls': per leg, set leaves what set_external_kernel leaves for a row built from the columns, get writes what
// get_external_kernel reads.  Nothing is computed but the conversions.
#pragma once

constexpr int kFhFields = SHC_FH_FIELD_COUNT;
static_assert(sizeof(shc_foothold_spec) == 64 && offsetof(shc_foothold_spec, row_stride) == 48 && offsetof(shc_foothold_spec, pad) == 56,
              "shc_foothold_spec: 12 int32, row_stride, pad");
static_assert(kFhFields == 6 && SHC_FH_POSITION == 0 && SHC_FH_DEFINED == 5, "position, rotation, transform, clearance, frame, defined");
// the records are laid out alike: pose at base, transform at base + 7, then (target, planner target) clearance and flags, (default) flags
static_assert(ExtFields::T_POSE % 2 == 0 && ExtFields::D_POSE % 2 == 0 && ExtFields::P_POSE % 2 == 0 && ExtFields::T_TRANSFORM == ExtFields::T_POSE + 7 &&
                  ExtFields::D_TRANSFORM == ExtFields::D_POSE + 7 && ExtFields::P_TRANSFORM == ExtFields::P_POSE + 7 && ExtFields::T_CLEARANCE == ExtFields::T_POSE + 14 &&
                  ExtFields::T_FLAGS == ExtFields::T_POSE + 15 && ExtFields::P_CLEARANCE == ExtFields::P_POSE + 14 && ExtFields::P_FLAGS == ExtFields::P_POSE + 15 &&
                  ExtFields::D_FLAGS == ExtFields::D_POSE + 14,
              "the foothold kernels move a record's pose and transform as seven plane pairs from an even base");

// columns per leg of a field
__host__ __device__ constexpr int fh_field_width(int field) { return field == SHC_FH_POSITION ? 3 : field == SHC_FH_ROTATION ? 4 : field == SHC_FH_TRANSFORM ? 7 : 1; }

// shc_foothold_spec for row_layout (shc_rows.hpp): every field is per leg
struct FhRows {
  using Spec = shc_foothold_spec;
  static constexpr const char *name = "shc_foothold_spec", *n_fields_why = ".n_fields outside 1 .. SHC_FH_FIELD_COUNT";
  static constexpr int fields = kFhFields, most_fields = kFhFields;
  static constexpr bool has_dof = false;
  static bool per_leg(int) { return true; }
  static int width(int field, int) { return fh_field_width(field); }
  static const char *own(const Spec *s) {
    if (s->which != SHC_EXTERNAL_TARGET && s->which != SHC_EXTERNAL_DEFAULT && s->which != SHC_EXTERNAL_PLANNER_TARGET)
      return "shc_foothold_spec.which must be SHC_EXTERNAL_TARGET, SHC_EXTERNAL_DEFAULT or SHC_EXTERNAL_PLANNER_TARGET";
    if (s->mode != SHC_FH_REQUEST && s->mode != SHC_FH_REFRESH_TRANSFORM) return "shc_foothold_spec.mode is neither SHC_FH_REQUEST nor SHC_FH_REFRESH_TRANSFORM";
    return nullptr;
  }
};
// ... and what the set calls ask of the fields for the spec's mode (the layout calls and the get calls take any selection)
static const char *fh_set_fields(const shc_foothold_spec *s, const RowLayout &lay) {
  if (s->mode == SHC_FH_REQUEST && !(lay.mask & (1u << SHC_FH_POSITION))) return "SHC_FH_REQUEST needs SHC_FH_POSITION";
  if (s->mode == SHC_FH_REFRESH_TRANSFORM) {
    if (!(lay.mask & (1u << SHC_FH_TRANSFORM))) return "SHC_FH_REFRESH_TRANSFORM needs SHC_FH_TRANSFORM";
    if (lay.mask & ~(1u << SHC_FH_TRANSFORM | 1u << SHC_FH_DEFINED)) return "SHC_FH_REFRESH_TRANSFORM takes SHC_FH_TRANSFORM and SHC_FH_DEFINED only";
  }
  return nullptr;
}

extern "C" int64_t shc_foothold_width(const shc_foothold_spec *spec) { return row_width<FhRows>(spec); }
extern "C" int shc_foothold_column(const shc_foothold_spec *spec, int field, int leg, int k) { return row_column<FhRows>(spec, field, leg, k); }

// The kernels' view of a spec (has_pad, pad: get only)
struct FhArgs : RowArgs<kFhFields> {
  int32_t which, refresh, rough_terrain;
};

// The geometry and the tile of shc_rows.hpp, copy-in: the rows in[row * row_stride], row = ids[robot] or the robot's own index.  Lane (robot, leg)
// then reads its leg's columns back and does what set_external_kernel does for that leg - the same branches in the same order, so the records,
// the sequence state and the count of dropped rows are that kernel's.  A record's pose and transform are seven plane pairs from an even
// field (double2 stores at the lane's slot: consecutive lanes on consecutive 16-byte elements); clearance and flags are the eighth pair of a
// target, the flags of a default a single plane entry.  The dropped rows of the wavefront are counted with a ballot and added by lane 0 with
// one atomic.  The tile is at most 21 rows x 137 x 8 B = 23 KiB (3 legs, every field, 8-leg row geometry); a hexapod's 102-column float32
// row 10 x 103 x 4 B.
template <int L, class T>
__global__ __launch_bounds__(64) void footholds_set_kernel(const T *__restrict__ in, DevState st, SeqRobotState *__restrict__ seq, const FhArgs a,
                                                           const int64_t *__restrict__ ids, unsigned long long *__restrict__ ignored, int64_t first, int64_t end) {
  using X = ExtFields;
  constexpr int rpw = 64 / L;
  const RowGroup<L> rg(first, end);
  const int lane = rg.lane, gi = rg.gi, leg = rg.leg;
  const int64_t rob = rg.rob;
  T *tile = row_tile<T>();

  row_tile_in(tile, in, rg, a, ids, 0);
  __syncthreads();

  bool dropped = false;
  if (rg.live) {
    const T *row = tile + gi * a.pitch;
    auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
    auto column = [&](int f, int k) { return static_cast<double>(row[a.col[f] + leg * fh_field_width(f) + k]); };
    const double d = sel(SHC_FH_DEFINED) ? column(SHC_FH_DEFINED, 0) : 1.0;
    if (d >= 0.0) { // (negative or NaN: the leg is left alone)
      const int64_t slot = rg.slot, ns = st.n_slots;
      double2 *planes = reinterpret_cast<double2 *>(st.ext);
      int which = a.which;
      ExtAt at = ext_record(which);
      if (a.refresh) { // generateExternalTargetTransforms: only defined requests are refreshed
        if ((int(st.ext[leg_field_index(at.flags, slot, ns)]) & 1) != 0) {
#pragma unroll
          for (int k = 0; k < 7; ++k) st.ext[leg_field_index(at.base + 7 + k, slot, ns)] = column(SHC_FH_TRANSFORM, k);
        }
      } else if (!(d > 0.0)) { // withdrawn: defined_ = false, the rest of the record stays
        double &flags = st.ext[leg_field_index(at.flags, slot, ns)];
        flags = double(int(flags) & ~1);
      } else {
        // targetTipPoseCallback, as set_external_kernel: a stepper takes a request only while its robot is not STOPPED; the target of a robot
        // that stands goes to its LegPoser, a default for it - and a stepper request without rough terrain mode - is dropped
        const int walk_state = st.robi[rob_index(rob, RobotFields::I_WORD, rpw, RobotFields::I_COUNT)] & 3;
        if (which == 2 || (which == 0 && walk_state == WS_STOPPED)) {
          which = 2, at = ext_record(2);
          seq[rob].tip_pose_acquired = 1;
        } else if (walk_state == WS_STOPPED || !a.rough_terrain) {
          dropped = true;
        }
        if (!dropped) {
          double v[16]; // pose 0 .. 6, transform 7 .. 13, clearance, flags: the callback's values where the spec names no field
#pragma unroll
          for (int k = 0; k < 3; ++k) v[k] = column(SHC_FH_POSITION, k);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[3 + k] = sel(SHC_FH_ROTATION) ? column(SHC_FH_ROTATION, k) : 0.0;
#pragma unroll
          for (int k = 0; k < 7; ++k) v[7 + k] = sel(SHC_FH_TRANSFORM) ? column(SHC_FH_TRANSFORM, k) : k == 3 ? 1.0 : 0.0;
          v[14] = sel(SHC_FH_SWING_CLEARANCE) ? column(SHC_FH_SWING_CLEARANCE, 0) : 0.0;
          v[15] = double(1 | (sel(SHC_FH_FRAME_IS_ODOM_IDEAL) && column(SHC_FH_FRAME_IS_ODOM_IDEAL, 0) != 0.0 ? 2 : 0));
#pragma unroll
          for (int k = 0; k < 7; ++k) planes[int64_t(at.base / 2 + k) * ns + slot] = double2{v[2 * k], v[2 * k + 1]};
          if (which == 1)
            st.ext[leg_field_index(X::D_FLAGS, slot, ns)] = v[15];
          else
            planes[int64_t(at.base / 2 + 7) * ns + slot] = double2{v[14], v[15]};
        }
      }
    }
  }
  if (ignored) { // launch-uniform
    const unsigned long long m = __ballot(dropped);
    if (lane == 0 && m != 0) atomicAdd(ignored, (unsigned long long)__popcll(m));
  }
}

// The geometry and the tile of shc_rows.hpp, copy-out.  The tile is filled with `pad` first when the row has legs the morphology lacks; lane
// (robot, leg) then loads its leg's record - eight plane pairs of a target, seven and the flags of a default - and writes the selected columns
// as get_external_kernel and the host getter's conversion give them; the rows leave with consecutive lanes on consecutive elements.
template <int L, class T>
__global__ __launch_bounds__(64) void footholds_get_kernel(T *__restrict__ out, DevState st, const FhArgs a, const int64_t *__restrict__ ids, int64_t first, int64_t end) {
  using X = ExtFields;
  const RowGroup<L> rg(first, end);
  const int gi = rg.gi, leg = rg.leg;
  T *tile = row_tile<T>();

  row_tile_pad(tile, rg, a);
  if (rg.live) {
    T *row = tile + gi * a.pitch;
    auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
    auto put = [&](int f, int k, double x) { row[a.col[f] + leg * fh_field_width(f) + k] = static_cast<T>(x); };
    const int64_t slot = rg.slot, ns = st.n_slots;
    const double2 *planes = reinterpret_cast<const double2 *>(st.ext);
    const ExtAt at = ext_record(a.which);
    double v[16];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double2 p = planes[int64_t(at.base / 2 + k) * ns + slot];
      v[2 * k] = p.x, v[2 * k + 1] = p.y;
    }
    if (a.which == 1) {
      v[14] = 0.0, v[15] = st.ext[leg_field_index(X::D_FLAGS, slot, ns)];
    } else {
      const double2 p = planes[int64_t(at.base / 2 + 7) * ns + slot];
      v[14] = p.x, v[15] = p.y;
    }
    if (sel(SHC_FH_POSITION)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) put(SHC_FH_POSITION, k, v[k]);
    }
    if (sel(SHC_FH_ROTATION)) {
#pragma unroll
      for (int k = 0; k < 4; ++k) put(SHC_FH_ROTATION, k, v[3 + k]);
    }
    if (sel(SHC_FH_TRANSFORM)) {
#pragma unroll
      for (int k = 0; k < 7; ++k) put(SHC_FH_TRANSFORM, k, v[7 + k]);
    }
    if (sel(SHC_FH_SWING_CLEARANCE)) put(SHC_FH_SWING_CLEARANCE, 0, v[14]);
    const int flags = int(v[15]);
    if (sel(SHC_FH_FRAME_IS_ODOM_IDEAL)) put(SHC_FH_FRAME_IS_ODOM_IDEAL, 0, double((flags >> 1) & 1));
    if (sel(SHC_FH_DEFINED)) put(SHC_FH_DEFINED, 0, double(flags & 1));
  }
  __syncthreads();
  row_tile_out(out, tile, rg, a, ids, 0);
}

// What an engine refuses of a spec that is valid on its own (the host calls' own answers: external_select)
static int footholds_check(const shc_engine *e, const shc_foothold_spec *spec) {
  if (spec->legs < e->L) return fail(SHC_ERR_INVALID_ARG, "shc_foothold_spec.legs is below the engine's legs");
  if (spec->which == SHC_EXTERNAL_DEFAULT && !e->params.rough_terrain_mode)
    return fail(SHC_ERR_UNSUPPORTED, "external default poses are read in rough_terrain_mode only (walk_controller.cpp:988)");
  return SHC_OK;
}

static FhArgs fh_args(const shc_engine *e, const shc_foothold_spec *spec, const RowLayout &lay, int64_t row_stride) {
  FhArgs a{};
  row_args(a, lay, spec->dtype, row_stride, spec->legs > e->L, spec->pad);
  a.which = spec->which, a.refresh = spec->mode == SHC_FH_REFRESH_TRANSFORM, a.rough_terrain = e->params.rough_terrain_mode ? 1 : 0;
  return a;
}

// The set pass over every instance of an engine on its stream, with the host call's host-side effects.  `in` and `ignored` are device
// pointers ready on the engine's stream; rows ids[instance] (ids != NULL, a device table) or instance.  The caller has checked everything and
// joined split steps.
static int footholds_apply(shc_engine *e, const shc_foothold_spec *spec, const RowLayout &lay, const void *in, int64_t row_stride, const int64_t *ids, int64_t *ignored) {
  int64_t n_rows = 0;
  int rc = external_select(e, spec->which, 0, e->n, -1, &n_rows); // the lazy allocations of the host calls (records, sequence state)
  if (rc != SHC_OK) return rc;
  if (spec->mode == SHC_FH_REQUEST) e->rt_flags |= RT_EXTERNAL; // as shc_engine_set_external_target
  const FhArgs a = fh_args(e, spec, lay, row_stride);
  const unsigned grid = row_grid(e->L, 0, e->n);
  const size_t lds = row_tile_bytes(e->L, a.pitch, spec->dtype);
  unsigned long long *ign = reinterpret_cast<unsigned long long *>(ignored);
  rc = dispatch_legs(e, [&](auto l) -> int {
    constexpr int L = decltype(l)::value;
    if (spec->dtype == SHC_OBS_F32)
      footholds_set_kernel<L, float><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<const float *>(in), e->st, e->d_seq, a, ids, ign, 0, e->n);
    else
      footholds_set_kernel<L, double><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<const double *>(in), e->st, e->d_seq, a, ids, ign, 0, e->n);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

// The get pass: every instance's records into rows ids[instance] or instance of the device array `out`, on the engine's stream
static int footholds_read(shc_engine *e, const shc_foothold_spec *spec, const RowLayout &lay, void *out, int64_t row_stride, const int64_t *ids) {
  int64_t n_rows = 0;
  int rc = external_select(e, spec->which, 0, e->n, -1, &n_rows); // (the host getter's lazy allocations)
  if (rc != SHC_OK) return rc;
  const FhArgs a = fh_args(e, spec, lay, row_stride);
  const unsigned grid = row_grid(e->L, 0, e->n);
  const size_t lds = row_tile_bytes(e->L, a.pitch, spec->dtype);
  rc = dispatch_legs(e, [&](auto l) -> int {
    constexpr int L = decltype(l)::value;
    if (spec->dtype == SHC_OBS_F32)
      footholds_get_kernel<L, float><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<float *>(out), e->st, a, ids, 0, e->n);
    else
      footholds_get_kernel<L, double><<<dim3(grid), dim3(64), lds, e->stream>>>(static_cast<double *>(out), e->st, a, ids, 0, e->n);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

extern "C" int shc_engine_set_footholds(shc_engine *e, const shc_foothold_spec *spec, const void *rows, int on_device, int64_t *ignored) {
  SHC_ENTER(e);
  if (!spec || !rows) return fail(SHC_ERR_INVALID_ARG, "spec or rows is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<FhRows>(spec, lay)) return bad;
  if (const char *fields = fh_set_fields(spec, lay)) return fail(SHC_ERR_INVALID_ARG, fields);
  int rc = footholds_check(e, spec);
  if (rc != SHC_OK) return rc;
  if ((rc = row_aligned(rows, spec->dtype, "rows")) != SHC_OK) return rc;
  if (reinterpret_cast<uintptr_t>(ignored) & 7) return fail(SHC_ERR_INVALID_ARG, "ignored must be aligned to 8 bytes");
  if ((rc = join_side(e)) != SHC_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t stride = row_stride_of(spec, lay);
  if (on_device) return footholds_apply(e, spec, lay, rows, stride, nullptr, ignored);
  int64_t h_ignored = 0; // (the count's word stands behind the rows on the device)
  rc = rows_from_host(e, rows, e->n, lay.width, stride, spec->dtype, &h_ignored,
                      [&](const void *d, int64_t *d_ignored) { return footholds_apply(e, spec, lay, d, lay.width, nullptr, d_ignored); });
  if (rc == SHC_OK && ignored) *ignored += h_ignored;
  return rc;
}

extern "C" int shc_engine_get_footholds(shc_engine *e, const shc_foothold_spec *spec, void *rows, int on_device) {
  SHC_ENTER(e);
  if (!spec || !rows) return fail(SHC_ERR_INVALID_ARG, "spec or rows is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<FhRows>(spec, lay)) return bad;
  if (spec->mode != SHC_FH_REQUEST) return fail(SHC_ERR_INVALID_ARG, "shc_foothold_spec.mode must be 0 for shc_engine_get_footholds");
  int rc = footholds_check(e, spec);
  if (rc != SHC_OK) return rc;
  if ((rc = row_aligned(rows, spec->dtype, "rows")) != SHC_OK) return rc;
  if ((rc = join_side(e)) != SHC_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t stride = row_stride_of(spec, lay);
  if (on_device) return footholds_read(e, spec, lay, rows, stride, nullptr);
  return rows_to_host(e, rows, e->n, lay.width, stride, spec->dtype, [&](void *d) { return footholds_read(e, spec, lay, d, lay.width, nullptr); });
}
