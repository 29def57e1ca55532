// shc_reach.hpp — the reach probe: how far along the straight line from its present tip position to a candidate tip target every leg of
// every instance gets with the engine's own IK, for C candidates per robot, in one device pass that writes nothing into the engine:
// shc_reach_width, shc_reach_column, shc_engine_probe_reach.  Included by shc_engine.hip behind the foothold pass (uses apply_ik_core of
// shc_leg_api.hpp, load_leg_fields of shc_leg_msgs.hpp, the row geometry, the LDS tile and its mover of shc_rows.hpp and the entry-point
// macros).  The fleet form (shc_fleet_reach.hpp) launches the same kernel with a part's caller ids as the row table.
//
// The definition is the line search of Leg::generateWorkspace (model.cpp:397-470) with the per-leg calls of the boundary: per candidate,
// S times setDesiredTipPose(o + (t - o) s / S, rotation undefined) and applyIK(simulation = true) from the stored joints, stopped at the
// first step that returns 0.  What shc_leg_apply_ik runs per leg is apply_ik_core; the closing tip-force estimate feeds nothing back into
// the joints and nothing is stored, so it is left out.
#pragma once

constexpr int kReachFields = SHC_REACH_FIELD_COUNT;
static_assert(kReachFields == 4 && SHC_REACH_FRACTION == 0 && SHC_REACH_Q == 3, "fraction, limit proximity, tip, q");
static_assert(sizeof(shc_reach_spec) == 72 && offsetof(shc_reach_spec, row_stride) == 48 && offsetof(shc_reach_spec, target_row_stride) == 56 &&
                  offsetof(shc_reach_spec, pad) == 64,
              "shc_reach_spec: 11 int32, 4 bytes of alignment, row_stride, target_row_stride, pad");
constexpr int kReachMaxCandidates = 64, kReachMaxSteps = 4096;

// shc_reach_spec for row_layout (shc_rows.hpp): every field is per leg; the layout is that of ONE candidate's block
struct ReachRows {
  using Spec = shc_reach_spec;
  static constexpr const char *name = "shc_reach_spec", *n_fields_why = ".n_fields outside 1 .. SHC_REACH_FIELD_COUNT";
  static constexpr int fields = kReachFields, most_fields = kReachFields;
  static constexpr bool has_dof = true;
  static bool per_leg(int) { return true; }
  static int width(int field, int dof) { return field == SHC_REACH_TIP ? 3 : field == SHC_REACH_Q ? dof : 1; }
  static const char *own(const Spec *s) {
    if (s->candidates < 1 || s->candidates > kReachMaxCandidates) return ".candidates outside 1 .. 64";
    if (s->steps < 1 || s->steps > kReachMaxSteps) return ".steps outside 1 .. 4096";
    return nullptr;
  }
};
// row_layout, and what the two strides of a robot's rows ask: C blocks of D columns, C blocks of legs x 3 columns
static const char *reach_layout(const shc_reach_spec *s, RowLayout &lay) {
  if (const char *why = row_layout<ReachRows>(s, lay)) return why;
  if (s->row_stride != 0 && s->row_stride < lay.width * s->candidates) return ".row_stride is below candidates x the width of a block";
  if (s->target_row_stride != 0 && s->target_row_stride < int64_t(s->candidates) * s->legs * 3) return ".target_row_stride is below candidates x legs x 3";
  return nullptr;
}
static int reach_resolve(const shc_reach_spec *spec, RowLayout &lay) {
  const char *why = reach_layout(spec, lay);
  if (!why) return SHC_OK;
  return fail(SHC_ERR_INVALID_ARG, why[0] == '.' ? std::string(ReachRows::name) + why : std::string(why));
}

extern "C" int64_t shc_reach_width(const shc_reach_spec *spec) {
  RowLayout lay;
  if (const int bad = reach_resolve(spec, lay)) return -int64_t(bad);
  return lay.width;
}
extern "C" int shc_reach_column(const shc_reach_spec *spec, int field, int leg, int k) {
  RowLayout lay;
  if (reach_layout(spec, lay)) return -1;
  return row_column<ReachRows>(spec, field, leg, k);
}

// The kernel's view of a spec: the head serves the mover on the output side (one candidate's block of D columns, the robots row_stride
// apart), `in` on the target side (one candidate's legs x 3 columns)
struct ReachIn {
  int32_t width, pitch;
  int64_t row_stride;
};
struct ReachArgs : RowArgs<kReachFields> {
  ReachIn in;
  int32_t dof;       // columns per leg of SHC_REACH_Q
  int32_t steps;     // S
  int32_t clamp_pos; // clamp_joint_positions
  double dt;         // time_delta
};

// desired = o (1 - w) + t w per component: each product and the sum rounded once
__device__ __forceinline__ V3 reach_desired(V3 o, V3 t, double w) {
#pragma clang fp contract(off)
  const double u = 1.0 - w;
  const double x0 = o.x * u, x1 = t.x * w, y0 = o.y * u, y1 = t.y * w, z0 = o.z * u, z1 = t.z * w;
  return V3{x0 + x1, y0 + y1, z0 + z1};
}

// What one leg's line search leaves
template <int NJ>
struct ReachLeg {
  double q[NJ];
  V3 tip;
  double proximity;
  int done;
};
// The line search of one lane from its stored joints.  `alive` is the lane's own; the loop runs as long as a lane of the wavefront is alive
// (the trip count is a kernel argument and the ballot is wave-uniform), a lane that has stopped rides along masked.  Nothing is stored: the
// state is read through a const reference, once, as whole planes.
template <int NJ>
__device__ __forceinline__ void reach_search(const DevState &st, const LegConst<NJ> &lc, int64_t slot, bool alive, V3 target, const ReachArgs &a, ReachLeg<NJ> &r) {
  using FD = Fields<NJ>;
  static_assert(FD::Q == 0 && FD::QD == NJ, "Q and QD are the first planes of a leg slot");
  double qd[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) r.q[j] = 0.0, qd[j] = 0.0;
  r.tip = V3{0.0, 0.0, 0.0}, r.proximity = 0.0, r.done = 0;
  V3 origin{0.0, 0.0, 0.0};
  if (alive) {
    double v[2 * NJ];
    load_leg_fields<FD::Q, 2 * NJ>(reinterpret_cast<const double2 *>(st.legd), st.n_slots, slot, v);
#pragma unroll
    for (int j = 0; j < NJ; ++j) r.q[j] = v[j], qd[j] = v[NJ + j];
    Chain<NJ> ch;
    fk_chain<NJ>(lc, r.q, ch);
    origin = tip_robot_frame(lc, ch.pe); // what apply_ik_dev measures from the stored joints
    r.tip = origin;
  }
  const double steps = double(a.steps);
  for (int s = 1; s <= a.steps; ++s) {
    if (__ballot(alive) == 0) break;
    if (alive) {
      const V3 desired = reach_desired(origin, target, double(s) / steps);
      Chain<NJ> ch; // (rotation undefined: one position solve, no retry; nothing to keep beside the joints)
      const IkOutcome ik = apply_ik_core<NJ>(
          lc, r.q, qd, desired, false, V3{0.0, 0.0, 0.0}, false, a.clamp_pos != 0, a.dt, ch, []() {}, [](const Chain<NJ> &, bool) {});
      r.tip = tip_robot_frame(lc, ch.pe);
      r.proximity = ik.success;
      if (ik.success == 0.0)
        alive = false;
      else
        ++r.done;
    }
  }
}

// The geometry of shc_rows.hpp, one leg per lane, with the candidates as the grid's second dimension: block (b, c) serves candidate c of the
// robot group b.  The wavefront copies candidate c's legs x 3 target columns of its robots into the tile, every lane takes its leg's three,
// and the same LDS then becomes the output tile - filled with `pad` where the row has columns no lane owns - that the lanes write their
// columns into and that leaves with consecutive lanes on consecutive elements: rows ids[robot] (a fleet part's caller ids) or robot - first.
// A lane whose target has a NaN is not asked: its columns hold `pad`.  The largest tile is 21 rows x 89 x 8 B = 14.6 KiB (3 legs, every
// field, 8 x 6 row geometry); a hexapod's fraction + limit proximity + tip in float32 10 x 31 x 4 B.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void reach_probe_kernel(T *__restrict__ out, const T *__restrict__ targets, const DevState st, const SharedConsts<L, NJ> *__restrict__ gc,
                                                         const ReachArgs a, const int64_t *__restrict__ ids, int64_t first, int64_t end) {
  const RowGroup<L> rg(first, end);
  const int gi = rg.gi, leg = rg.leg;
  const int cand = blockIdx.y;
  T *tile = row_tile<T>();

  row_tile_in(tile, targets + int64_t(cand) * a.in.width, rg, a.in, ids, first);
  __syncthreads();
  V3 target{0.0, 0.0, 0.0};
  if (rg.live) {
    const T *t = tile + gi * a.in.pitch + leg * 3;
    target = V3{static_cast<double>(t[0]), static_cast<double>(t[1]), static_cast<double>(t[2])};
  }
  __syncthreads(); // the tile changes sides
  const bool asked = rg.live && target.x == target.x && target.y == target.y && target.z == target.z;

  ReachLeg<NJ> r;
  reach_search<NJ>(st, gc->leg[leg], rg.slot, asked, target, a, r);

  row_tile_pad(tile, rg, a);
  if (rg.live) {
    T *row = tile + gi * a.pitch;
    const T pad = static_cast<T>(a.pad);
    auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
    if (sel(SHC_REACH_FRACTION)) row[a.col[SHC_REACH_FRACTION] + leg] = asked ? static_cast<T>(double(r.done) / double(a.steps)) : pad;
    if (sel(SHC_REACH_LIMIT_PROXIMITY)) row[a.col[SHC_REACH_LIMIT_PROXIMITY] + leg] = asked ? static_cast<T>(r.proximity) : pad;
    if (sel(SHC_REACH_TIP)) {
      T *d = row + a.col[SHC_REACH_TIP] + leg * 3;
      d[0] = asked ? static_cast<T>(r.tip.x) : pad, d[1] = asked ? static_cast<T>(r.tip.y) : pad, d[2] = asked ? static_cast<T>(r.tip.z) : pad;
    }
    if (sel(SHC_REACH_Q)) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) row[a.col[SHC_REACH_Q] + leg * a.dof + j] = asked ? static_cast<T>(r.q[j]) : pad;
    }
  }
  __syncthreads();
  row_tile_out(out + int64_t(cand) * a.width, tile, rg, a, ids, first);
}

// ---- host side
// What an engine refuses of a spec that is valid on its own
static int reach_check(const shc_engine *e, const shc_reach_spec *spec) {
  if (spec->legs < e->L || spec->dof < e->NJ) return fail(SHC_ERR_INVALID_ARG, "shc_reach_spec.legs / dof are below the engine's legs / longest leg's DOF");
  return SHC_OK;
}
// ... and of the two arrays, whoever calls
static int reach_arrays_check(const shc_reach_spec *spec, const void *targets, const void *out) {
  const int rc = row_aligned(targets, spec->dtype, "targets");
  return rc != SHC_OK ? rc : row_aligned(out, spec->dtype, "out");
}

// The launch on the engine's stream: instances [first, first + count), their targets in and their blocks into rows ids[instance] (ids != NULL,
// a device table) or instance - first of the two device arrays.  The caller has checked everything and joined split steps.
static int reach_launch(shc_engine *e, const shc_reach_spec *spec, const RowLayout &lay, const void *targets, void *out, const int64_t *ids, int64_t first, int64_t count) {
  if (count == 0) return SHC_OK;
  ReachArgs a{};
  row_args(a, lay, spec->dtype, spec->row_stride ? spec->row_stride : lay.width * spec->candidates, spec->legs > e->L || spec->dof > e->NJ, spec->pad);
  a.in.width = spec->legs * 3, a.in.pitch = a.in.width | 1;
  a.in.row_stride = spec->target_row_stride ? spec->target_row_stride : int64_t(spec->candidates) * a.in.width;
  a.dof = spec->dof, a.steps = spec->steps, a.clamp_pos = e->params.clamp_joint_positions ? 1 : 0, a.dt = e->params.time_delta;
  const dim3 grid(row_grid(e->L, first, first + count), unsigned(spec->candidates));
  const size_t lds = row_tile_bytes(e->L, std::max(a.pitch, a.in.pitch), spec->dtype);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    const SharedConsts<L, NJ> *gc = (const SharedConsts<L, NJ> *)e->d_consts;
    if (spec->dtype == SHC_OBS_F32)
      reach_probe_kernel<L, NJ, float><<<grid, dim3(64), lds, e->stream>>>(static_cast<float *>(out), static_cast<const float *>(targets), e->st, gc, a, ids, first, first + count);
    else
      reach_probe_kernel<L, NJ, double><<<grid, dim3(64), lds, e->stream>>>(static_cast<double *>(out), static_cast<const double *>(targets), e->st, gc, a, ids, first,
                                                                           first + count);
    return SHC_OK;
  });
  if (rc != SHC_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SHC_OK;
}

extern "C" int shc_engine_probe_reach(shc_engine *e, int64_t first, int64_t count, const shc_reach_spec *spec, const void *targets, void *out) {
  SHC_ENTER(e);
  if (!spec || !targets || !out) return fail(SHC_ERR_INVALID_ARG, "spec, targets or out is NULL");
  RowLayout lay;
  if (const int bad = reach_resolve(spec, lay)) return bad;
  int rc = reach_check(e, spec);
  if (rc != SHC_OK) return rc;
  if (first < 0 || count < 0 || first > e->n || count > e->n - first) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if ((rc = reach_arrays_check(spec, targets, out)) != SHC_OK) return rc;
  if (count == 0) return SHC_OK;
  if ((rc = join_side(e)) != SHC_OK) return rc; // split launches: the engine's stream follows both halves before it reads their joints
  HIP_TRY(hipSetDevice(e->device));
  return reach_launch(e, spec, lay, targets, out, nullptr, first, count);
}
