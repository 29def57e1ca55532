// shc_step_plan.hpp — the step plan pass: every LegStepper's three Bezier curves, stride, clearance, default / target tip and the tip path of the
// rest of its running period as one dense [rows][D] array in one device pass: shc_plan_width, shc_plan_column, shc_engine_get_step_plan.
// Included by shc_engine.hip behind the reach probe (uses its rob_index / walk_state_of, load_leg_fields of shc_leg_msgs.hpp, the row geometry, the
// LDS tile and its mover of shc_rows.hpp and the entry-point macros).  The fleet form (shc_fleet_step_plan.hpp) launches the same kernel with a
// part's caller ids as the row table.
//
// The engine does not store the control nodes: cycle_back regenerates them in registers every iteration.  The node formulas are RESTATED here, line
// by line against walk_controller.cpp and shc_cycle.hpp (the branching form, shc_cycle.hpp:1483-1607, which the straight forms :1370-1480 repeat
// operation for operation) - not hoisted out of the cycle, whose kernels are held to their instructions.  tests/test_gpu_step_plan.py holds the
// two copies together: sample h of SHC_PLAN_PATH must be the walker tip the cycle kernel produces h cycles later.
// The field list is launch-uniform (PlanArgs, a kernel argument): every field sits behind a scalar branch on the mask, so a field that is not
// selected costs neither loads nor arithmetic.
#pragma once

constexpr int kPlanFields = SHC_PLAN_FIELD_COUNT;
static_assert(kPlanFields == 12 && SHC_PLAN_SWING_1_NODES == 0 && SHC_PLAN_PATH == 9 && SHC_PLAN_WALK_PLANE == 10, "ten per-leg fields, then two per-robot fields");
static_assert(sizeof(shc_plan_spec) == 88 && offsetof(shc_plan_spec, row_stride) == 72 && offsetof(shc_plan_spec, pad) == 80,
              "shc_plan_spec: 17 int32, 4 bytes of alignment, row_stride, pad");

// shc_plan_spec for row_layout (shc_rows.hpp): widths scale with the horizon (SHC_PLAN_PATH)
struct PlanRows {
  using Spec = shc_plan_spec;
  static constexpr const char *name = "shc_plan_spec", *n_fields_why = ".n_fields outside 1 .. SHC_PLAN_FIELD_COUNT";
  static constexpr int fields = kPlanFields, most_fields = kPlanFields;
  static constexpr bool has_dof = false;
  static int scale(const Spec *s) { return s->horizon; }
  static bool per_leg(int field) { return field < SHC_PLAN_WALK_PLANE; }
  static int width(int field, int horizon) {
    switch (field) {
      case SHC_PLAN_SWING_1_NODES: case SHC_PLAN_SWING_2_NODES: case SHC_PLAN_STANCE_NODES: return 15;
      case SHC_PLAN_ITERATION: case SHC_PLAN_ITERATIONS: return 1;
      case SHC_PLAN_PATH: return 3 * horizon;
      default: return 3;
    }
  }
  static const char *own(const Spec *s) {
    if (s->horizon < 0 || s->horizon > SHC_PLAN_MAX_HORIZON) return ".horizon outside 0 .. 16";
    if (s->horizon == 0)
      for (int i = 0; i < s->n_fields; ++i)
        if (s->fields[i] == SHC_PLAN_PATH) return ".horizon is 0 and SHC_PLAN_PATH is named";
    return nullptr;
  }
};

extern "C" int64_t shc_plan_width(const shc_plan_spec *spec) { return row_width<PlanRows>(spec); }
extern "C" int shc_plan_column(const shc_plan_spec *spec, int field, int leg, int k) { return row_column<PlanRows>(spec, field, leg, k); }

// The kernel's view of a spec and of the step cycle (CycleParams of the engine's next launch: launch-uniform, scalar loads)
struct PlanArgs : RowArgs<kPlanFields> {
  int32_t horizon; // H
  int32_t period, swing_start, swing_end, stance_start, swing_iterations, stance_iterations;
  int32_t rough, force_normal_touchdown;
  double dt, inv_dt, swing_delta_t, dt_over_swing_dt, stance_dt, swing_height, swing_width;
};

// The geometry and the tile of shc_rows.hpp, copy-out, as observe_kernel: the lanes build their robots' rows in the tile, the rows leave with
// consecutive lanes on consecutive elements.  A lane holds at most two curves at a time (30 doubles); the path loop runs to the launch-uniform H
// with per-lane predicates, and nothing is indexed at run time but the tile.
template <int L, int NJ, class T>
__global__ __launch_bounds__(64) void step_plan_kernel(T *__restrict__ out, DevState st, const SharedConsts<L, NJ> *__restrict__ gc, const PlanArgs a,
                                                       const int64_t *__restrict__ ids, int64_t first, int64_t count) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  const RowGroup<L> rg(first, first + count);
  const int gi = rg.gi, leg = rg.leg;
  const int64_t rob = rg.rob;
  T *tile = row_tile<T>();

  row_tile_pad(tile, rg, a);
  if (rg.live) {
    T *row = tile + gi * a.pitch;
    const T pad = static_cast<T>(a.pad);
    auto sel = [&](int f) { return (a.mask >> f & 1u) != 0; };
    auto put3 = [&](T *d, V3 v, bool defined) {
      d[0] = defined ? static_cast<T>(v.x) : pad, d[1] = defined ? static_cast<T>(v.y) : pad, d[2] = defined ? static_cast<T>(v.z) : pad;
    };
    auto put15 = [&](int f, V3 n0, V3 n1, V3 n2, V3 n3, V3 n4, bool defined) {
      T *d = row + a.col[f] + leg * 15;
      put3(d, n0, defined), put3(d + 3, n1, defined), put3(d + 6, n2, defined), put3(d + 9, n3, defined), put3(d + 12, n4, defined);
    };
    const double2 *planes = reinterpret_cast<const double2 *>(st.legd);
    const int64_t slot = rg.slot;
    auto rob3 = [&](int f) {
      return V3{st.robd[rob_index(rob, f, rpw, R::COUNT)], st.robd[rob_index(rob, f + 1, rpw, R::COUNT)], st.robd[rob_index(rob, f + 2, rpw, R::COUNT)]};
    };
    constexpr uint32_t kCurves = 1u << SHC_PLAN_SWING_1_NODES | 1u << SHC_PLAN_SWING_2_NODES | 1u << SHC_PLAN_STANCE_NODES | 1u << SHC_PLAN_PATH;
    constexpr uint32_t kPeriod = kCurves | 1u << SHC_PLAN_ITERATION | 1u << SHC_PLAN_ITERATIONS;

    // ---- what the last updateTipPosition saw (the header's DEFINITION): iteratePhase (:639) ran behind it (:637)
    bool ran = false, swing = false, standard = true;
    int phase = 0;
    const LegConst<NJ> &lc = gc->leg[leg];
    if (a.mask & (kPeriod | 1u << SHC_PLAN_SWING_CLEARANCE)) {
      const int word = st.legi[slot];
      const int walk_state = walk_state_of(st.robi, rob, rpw);
      const int stored_phase = (word >> LW_PHASE_SHIFT) & LW_PHASE_MASK;
      const bool acp = (word & LW_ACP) != 0, cfs = (word & LW_CFS) != 0;
      const bool walking = st.manual == nullptr || st.manual[rob].leg_state[leg] == LS_WALKING;
      phase = stored_phase - 1;
      if (phase < 0) phase += a.period;
      // The STOPPED -> STARTING cycle (:532-545) sets every phase to its offset, clears at_correct_phase and returns before the steppers.  No
      // later cycle of STARTING leaves that record: a leg gets at_correct_phase in the first cycle that runs, or is held in FORCE_STANCE without it
      // and reaches swing_end before its phase comes round to the offset again (shc_cycle.hpp:1219-1297).  What would break the rule is a
      // setter that writes a phase equal to the offset into a STARTING robot (shc_engine_set_state with such a record): the definition
      // excludes setters since the last cycle.  A robot frozen by a manual leg (:492-505) keeps its record, so its legs keep their curves.
      const bool started_now = walk_state == WS_STARTING && !acp && stored_phase == lc.phase_offset;
      ran = walk_state != WS_STOPPED && walking && (word & 3) != SS_FORCE_STOP && !started_now;
      swing = ran && phase >= a.swing_start && phase < a.swing_end && !(walk_state == WS_STARTING && !acp); // :585-592, :909
      standard = swing || cfs; // :1025 (shc_cycle.hpp:1324)
    }
    const bool stance = ran && !swing;
    // :1026-1041 (shc_cycle.hpp:1325-1328)
    const int mss = standard ? a.stance_start : lc.phase_offset;
    const int stance_iter = standard ? a.stance_iterations : lc.first_stance_iterations;
    const double stance_dt = standard ? a.stance_dt : lc.first_stance_dt;
    int iteration = phase - a.swing_start + 1; // :1050 (shc_cycle.hpp:1493)
    if (!swing) {                              // :1153 (shc_cycle.hpp:1584-1587)
      iteration = mod_i(phase + (a.period - mss), a.period) + 1;
    }
    const int iterations = swing ? a.swing_iterations : stance_iter;
    if (sel(SHC_PLAN_ITERATION)) row[a.col[SHC_PLAN_ITERATION] + leg] = ran ? static_cast<T>(double(iteration)) : pad;
    if (sel(SHC_PLAN_ITERATIONS)) row[a.col[SHC_PLAN_ITERATIONS] + leg] = ran ? static_cast<T>(double(iterations)) : pad;

    // ---- swing_clearance_ (:944, shc_cycle.hpp:1486-1490; external target :1071, shc_cycle.hpp:1532)
    V3 clearance{0, 0, 0};
    if (a.mask & (kCurves | 1u << SHC_PLAN_SWING_CLEARANCE)) {
      V3 pn = rob3(R::PNORM_PREV);
      const bool flat_n = pn.x == 0.0 && pn.y == 0.0 && pn.z == 1.0;
      if (!flat_n) pn = normalized(pn);
      clearance = scaled(pn, a.swing_height);
      if (a.rough && st.ext != nullptr && swing) {
        const double2 cf = reinterpret_cast<const double2 *>(st.ext)[(ExtFields::T_CLEARANCE / 2) * st.n_slots + slot];
        if (int(cf.y) & 1) clearance = normalized(clearance) * cf.x;
      }
      if (sel(SHC_PLAN_SWING_CLEARANCE)) put3(row + a.col[SHC_PLAN_SWING_CLEARANCE] + leg * 3, clearance, true);
    }

    if (a.mask & kCurves) {
      // walker tip, its velocity, swing origin and its velocity, stance origin, default, target, stride: eight 3-vectors, consecutive fields
      double v[24];
      load_leg_fields<FD::TIP, 24>(planes, st.n_slots, slot, v);
      const V3 tip{v[0], v[1], v[2]}, tvel{v[3], v[4], v[5]}, sorg{v[6], v[7], v[8]}, svel{v[9], v[10], v[11]}, torg{v[12], v[13], v[14]};
      const V3 dflt{v[15], v[16], v[17]}, targ{v[18], v[19], v[20]}, strd{v[21], v[22], v[23]};
      if (sel(SHC_PLAN_DEFAULT_TIP)) put3(row + a.col[SHC_PLAN_DEFAULT_TIP] + leg * 3, dflt, true);
      if (sel(SHC_PLAN_TARGET_TIP)) put3(row + a.col[SHC_PLAN_TARGET_TIP] + leg * 3, targ, true);
      if (sel(SHC_PLAN_STRIDE_VECTOR)) put3(row + a.col[SHC_PLAN_STRIDE_VECTOR] + leg * 3, strd, true);

      const bool first_half = iteration <= a.swing_iterations / 2; // :1051
      bool ground_contact = false;                                  // :1110 (shc_cycle.hpp:1511)
      if (a.rough) ground_contact = planes[(FD::STEP_PLANE / 2 + 1) * st.n_slots + slot].y != 0.0;
      // generatePrimarySwingControlNodes (:1238-1261, shc_cycle.hpp:1551-1557)
      V3 mid{(sorg.x + targ.x) / 2.0, (sorg.y + targ.y) / 2.0, fmax(sorg.z, targ.z)};
      mid = mid + clearance;
      mid.y += (lc.stance_y > 0.0) ? a.swing_width : -a.swing_width;
      const V3 sep1 = scaled(svel * 0.25, a.dt_over_swing_dt);
      V3 n1_0 = sorg, n1_1 = sorg + sep1, n1_2 = sorg + scaled(sep1, 2.0);
      V3 n1_3{(mid.x + n1_2.x) / 2.0, (mid.y + n1_2.y) / 2.0, mid.z};
      V3 n1_4 = mid;
      // generateSecondarySwingControlNodes (:1265-1291, shc_cycle.hpp:1559-1564); stance_delta_t_ is the standard one in a swing (:1025)
      const V3 fv = scaled(-strd, a.stance_dt * a.inv_dt);
      const V3 sep2 = scaled(fv * 0.25, a.dt_over_swing_dt);
      V3 n2_0 = n1_4, n2_1 = n1_4 - (n1_3 - n1_4), n2_2 = targ - scaled(sep2, 2.0), n2_3 = targ - sep2, n2_4 = targ;
      if (ground_contact && !first_half) { // :1283-1290: from current_tip_pose_ before this cycle's update (:1134)
        const V3 before = tip - scaled(tvel, a.dt);
        n2_0 = before, n2_1 = before + sep2, n2_2 = before + scaled(sep2, 2.0), n2_3 = before + scaled(sep2, 3.0), n2_4 = before + scaled(sep2, 4.0);
      }
      if (a.force_normal_touchdown && !ground_contact) { // forceNormalTouchdown (:1314-1329, shc_cycle.hpp:1565-1575)
        V3 bo = targ - scaled(sep2, 4.0);
        bo.z = fmax(sorg.z, targ.z);
        bo = bo + clearance;
        n1_4 = bo;
        n2_0 = bo;
        n2_2 = targ - scaled(sep2, 2.0);
        const V3 half = scaled(n2_2 - bo, 0.5);
        n1_3 = n2_0 - half;
        n2_1 = n2_0 + half;
      }
      if (sel(SHC_PLAN_SWING_1_NODES)) put15(SHC_PLAN_SWING_1_NODES, n1_0, n1_1, n1_2, n1_3, n1_4, swing);
      if (sel(SHC_PLAN_SWING_2_NODES)) put15(SHC_PLAN_SWING_2_NODES, n2_0, n2_1, n2_2, n2_3, n2_4, swing);
      // generateStanceControlNodes (:1167, :1295-1310, shc_cycle.hpp:1601-1606): five collinear equispaced nodes
      const double stride_scaler = standard ? 1.0 : lc.first_stride_scaler;
      const V3 sep = scaled((-strd) * stride_scaler, 0.25);
      const V3 s_0 = torg, s_1 = torg + sep, s_2 = torg + scaled(sep, 2.0), s_3 = torg + scaled(sep, 3.0), s_4 = torg + scaled(sep, 4.0);
      if (sel(SHC_PLAN_STANCE_NODES)) put15(SHC_PLAN_STANCE_NODES, s_0, s_1, s_2, s_3, s_4, stance);

      if (sel(SHC_PLAN_PATH)) {
        // curve A: the primary swing curve or the stance curve; curve B: the secondary swing curve (:1121-1130, :1172-1173)
        const V3 a0 = sel3(swing, n1_0, s_0), a1 = sel3(swing, n1_1, s_1), a2 = sel3(swing, n1_2, s_2), a3 = sel3(swing, n1_3, s_3), a4 = sel3(swing, n1_4, s_4);
        const double delta_t = swing ? a.swing_delta_t : stance_dt;
        const int half_iterations = a.swing_iterations / 2;
        V3 p = tip;
        T *d = row + a.col[SHC_PLAN_PATH] + leg * 3 * a.horizon;
        for (int h = 1; h <= a.horizon; ++h, d += 3) {
          const int j = iteration + h;
          const bool on_a = !swing || j <= half_iterations;
          const double t = swing ? (on_a ? a.swing_delta_t * j : a.swing_delta_t * (j - half_iterations)) : j * stance_dt;
          const V3 b0 = sel3(on_a, a0, n2_0), b1 = sel3(on_a, a1, n2_1), b2 = sel3(on_a, a2, n2_2), b3 = sel3(on_a, a3, n2_3), b4 = sel3(on_a, a4, n2_4);
          p = p + scaled(quartic_bezier_dot(b0, b1, b2, b3, b4, t), delta_t); // (shc_cycle.hpp:1578-1581, :1606, :1608)
          put3(d, p, ran && j <= iterations);
        }
      }
    } else {
      auto stored3 = [&](int f, auto field) {
        if (!sel(f)) return;
        double v[3];
        load_leg_fields<decltype(field)::value, 3>(planes, st.n_slots, slot, v);
        put3(row + a.col[f] + leg * 3, V3{v[0], v[1], v[2]}, true);
      };
      stored3(SHC_PLAN_DEFAULT_TIP, std::integral_constant<int, FD::DFLT>{});
      stored3(SHC_PLAN_TARGET_TIP, std::integral_constant<int, FD::TARG>{});
      stored3(SHC_PLAN_STRIDE_VECTOR, std::integral_constant<int, FD::STRD>{});
    }
    // the per-robot fields: the group's first lane
    if (leg == 0) {
      if (sel(SHC_PLAN_WALK_PLANE)) put3(row + a.col[SHC_PLAN_WALK_PLANE], rob3(R::PLANE_PREV), true);
      if (sel(SHC_PLAN_WALK_PLANE_NORMAL)) put3(row + a.col[SHC_PLAN_WALK_PLANE_NORMAL], rob3(R::PNORM_PREV), true);
    }
  }
  __syncthreads();
  row_tile_out(out, tile, rg, a, ids, first);
}

// What an engine refuses of a spec that is valid on its own
static int step_plan_check(const shc_engine *e, const shc_plan_spec *spec) {
  if (spec->legs < e->L) return fail(SHC_ERR_INVALID_ARG, "shc_plan_spec.legs is below the engine's legs");
  return SHC_OK;
}

// The tile rule.  The other row passes' largest tile is 21 rows x 349 x 8 B (the observation pass: 3 legs, every field, 8 x 6 row geometry); the
// widest step plan row - every field, H = 16, 8-leg geometry on 3 legs, float64 - would need 21 x 871 x 8 B.  A row whose tile is larger than the
// others' largest is served in runs of whole consecutive fields, one launch of the same kernel per run, each run as long as its tile stays within
// that size; a field that exceeds it alone (SHC_PLAN_PATH with H = 16 in 8-leg geometry on 3 legs: 21 x 385 x 8 B) is a run of its own, still
// below the 64 KiB a workgroup has without opting into more.
constexpr size_t kPlanTileBytes = size_t(21) * 349 * 8;
static_assert(size_t(64 / 3) * ((SHC_MAX_LEGS * 3 * SHC_PLAN_MAX_HORIZON) | 1) * 8 <= 64 * 1024, "the widest single field fits the LDS of a workgroup");

// The launches on the engine's stream: instances [first, first + count) into rows ids[instance] (ids != NULL, a device table) or instance - first
// of the device array `out`.  The caller has checked everything and joined split steps.
static int step_plan_launch(shc_engine *e, const shc_plan_spec *spec, const RowLayout &lay, void *out, int64_t row_stride, const int64_t *ids, int64_t first, int64_t count) {
  PlanArgs a{};
  a.horizon = spec->horizon;
  const CycleParams &cp = e->cp;
  a.period = cp.period, a.swing_start = cp.swing_start, a.swing_end = cp.swing_end, a.stance_start = cp.stance_start;
  a.swing_iterations = cp.swing_iterations, a.stance_iterations = cp.stance_iterations;
  a.rough = cp.rough_terrain ? 1 : 0, a.force_normal_touchdown = cp.force_normal_touchdown;
  a.dt = cp.dt, a.inv_dt = cp.inv_dt, a.swing_delta_t = cp.swing_delta_t, a.dt_over_swing_dt = cp.dt_over_swing_dt, a.stance_dt = cp.stance_dt;
  a.swing_height = cp.swing_height, a.swing_width = cp.swing_width;
  const unsigned grid = row_grid(e->L, first, first + count);
  const size_t es = row_element_bytes(spec->dtype);
  auto width_of = [&](int f) { return PlanRows::width(f, spec->horizon) * (PlanRows::per_leg(f) ? spec->legs : 1); };
  auto tile_of = [&](int64_t width) { return row_tile_bytes(e->L, int(width) | 1, spec->dtype); };
  for (int i = 0; i < spec->n_fields;) {
    // the run of fields [i, j): the whole row when its tile is no larger than the other passes' largest
    RowLayout run;
    for (int f = 0; f < kRowMaxFields; ++f) run.col[f] = -1;
    run.mask = 0, run.width = 0;
    int j = i;
    const bool whole = tile_of(lay.width) <= kPlanTileBytes;
    while (j < spec->n_fields && (whole || j == i || tile_of(run.width + width_of(spec->fields[j])) <= kPlanTileBytes)) {
      const int f = spec->fields[j++];
      run.mask |= 1u << f, run.col[f] = int32_t(run.width), run.width += width_of(f);
    }
    row_args(a, run, spec->dtype, row_stride, spec->legs > e->L, spec->pad);
    char *dst = static_cast<char *>(out) + size_t(lay.col[spec->fields[i]]) * es;
    const size_t lds = tile_of(run.width);
    const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      const SharedConsts<L, NJ> *gc = (const SharedConsts<L, NJ> *)e->d_consts;
      if (spec->dtype == SHC_OBS_F32)
        step_plan_kernel<L, NJ, float><<<dim3(grid), dim3(64), lds, e->stream>>>(reinterpret_cast<float *>(dst), e->st, gc, a, ids, first, count);
      else
        step_plan_kernel<L, NJ, double><<<dim3(grid), dim3(64), lds, e->stream>>>(reinterpret_cast<double *>(dst), e->st, gc, a, ids, first, count);
      return SHC_OK;
    });
    if (rc != SHC_OK) return rc;
    HIP_TRY(hipGetLastError());
    i = j;
  }
  return SHC_OK;
}

extern "C" int shc_engine_get_step_plan(shc_engine *e, int64_t first, int64_t count, const shc_plan_spec *spec, void *out, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!spec || !out) return fail(SHC_ERR_INVALID_ARG, "spec or out is NULL");
  RowLayout lay;
  if (const int bad = row_resolve<PlanRows>(spec, lay)) return bad;
  int rc = step_plan_check(e, spec);
  if (rc != SHC_OK) return rc;
  if (first < 0 || count < 0 || first > e->n || count > e->n - first) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if ((rc = row_aligned(out, spec->dtype, "out")) != SHC_OK) return rc;
  if (count == 0) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t stride = row_stride_of(spec, lay);
  if (on_device) return step_plan_launch(e, spec, lay, out, stride, nullptr, first, count);
  return rows_to_host(e, out, count, lay.width, stride, spec->dtype,
                      [&](void *d) { return step_plan_launch(e, spec, lay, d, lay.width, nullptr, first, count); });
}
