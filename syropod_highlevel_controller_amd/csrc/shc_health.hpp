// shc_health.hpp — the reference's tracking warnings ("IK Clamping Event/s", model.cpp:811-853; "Inverse kinematics deviation!", :914-929; the limit
// proximity updateJointPositions / applyIK return, :843-849, :903, :940) for a range of instances in one device pass: shc_engine_scan_health.
// Included by shc_engine.hip (uses its rob_index, derive_tips, load_leg_fields of shc_leg_msgs.hpp and the entry-point macros).
//
// The arithmetic lives in two host + device functions, leg_health (one leg) and robot_health (the record of one robot from its legs);
// health_scan_kernel calls them, and so does the host-only shc_debug_robot_health.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

static_assert(sizeof(shc_robot_health) == 32 && offsetof(shc_robot_health, flags) == 24 && offsetof(shc_robot_health, leg_masks) == 28,
              "shc_robot_health is 32 bytes without padding");
static_assert(sizeof(shc_health_criteria) == 24, "shc_health_criteria is 24 bytes");
constexpr uint32_t kHealthAllFlags = SHC_HEALTH_IK_DEVIATION | SHC_HEALTH_POSITION_LIMIT | SHC_HEALTH_SPEED_LIMIT | SHC_HEALTH_NEAR_LIMIT |
                                     SHC_HEALTH_TIP_DEVIATION | SHC_HEALTH_NONFINITE;

// What one leg contributes.  bits: 1 = IK deviation, 2 = on a position limit, 4 = on the speed limit, 8 = a non-finite value
struct LegHealth {
  double proximity, deviation, speed_ratio;
  uint32_t bits;
};
SHC_HD bool health_finite(double v) { return v - v == 0.0; } // false for NaN and +-Inf (no library call: host and device agree)
SHC_HD bool health_finite(const V3 &v) { return health_finite(v.x) && health_finite(v.y) && health_finite(v.z); }

// One leg, over its own joints (LegConst::jactive; the padding joints of a shorter leg have no limits and no motor):
//   proximity    Leg::updateJointPositions' return value (model.cpp:803, :843-849) on the stored desired_position_: starting from 1.0, the
//                minimum of min(|min - q|, |max - q|) / ((max - min) / 2) - a true division - with 1.0 for a zero-range joint (:848)
//   bit 2        a joint of non-zero range with q <= min or q >= max: the state a position clamp leaves (:827-841)
//   speed_ratio  the maximum of |desired_velocity_| / max_angular_speed_ (:814); bit 4: a joint with ratio >= 1, the state a velocity clamp leaves (:812-821)
//   deviation    the maximum over the axes of |current_tip_pose_ - desired_tip_pose_| (:918), desired_tip_pose_ = poser tip + admittance_delta_
//                (setDesiredTipPose, :660-661); apply_delta = false for a MANUAL / WALKING_TO_MANUAL leg (:656)
//   bit 1        the leg word's LW_IKFAIL (:916-929); bit 8: any of the values above, or the walker tip, is NaN / +-Inf
// Minima and maxima skip NaN operands (fmin / fmax), so the flags of a non-finite robot are still defined.
template <int NJ, class LC>
SHC_HD LegHealth leg_health(const LC &lc, const double (&q)[NJ], const double (&qd)[NJ], const V3 &walker_tip, const V3 &poser_tip, const V3 &model_tip,
                            const V3 &admittance_delta, bool apply_delta, bool ik_failed) {
  LegHealth h{1.0, 0.0, 0.0, ik_failed ? 1u : 0u};
  bool finite = health_finite(walker_tip) && health_finite(poser_tip) && health_finite(model_tip) && health_finite(admittance_delta);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (lc.jactive[j] == 0.0) continue;
    finite = finite && health_finite(q[j]) && health_finite(qd[j]);
    const double min_diff = fabs(lc.jmin[j] - q[j]), max_diff = fabs(lc.jmax[j] - q[j]);
    const double half_joint_range = (lc.jmax[j] - lc.jmin[j]) / 2.0;
    const double limit_proximity = half_joint_range != 0.0 ? fmin(min_diff, max_diff) / half_joint_range : 1.0;
    h.proximity = fmin(h.proximity, limit_proximity);
    if (half_joint_range != 0.0 && (q[j] <= lc.jmin[j] || q[j] >= lc.jmax[j])) h.bits |= 2u;
    const double ratio = fabs(qd[j]) / lc.jvmax[j];
    h.speed_ratio = fmax(h.speed_ratio, ratio);
    if (ratio >= 1.0) h.bits |= 4u;
  }
  const V3 desired = apply_delta ? poser_tip + admittance_delta : poser_tip;
  const V3 e = model_tip - desired;
  h.deviation = fmax(fmax(fabs(e.x), fabs(e.y)), fabs(e.z));
  if (!finite) h.bits |= 8u;
  return h;
}

// The record of one robot from its legs: leg(l) returns the LegHealth of leg l (an array on the host, a cross-lane read in the kernel).
// NULL criteria of the ABI arrive here as select 0 with thresholds no value passes (-Inf / +Inf).
template <class LegOf>
SHC_HD shc_robot_health robot_health(int legs, LegOf &&leg, bool pose_finite, const shc_health_criteria &c) {
  shc_robot_health r;
  r.min_limit_proximity = 1.0, r.max_tip_deviation = 0.0, r.max_speed_ratio = 0.0;
  uint32_t masks = 0;
#pragma unroll
  for (int l = 0; l < legs; ++l) {
    const LegHealth h = leg(l);
    r.min_limit_proximity = fmin(r.min_limit_proximity, h.proximity);
    r.max_tip_deviation = fmax(r.max_tip_deviation, h.deviation);
    r.max_speed_ratio = fmax(r.max_speed_ratio, h.speed_ratio);
    masks |= ((h.bits & 1u) << l) | (((h.bits >> 1) & 1u) << (8 + l)) | (((h.bits >> 2) & 1u) << (16 + l)) | (((h.bits >> 3) & 1u) << (24 + l));
  }
  uint32_t flags = 0;
  if (masks & 0x000000ffu) flags |= SHC_HEALTH_IK_DEVIATION;
  if (masks & 0x0000ff00u) flags |= SHC_HEALTH_POSITION_LIMIT;
  if (masks & 0x00ff0000u) flags |= SHC_HEALTH_SPEED_LIMIT;
  if ((masks & 0xff000000u) || !pose_finite) flags |= SHC_HEALTH_NONFINITE;
  if (r.min_limit_proximity < c.near_limit_proximity) flags |= SHC_HEALTH_NEAR_LIMIT;
  if (r.max_tip_deviation > c.tip_deviation) flags |= SHC_HEALTH_TIP_DEVIATION;
  r.flags = flags, r.leg_masks = masks;
  return r;
}

static shc_health_criteria health_criteria(const shc_health_criteria *c) {
  if (c) return *c;
  return shc_health_criteria{0u, 0u, -INFINITY, INFINITY};
}

// ---- the batched form
// Pass 1.  The geometry of shc_rows.hpp (RowGroup) for [first, first + count), the joint planes read as double2 per lane.  The per-leg figures meet in
// the robot over the L lanes of its group (Group<L>: the cycle's cross-lane reads); every lane of a group forms the same record.  The records of a
// wavefront are consecutive in `health`: each group's first lane puts its 32 bytes into an LDS strip and the wavefront writes the strip out as
// contiguous 16-byte stores.  restore_map takes i or -1 for the robots of the range here (the entries outside it are filled by the caller), and
// the wavefront's selection - bit g = robot g of the group is selected - goes to wave_mask[b], its population count to wave_count[b], for the
// compaction passes below.  MODEL_TIP / POSER_TIP must have been derived (derive_tips).
template <int L, int NJ>
__global__ __launch_bounds__(64) void health_scan_kernel(ulonglong2 *__restrict__ health, int64_t *__restrict__ restore_map,
                                                         unsigned long long *__restrict__ wave_mask, uint32_t *__restrict__ wave_count, DevState st,
                                                         const SharedConsts<L, NJ> *__restrict__ gc, const shc_health_criteria crit, int64_t first,
                                                         int64_t count) {
  using FD = Fields<NJ>;
  using R = RobotFields;
  constexpr int rpw = 64 / L;
  __shared__ ulonglong2 strip[2 * rpw];
  // (RowGroup's lines written out: taken through the struct this kernel, alone of the seven, allocates two more SGPRs)
  const int lane = threadIdx.x;
  const int64_t w = first / rpw + blockIdx.x;
  const int gi = lane / L, leg = lane - gi * L;
  const int64_t rob = w * rpw + gi, end = first + count;
  const bool live = gi < rpw && rob >= first && rob < end;
  const int64_t rob_lo = w * rpw > first ? w * rpw : first, rob_hi = (w + 1) * rpw < end ? (w + 1) * rpw : end;
  const int g0 = int(rob_lo - w * rpw), n_rob = int(rob_hi - rob_lo);

  LegHealth lh{1.0, 0.0, 0.0, 0u};
  bool pose_finite = true;
  if (live) {
    const double2 *planes = reinterpret_cast<const double2 *>(st.legd);
    const int64_t slot = w * 64 + lane;
    double v[2 * NJ + 3], q[NJ], qd[NJ], pt[3], mt[3], ad[3]; // Q, QD, TIP are consecutive fields
    load_leg_fields<FD::Q, 2 * NJ + 3>(planes, st.n_slots, slot, v);
#pragma unroll
    for (int j = 0; j < NJ; ++j) q[j] = v[j], qd[j] = v[NJ + j];
    load_leg_fields<FD::POSER_TIP, 3>(planes, st.n_slots, slot, pt);
    load_leg_fields<FD::MODEL_TIP, 3>(planes, st.n_slots, slot, mt);
    load_leg_fields<FD::ADM_DELTA, 3>(planes, st.n_slots, slot, ad);
    const int leg_state = st.manual != nullptr ? st.manual[rob].leg_state[leg] : LS_WALKING;
    lh = leg_health<NJ>(gc->leg[leg], q, qd, V3{v[2 * NJ], v[2 * NJ + 1], v[2 * NJ + 2]}, V3{pt[0], pt[1], pt[2]}, V3{mt[0], mt[1], mt[2]},
                        V3{ad[0], ad[1], ad[2]}, leg_state != LS_MANUAL && leg_state != LS_WALKING_TO_MANUAL, (st.legi[slot] & LW_IKFAIL) != 0);
#pragma unroll
    for (int k = 0; k < 7; ++k) pose_finite = pose_finite && health_finite(st.robd[rob_index(rob, R::CPOSE + k, rpw, R::COUNT)]); // Model::current_pose_
  }
  // (every lane of the wavefront takes part in the cross-lane reads; the lanes past the last group read group 0 and are not used)
  const Group<L> grp{gi < rpw ? gi * L : 0};
  const shc_robot_health rec = robot_health(
      L, [&](int l) { return LegHealth{grp.get(lh.proximity, l), grp.get(lh.deviation, l), grp.get(lh.speed_ratio, l), uint32_t(grp.get(int(lh.bits), l))}; },
      pose_finite, crit);
  const bool selected = live && (rec.flags & crit.select) != 0;
  const bool leader = live && leg == 0;
  const unsigned long long ballot = __ballot(leader && selected); // bit = lane of a selected robot's first leg
  if (leader) {
    if (restore_map != nullptr) restore_map[rob] = selected ? rob : int64_t(-1);
    if (health != nullptr) {
      strip[2 * gi] = ulonglong2{(unsigned long long)__double_as_longlong(rec.min_limit_proximity), (unsigned long long)__double_as_longlong(rec.max_tip_deviation)};
      strip[2 * gi + 1] = ulonglong2{(unsigned long long)__double_as_longlong(rec.max_speed_ratio), (unsigned long long)rec.flags | ((unsigned long long)rec.leg_masks << 32)};
    }
  }
  if (wave_mask != nullptr && lane == 0) {
    unsigned long long m = 0;
#pragma unroll
    for (int g = 0; g < rpw; ++g) m |= ((ballot >> (g * L)) & 1ull) << g;
    wave_mask[blockIdx.x] = m;
    wave_count[blockIdx.x] = uint32_t(__popcll(m));
  }
  if (health != nullptr) {
    __syncthreads();
    const int64_t rec0 = rob_lo - first;
    if (lane < 2 * n_rob) health[2 * rec0 + lane] = strip[2 * g0 + lane];
  }
}

// Pass 2, once per level: counts[0 .. m) -> their exclusive prefix sums within tiles of kHealthTile entries, in place, and each tile's total to
// totals[tile]; one wavefront per workgroup, four consecutive entries per lane.  The totals of a level are the counts of the next one, until a
// level has one tile: that launch also writes the grand total to *n_selected (when asked for).  No workgroup waits on another: the levels are
// separate launches on the engine's stream.
constexpr int kHealthTile = 256;
__global__ __launch_bounds__(64) void health_scan_counts_kernel(uint32_t *__restrict__ counts, int64_t m, uint32_t *__restrict__ totals,
                                                                int64_t *__restrict__ n_selected) {
  const int lane = threadIdx.x;
  const int64_t i0 = int64_t(blockIdx.x) * kHealthTile + 4 * lane;
  uint32_t c[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k] = i0 + k < m ? counts[i0 + k] : 0u;
    sum += c[k];
  }
  uint32_t incl = sum; // inclusive scan of the lanes' sums
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(incl), off, 64));
    if (lane >= off) incl += o;
  }
  uint32_t run = incl - sum;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < m) counts[i0 + k] = run;
    run += c[k];
  }
  if (lane == 63) {
    totals[blockIdx.x] = incl;
    if (n_selected != nullptr && gridDim.x == 1) *n_selected = int64_t(incl);
  }
}

// Pass 3: the ids of the selected robots, ascending.  Thread t serves group slot t % 32 of wavefront t / 32 (a wavefront holds at most 21 robots):
// the wavefront's offset is the sum of its prefix on every level, a robot's place behind it the number of selected robots before it in the mask.
struct HealthLevels {
  int n;              // levels in use
  int64_t offset[5];  // level k's prefix array starts at counts[offset[k]]; level k has one entry per kHealthTile entries of level k - 1
};
__global__ __launch_bounds__(256) void health_scatter_kernel(int64_t *__restrict__ selected, const unsigned long long *__restrict__ wave_mask,
                                                             const uint32_t *__restrict__ counts, HealthLevels lv, int64_t n_blocks, int64_t wave0, int rpw) {
  const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t b = t >> 5;
  const int g = int(t & 31);
  if (b >= n_blocks || g >= rpw) return;
  const unsigned long long m = wave_mask[b];
  if (!((m >> g) & 1ull)) return;
  int64_t pos = 0, idx = b;
  for (int k = 0; k < lv.n; ++k) {
    pos += counts[lv.offset[k] + idx];
    idx /= kHealthTile;
  }
  pos += __popcll(m & ((1ull << g) - 1ull));
  selected[pos] = (wave0 + b) * rpw + g;
}

// Words of the engine's count buffer for `waves` wavefronts: the masks (8 bytes each) first, then the levels of counts and a last word for the top total
static HealthLevels health_levels(int64_t waves, int64_t *count_words) {
  HealthLevels lv{};
  int64_t off = 0, m = waves;
  for (;;) {
    lv.offset[lv.n++] = off;
    off += m;
    if (m <= kHealthTile) break;
    m = (m + kHealthTile - 1) / kHealthTile;
  }
  *count_words = off + 1; // + the total of the top level
  return lv;
}

extern "C" int shc_engine_scan_health(shc_engine *e, int64_t first, int64_t count, const shc_health_criteria *criteria, shc_robot_health *health,
                                      int64_t *restore_map, int64_t *selected, int64_t *n_selected, int on_device) {
  SHC_ENTER_JOINED(e);
  if (!health && !restore_map && !selected && !n_selected) return fail(SHC_ERR_INVALID_ARG, "health, restore_map, selected and n_selected are all NULL");
  if (first < 0 || count < 0 || first > e->n || count > e->n - first) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  const shc_health_criteria crit = health_criteria(criteria);
  if (crit.reserved != 0) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.reserved must be 0");
  if (crit.select & ~kHealthAllFlags) return fail(SHC_ERR_INVALID_ARG, "shc_health_criteria.select has bits outside SHC_HEALTH_*");
  if (on_device && ((reinterpret_cast<uintptr_t>(health) & 15) ||
                    ((reinterpret_cast<uintptr_t>(restore_map) | reinterpret_cast<uintptr_t>(selected) | reinterpret_cast<uintptr_t>(n_selected)) & 7)))
    return fail(SHC_ERR_INVALID_ARG, "device buffers: health must be 16-byte aligned, the int64 buffers 8-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  const int rpw = 64 / e->L;
  const int64_t n = e->n, end = first + count;
  if (!e->d_health) { // once per engine: masks and counts for a scan of the whole batch (a scan of a range needs no more)
    int64_t words;
    (void)health_levels(e->n_waves, &words);
    HIP_TRY(hipMalloc(&e->d_health, size_t(e->n_waves) * 8 + size_t(words) * 4));
  }
  // host form: the list's length comes back first - it decides how much of `selected` is written
  int64_t n_sel = 0;
  HostCall hc(e);
  ulonglong2 *d_health = reinterpret_cast<ulonglong2 *>(hc.out(health, size_t(count), on_device));
  int64_t *d_map = hc.out(restore_map, size_t(n), on_device);
  int64_t *d_list = selected && !on_device && count ? hc.scratch<int64_t>(size_t(count)) : selected;
  int64_t *d_nsel = on_device ? n_selected : (n_selected || selected) ? hc.out(&n_sel, 1, 0) : nullptr;
  if (const int rc = hc.status()) return rc;
  const bool compact = d_list != nullptr || d_nsel != nullptr;

  int rc = SHC_OK;
  hipError_t err = hipSuccess;
  // restore_map outside the range: -1 is the byte 0xff eight times
  if (d_map && first > 0) err = hipMemsetAsync(d_map, 0xff, size_t(first) * 8, e->stream);
  if (d_map && end < n && err == hipSuccess) err = hipMemsetAsync(d_map + end, 0xff, size_t(n - end) * 8, e->stream);
  if (count == 0) {
    if (d_nsel && err == hipSuccess) err = hipMemsetAsync(d_nsel, 0, 8, e->stream);
  } else if (err == hipSuccess && (rc = derive_tips(e)) == SHC_OK) {
    const int64_t wave0 = first / rpw, grid = row_grid(e->L, first, end);
    unsigned long long *masks = compact ? reinterpret_cast<unsigned long long *>(e->d_health) : nullptr;
    uint32_t *counts = compact ? reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(e->d_health) + size_t(e->n_waves) * 8) : nullptr;
    rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
      constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
      health_scan_kernel<L, NJ><<<dim3((unsigned)grid), dim3(64), 0, e->stream>>>(d_health, d_map, masks, counts, e->st, (const SharedConsts<L, NJ> *)e->d_consts, crit,
                                                                                 first, count);
      return SHC_OK;
    });
    if (rc == SHC_OK) err = hipGetLastError();
    if (rc == SHC_OK && err == hipSuccess && compact) {
      int64_t words;
      const HealthLevels lv = health_levels(grid, &words);
      int64_t m = grid;
      for (int k = 0; k < lv.n && err == hipSuccess; ++k) { // level k's totals are level k + 1's counts (the top level's: the last word)
        const int64_t tiles = (m + kHealthTile - 1) / kHealthTile;
        health_scan_counts_kernel<<<dim3((unsigned)tiles), dim3(64), 0, e->stream>>>(counts + lv.offset[k], m, counts + lv.offset[k] + m, k == lv.n - 1 ? d_nsel : nullptr);
        err = hipGetLastError();
        m = tiles;
      }
      if (d_list && err == hipSuccess) {
        health_scatter_kernel<<<dim3((unsigned)((grid * 32 + 255) / 256)), dim3(256), 0, e->stream>>>(d_list, masks, counts, lv, grid, wave0, rpw);
        err = hipGetLastError();
      }
    }
  }
  if (rc != SHC_OK) return rc;
  if (err != hipSuccess) return fail(SHC_ERR_HIP, std::string("health scan: ") + hipGetErrorString(err));
  if ((rc = hc.finish()) != SHC_OK || on_device) return rc;
  if (selected && n_sel) {
    hc.back(selected, d_list, size_t(n_sel));
    hc.wait_at_finish();
    if ((rc = hc.finish()) != SHC_OK) return rc;
  }
  if (n_selected) *n_selected = n_sel;
  return SHC_OK;
}

// One robot on the host, through leg_health / robot_health: see include/shc_batch.h
extern "C" int shc_debug_robot_health(const shc_params *params, const shc_health_criteria *criteria, const double *q, const double *qd,
                                      const double *poser_tip, const double *model_tip, const double *admittance, const int32_t *leg_status,
                                      const double *pose7, shc_robot_health *out) {
  if (!q || !qd || !poser_tip || !model_tip || !admittance || !leg_status || !pose7 || !out) return fail(SHC_ERR_INVALID_ARG, "NULL argument");
  int L, NJ;
  const int rc = validate_params(params, &L, &NJ);
  if (rc != SHC_OK) return rc;
  const shc_health_criteria crit = health_criteria(criteria);
  if (crit.reserved != 0 || (crit.select & ~kHealthAllFlags)) return fail(SHC_ERR_INVALID_ARG, "criteria: reserved must be 0, select within SHC_HEALTH_*");
  LegHealth legs[SHC_MAX_LEGS];
  dispatch_nj(NJ, [&](auto nj) {
    constexpr int N = decltype(nj)::value;
    for (int l = 0; l < L; ++l) {
      LegConst<N> lc;
      hostinit::fill_leg_const<N>(*params, l, lc);
      double ql[N], qdl[N];
      for (int j = 0; j < N; ++j) ql[j] = q[l * N + j], qdl[j] = qd[l * N + j];
      auto v3 = [&](const double *a) { return V3{a[3 * l], a[3 * l + 1], a[3 * l + 2]}; };
      legs[l] = leg_health<N>(lc, ql, qdl, V3{0.0, 0.0, 0.0}, v3(poser_tip), v3(model_tip), v3(admittance), true, (leg_status[l] & 4) != 0);
    }
    return 0;
  });
  bool pose_finite = true;
  for (int k = 0; k < 7; ++k) pose_finite = pose_finite && health_finite(pose7[k]);
  *out = robot_health(L, [&](int l) { return legs[l]; }, pose_finite, crit);
  return SHC_OK;
}
