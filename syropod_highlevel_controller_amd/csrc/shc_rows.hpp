// shc_rows.hpp — the row pattern of the dense-tensor device passes, written once: the block geometry (RowGroup), the LDS tile and its mover, and
// on the host the resolved spec (RowLayout, row_layout, row_column), the head of the kernel arguments (RowArgs), the launch sizes and the host
// forms.  Included by shc_engine.hip before the passes that use it: the record passes (shc_leg_msgs.hpp, shc_frames.hpp, shc_health.hpp) take
// the geometry (health_scan_kernel as the same lines written out) and the grid, the tensor passes (shc_observe.hpp, shc_actions.hpp,
// shc_footholds.hpp) all of it.  The fleet forms' shared part is fleet_rows_begin / fleet_rows_each of shc_fleet_io.hpp.
#pragma once

// ---- device side
// Geometry.  One leg per lane, floor(64 / L) robots per wavefront (the cycle's slot mapping: every plane read is contiguous across the
// wavefront), one wavefront per workgroup.  Block b serves the robot group w = first / rpw + b, clipped to [first, end): lane (gi, leg) is
// robot `rob` and `live` inside the range; groups [g0, g0 + n_rob) hold the robots rob_lo .. of this block; `slot` is the lane's leg slot.
template <int L>
struct RowGroup {
  static constexpr int rpw = 64 / L;
  int lane, gi, leg, g0, n_rob;
  int64_t w, rob, rob_lo, slot;
  bool live;
  __device__ __forceinline__ RowGroup(int64_t first, int64_t end) {
    lane = threadIdx.x;
    w = first / rpw + blockIdx.x;
    gi = lane / L, leg = lane - gi * L;
    rob = w * rpw + gi;
    live = gi < rpw && rob >= first && rob < end;
    rob_lo = w * rpw > first ? w * rpw : first;
    const int64_t rob_hi = (w + 1) * rpw < end ? (w + 1) * rpw : end;
    g0 = int(rob_lo - w * rpw), n_rob = int(rob_hi - rob_lo);
    slot = w * 64 + lane;
  }
};

// The tile.  A robot's row is contiguous in the caller's array, but its columns belong to different lanes (leg l of a per-leg field at
// l * width + k).  The wavefront therefore moves its rows through LDS - rpw rows of `pitch` elements of T - and crosses global memory with
// consecutive lanes on consecutive elements of a row: the lanes run through the block's rows one after the other, so a 64-lane access covers
// 64 consecutive elements of one row or the end of one and the start of the next (two contiguous runs - the seam), and its LDS side hits
// consecutive banks, conflict-free but for the seam.  Rows are at rows[row * row_stride]: row = ids[robot] (the caller's instance id of a
// fleet part's robot) or robot - row0.
// The lanes' own accesses are ds_read / ds_write_b32 / _b64: banks are (address / 4) mod 32, per 32 (b32) or 16 (b64) contiguous lanes.  Within
// a robot the lanes are 1, 3 or dof elements apart, robots `pitch` elements: pitch is width | 1, odd, so that for 4-byte elements the robots of
// a lane group start on distinct banks and the 3-column fields of a hexapod's legs (0, 3, .. 15) interleave with them - 2-way at most, which
// a store does not pay for and a read replays once; 8-byte elements use the even banks only and can meet 2- to 4-way.
// One dynamic LDS array serves every pass, as the element type of the launch.
extern __shared__ double2 row_tile_lds[];
template <class T>
__device__ __forceinline__ T *row_tile() {
  return reinterpret_cast<T *>(row_tile_lds);
}
// Element e = lane, lane + 64, .. of the block's n_rob x width elements: move(index in the caller's array, index in the tile); (r, c) follow by
// addition - 64 = dq * width + dr
template <int L, class A, class Move>
__device__ __forceinline__ void row_tile_walk(const RowGroup<L> &g, const A &a, const int64_t *__restrict__ ids, int64_t row0, Move &&move) {
  const int total = g.n_rob * a.width, dq = 64 / a.width, dr = 64 - dq * a.width;
  int r = g.lane / a.width, c = g.lane - r * a.width;
  for (int e = g.lane; e < total; e += 64) {
    const int64_t rr = g.rob_lo + r;
    const int64_t row = ids ? ids[rr] : rr - row0;
    move(row * a.row_stride + c, (g.g0 + r) * a.pitch + c);
    r += dq, c += dr;
    if (c >= a.width) c -= a.width, ++r;
  }
}
// copy-in: all `width` columns, those of legs or joints the morphology lacks included (they stay in the tile)
template <int L, class T, class A>
__device__ __forceinline__ void row_tile_in(T *tile, const T *__restrict__ in, const RowGroup<L> &g, const A &a, const int64_t *__restrict__ ids, int64_t row0) {
  row_tile_walk(g, a, ids, row0, [&](int64_t at, int t) { tile[t] = in[at]; });
}
template <int L, class T, class A>
__device__ __forceinline__ void row_tile_out(T *__restrict__ out, const T *tile, const RowGroup<L> &g, const A &a, const int64_t *__restrict__ ids, int64_t row0) {
  row_tile_walk(g, a, ids, row0, [&](int64_t at, int t) { out[at] = tile[t]; });
}
// With has_pad (the row has columns of legs / joints the morphology lacks) the tile is filled with `pad` first, so the columns no lane owns are defined
template <int L, class T, class A>
__device__ __forceinline__ void row_tile_pad(T *tile, const RowGroup<L> &g, const A &a) {
  if (a.has_pad) {
    const T pad = static_cast<T>(a.pad);
    for (int c = g.lane; c < g.rpw * a.pitch; c += 64) tile[c] = pad;
    __syncthreads();
  }
}

// ---- host side
// A spec resolved: the first column of every field (-1: not selected), the selected fields as a mask, the columns of a row.
constexpr int kRowMaxFields = 32; // the selected fields are one 32-bit mask
struct RowLayout {
  int32_t col[kRowMaxFields];
  uint32_t mask;
  int64_t width;
};
// nullptr when the spec is valid on its own (no engine asked yet), else what is wrong with it: a whole sentence, or from '.' on one that the
// struct's name opens (row_resolve puts it there - nothing is built or allocated for a valid spec).  P describes the struct: Spec; name;
// most_fields and n_fields_why - the bound of n_fields and the complaint about it; fields; has_dof; width(field, dof) - columns per leg
// (per_leg(field)) or per robot; own(spec) - the complaint about members only this struct has.
// (a spec without dof may scale field widths by a member of its own: P::scale(spec), which P::width then receives in place of dof)
template <class P, class = void>
struct RowScale {
  static int of(const typename P::Spec *) { return 0; }
};
template <class P>
struct RowScale<P, std::void_t<decltype(&P::scale)>> {
  static int of(const typename P::Spec *s) { return P::scale(s); }
};
template <class P>
static const char *row_layout(const typename P::Spec *s, RowLayout &lay) {
  if (!s) return "spec is NULL";
  if (s->n_fields < 1 || s->n_fields > P::most_fields) return P::n_fields_why;
  if (s->dtype != SHC_OBS_F64 && s->dtype != SHC_OBS_F32) return ".dtype is neither SHC_OBS_F64 nor SHC_OBS_F32";
  if (const char *why = P::own(s)) return why;
  if (s->reserved != 0) return ".reserved must be 0";
  int dof = 0;
  if constexpr (P::has_dof) {
    dof = s->dof;
    if (s->legs < 1 || s->legs > SHC_MAX_LEGS || dof < 1 || dof > SHC_MAX_JOINTS) return ".legs / dof outside 1 .. SHC_MAX_LEGS / SHC_MAX_JOINTS";
  } else {
    if (s->legs < 1 || s->legs > SHC_MAX_LEGS) return ".legs outside 1 .. SHC_MAX_LEGS";
    dof = RowScale<P>::of(s);
  }
  for (int f = 0; f < kRowMaxFields; ++f) lay.col[f] = -1;
  lay.mask = 0, lay.width = 0;
  for (int i = 0; i < s->n_fields; ++i) {
    const int f = s->fields[i];
    if (f < 0 || f >= P::fields) return ".fields names an unknown field";
    if (lay.mask & (1u << f)) return ".fields names a field twice";
    lay.mask |= 1u << f;
    lay.col[f] = int32_t(lay.width);
    lay.width += P::width(f, dof) * (P::per_leg(f) ? s->legs : 1);
  }
  if (s->row_stride != 0 && s->row_stride < lay.width) return ".row_stride is below the width of a row";
  return nullptr;
}
// SHC_OK, or the complaint of row_layout as the last error
template <class P>
static int row_resolve(const typename P::Spec *spec, RowLayout &lay) {
  const char *why = row_layout<P>(spec, lay);
  if (!why) return SHC_OK;
  return fail(SHC_ERR_INVALID_ARG, why[0] == '.' ? std::string(P::name) + why : std::string(why));
}
// shc_*_width and shc_*_column
template <class P>
static int64_t row_width(const typename P::Spec *spec) {
  RowLayout lay;
  if (const int bad = row_resolve<P>(spec, lay)) return -int64_t(bad);
  return lay.width;
}
template <class P>
static int row_column(const typename P::Spec *spec, int field, int leg, int k) {
  RowLayout lay;
  if (row_layout<P>(spec, lay) || field < 0 || field >= P::fields || lay.col[field] < 0) return -1;
  int dof = RowScale<P>::of(spec);
  if constexpr (P::has_dof) dof = spec->dof;
  const int w = P::width(field, dof);
  if (k < 0 || k >= w) return -1;
  if (!P::per_leg(field)) return lay.col[field] + k;
  if (leg < 0 || leg >= spec->legs) return -1;
  return lay.col[field] + leg * w + k;
}

static size_t row_element_bytes(int dtype) { return dtype == SHC_OBS_F32 ? 4 : 8; }
template <class Spec>
static int64_t row_stride_of(const Spec *spec, const RowLayout &lay) {
  return spec->row_stride ? spec->row_stride : lay.width;
}
static int row_aligned(const void *rows, int dtype, const char *name) {
  if (reinterpret_cast<uintptr_t>(rows) & (row_element_bytes(dtype) - 1)) return fail(SHC_ERR_INVALID_ARG, std::string(name) + " must be aligned to its element size");
  return SHC_OK;
}

// The head of a kernel's view of a spec (launch-uniform: scalar loads of the kernel arguments); what a pass adds stands behind it.  has_pad and
// pad serve the copy-out kernels (observe, footholds_get): the copy-in kernels (actions, footholds_set) carry them unread and never load them.
template <int N>
struct RowArgs {
  uint32_t mask;
  int32_t col[N];
  int32_t width, pitch; // columns of a row; elements between the rows of the LDS tile
  int32_t has_pad;      // the row has columns of legs / joints the morphology lacks
  int64_t row_stride;
  double pad;           // already rounded to the element type
};
template <int N>
static void row_args(RowArgs<N> &a, const RowLayout &lay, int dtype, int64_t row_stride, bool has_pad, double pad) {
  a.mask = lay.mask;
  for (int f = 0; f < N; ++f) a.col[f] = lay.col[f];
  a.width = int32_t(lay.width), a.pitch = int32_t(lay.width) | 1;
  a.has_pad = has_pad;
  a.row_stride = row_stride;
  a.pad = dtype == SHC_OBS_F32 ? double(static_cast<float>(pad)) : pad;
}
// The launch: one block per robot group that [first, end) touches, and the tile of a block
static unsigned row_grid(int legs, int64_t first, int64_t end) {
  const int rpw = 64 / legs;
  return (unsigned)((end - 1) / rpw - first / rpw + 1);
}
static size_t row_tile_bytes(int legs, int pitch, int dtype) { return size_t(64 / legs) * pitch * row_element_bytes(dtype); }

// The host forms.  Dense device rows in: the columns [0, width) of every row of the caller's array as dense rows on the device - with `word`, a
// zeroed 8-byte word behind them, which is read back after the pass - then pass(rows, word) on the engine's stream, and a wait.
template <class Pass>
static int rows_from_host(shc_engine *e, const void *rows, int64_t n, int64_t width, int64_t stride, int dtype, int64_t *word, Pass &&pass) {
  const size_t es = row_element_bytes(dtype);
  HostCall hc(e);
  const char *d = hc.in2d(rows, size_t(width) * es, size_t(stride) * es, size_t(n));
  int64_t *d_word = hc.out(word, 1, 0);
  int rc = hc.status();
  if (rc != SHC_OK) return rc;
  if (word) HIP_TRY(hipMemsetAsync(d_word, 0, 8, e->stream));
  if ((rc = pass(d, d_word)) != SHC_OK) return rc;
  return hc.finish();
}
// Dense device rows out: pass(rows) on the engine's stream, then the columns [0, width) of every row of the caller's array, and a wait
template <class Pass>
static int rows_to_host(shc_engine *e, void *rows, int64_t n, int64_t width, int64_t stride, int dtype, Pass &&pass) {
  const size_t es = row_element_bytes(dtype);
  HostCall hc(e);
  char *d = hc.out2d(rows, size_t(width) * es, size_t(stride) * es, size_t(n));
  int rc = hc.status();
  if (rc != SHC_OK || (rc = pass(d)) != SHC_OK) return rc;
  return hc.finish();
}
