// math_probe.hip — test code, not product: the device math primitives of shc_math.hpp / shc_leg.hpp / shc_cycle.hpp behind a
// small C interface, so that tests/test_math_primitives.py and tests/test_gpu_math_primitives.py can call each of them on chosen
// inputs.  The product headers are included unchanged; this file holds no arithmetic of its own - every op below only unpacks
// doubles, calls the product function and packs the result.
//
// Every op is one functor with a host + device run(in, out).  It is executed either by a host loop (the x86 half of the same
// source) or by a kernel with one case per lane in 64-lane blocks.  The two lane-grouped forms run one case per Group<L> in the
// cycle kernel's own group layout (shc_cycle_kernel.hpp: grp = lane / L, leg = lane - grp * L, tail lanes and groups past the
// end mirror a live group) and store, per lane, the grouped result next to the scalar result of the same lane.
//
// Built by the tests with engine.compile_with_product_flags (the shipped kernels' flags, so fp-contraction matches).
#include "../syropod_highlevel_controller_amd/csrc/shc_cycle.hpp"

#include <cstring>

using namespace shc;

namespace {

SHC_HD V3 ld3(const double *p) { return V3{p[0], p[1], p[2]}; }
SHC_HD Quat ldq(const double *p) { return Quat{p[0], p[1], p[2], p[3]}; }
SHC_HD Pose ldpose(const double *p) { return Pose{ld3(p), ldq(p + 3)}; }
SHC_HD void st3(double *o, V3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; }
SHC_HD void stq(double *o, Quat q) { o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z; }
SHC_HD void stpose(double *o, const Pose &p) { st3(o, p.p), stq(o + 3, p.r); }

template <int N, bool EXACT>
SHC_HD void run_spd(const double *in, double *out) {
  double a[N][N], b[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) a[i][j] = in[i * N + j];
    b[i] = in[N * N + i];
  }
  spd_solve<N, EXACT>(a, b);
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = b[i];
}

// name, doubles in, doubles out, body (in / out are register arrays of exactly those widths; integers travel as doubles)
#define SHC_PROBE_OPS(X)                                                                                                        \
  X(sincos_joint_reduce, 1, 2, sincos_joint<true>(in[0], &out[0], &out[1]))                                                     \
  X(sincos_joint_noreduce, 1, 2, sincos_joint<false>(in[0], &out[0], &out[1]))                                                  \
  X(euler_to_quat_extrinsic, 3, 4, stq(out, euler_to_quat(ld3(in), false)))                                                     \
  X(euler_to_quat_intrinsic, 3, 4, stq(out, euler_to_quat(ld3(in), true)))                                                      \
  X(quat_to_euler_extrinsic, 4, 3, st3(out, quat_to_euler(ldq(in), false)))                                                     \
  X(quat_to_euler_intrinsic, 4, 3, st3(out, quat_to_euler(ldq(in), true)))                                                      \
  X(from_two_vectors, 6, 4, stq(out, from_two_vectors(ld3(in), ld3(in + 3))))                                                   \
  X(quat_from_matrix, 9, 4, double m[9]; for (int i = 0; i < 9; ++i) m[i] = in[i]; stq(out, quat_from_matrix(m)))               \
  X(angle_axis_vector, 4, 3, st3(out, angle_axis_vector(ldq(in))))                                                              \
  X(slerp, 9, 4, stq(out, slerp(ldq(in), in[4], ldq(in + 5))))                                                                  \
  X(normalized_v3, 3, 3, st3(out, normalized(ld3(in))))                                                                         \
  X(normalized_quat, 4, 4, stq(out, normalized(ldq(in))))                                                                       \
  X(inverse, 4, 4, stq(out, inverse(ldq(in))))                                                                                  \
  X(rotate, 7, 3, st3(out, rotate(ldq(in), ld3(in + 4))))                                                                       \
  X(correct_rotation, 8, 4, stq(out, correct_rotation(ldq(in), ldq(in + 4))))                                                   \
  X(add_pose, 14, 7, stpose(out, add_pose(ldpose(in), ldpose(in + 7))))                                                         \
  X(remove_pose, 14, 7, stpose(out, remove_pose(ldpose(in), ldpose(in + 7))))                                                   \
  X(interpolate_pose, 15, 7, stpose(out, interpolate_pose(ldpose(in), in[7], ldpose(in + 8))))                                  \
  X(inverse_transform_vector, 10, 3, st3(out, inverse_transform_vector(ldpose(in), ld3(in + 7))))                               \
  X(projection, 6, 3, st3(out, projection(ld3(in), ld3(in + 3))))                                                               \
  X(rejection, 6, 3, st3(out, rejection(ld3(in), ld3(in + 3))))                                                                 \
  X(smooth_step, 1, 1, out[0] = smooth_step(in[0]))                                                                             \
  X(round_to_int, 1, 1, out[0] = double(round_to_int(in[0])))                                                                   \
  X(round_to_even_int, 1, 1, out[0] = double(round_to_even_int(in[0])))                                                         \
  X(mod_i, 2, 1, out[0] = double(mod_i(int(in[0]), int(in[1]))))                                                                \
  X(signd, 1, 1, out[0] = signd(in[0]))                                                                                         \
  X(clampd, 3, 1, out[0] = clampd(in[0], in[1], in[2]))                                                                         \
  X(quartic_bezier, 16, 3, V3 p[5]; for (int i = 0; i < 5; ++i) p[i] = ld3(in + 3 * i); st3(out, quartic_bezier(p, in[15])))    \
  X(quartic_bezier_dot, 16, 3, st3(out, quartic_bezier_dot(ld3(in), ld3(in + 3), ld3(in + 6), ld3(in + 9), ld3(in + 12), in[15]))) \
  X(fast_rcp, 1, 1, out[0] = fast_rcp<false>(in[0]))                                                                            \
  X(fast_rsqrt, 1, 1, out[0] = fast_rsqrt<false>(in[0]))                                                                        \
  X(spd_solve3_fast, 12, 3, (run_spd<3, false>(in, out)))                                                                       \
  X(spd_solve4_fast, 20, 4, (run_spd<4, false>(in, out)))                                                                       \
  X(spd_solve5_fast, 30, 5, (run_spd<5, false>(in, out)))                                                                       \
  X(spd_solve6_fast, 42, 6, (run_spd<6, false>(in, out)))                                                                       \
  X(spd_solve3_exact, 12, 3, (run_spd<3, true>(in, out)))                                                                       \
  X(spd_solve4_exact, 20, 4, (run_spd<4, true>(in, out)))                                                                       \
  X(spd_solve5_exact, 30, 5, (run_spd<5, true>(in, out)))                                                                       \
  X(spd_solve6_exact, 42, 6, (run_spd<6, true>(in, out)))                                                                       \
  X(tip_rotation_delta, 6, 3, st3(out, tip_rotation_delta(ld3(in), ld3(in + 3))))

#define X(NAME, NI, NO, BODY)                                  \
  struct Op_##NAME {                                           \
    static constexpr int NIN = NI, NOUT = NO;                  \
    SHC_HD static void run(const double *in, double *out) {    \
      BODY;                                                    \
    }                                                          \
  };
SHC_PROBE_OPS(X)
#undef X

// one case per lane, 64-lane blocks; the case is copied into registers first so that the functor sees no global pointers
template <class Op>
__global__ void __launch_bounds__(64) probe_kernel(const double *__restrict__ in, int n, double *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double li[Op::NIN], lo[Op::NOUT];
#pragma unroll
  for (int k = 0; k < Op::NIN; ++k) li[k] = in[size_t(i) * Op::NIN + k];
  Op::run(li, lo);
#pragma unroll
  for (int k = 0; k < Op::NOUT; ++k) out[size_t(i) * Op::NOUT + k] = lo[k];
}

template <class Op>
void host_loop(const double *in, int n, double *out) {
  for (int i = 0; i < n; ++i) {
    double li[Op::NIN], lo[Op::NOUT];
    for (int k = 0; k < Op::NIN; ++k) li[k] = in[size_t(i) * Op::NIN + k];
    Op::run(li, lo);
    for (int k = 0; k < Op::NOUT; ++k) out[size_t(i) * Op::NOUT + k] = lo[k];
  }
}

// The grouped forms.  WHICH 0: quat_to_euler_zyx_grouped (4 in; per lane 3 grouped + 3 scalar out),
//                     WHICH 1: euler_to_quat_zyx_grouped (3 in; per lane 4 grouped + 4 scalar out).
// Case c lives in wave c / RPW, group c % RPW; lane `leg` of it writes out[(c * L + leg) * NOUT ...].
template <int L, int WHICH>
__global__ void __launch_bounds__(64) grouped_kernel(const double *__restrict__ in, int n, double *__restrict__ out) {
  constexpr int RPW = 64 / L, NIN = WHICH == 0 ? 4 : 3, NRES = WHICH == 0 ? 3 : 4;
  const int lane = threadIdx.x;
  const int left = n - int(blockIdx.x) * RPW;
  const int here = left < RPW ? (left < 0 ? 0 : left) : RPW;
  if (here == 0) return; // wave-uniform
  int grp = lane / L;
  const int leg = lane - grp * L;
  const bool live = grp < here;
  if (!live) grp = here - 1; // mirror lanes: every shuffle stays well defined, they never store
  const int c = int(blockIdx.x) * RPW + grp;
  double li[NIN], res[2 * NRES];
#pragma unroll
  for (int k = 0; k < NIN; ++k) li[k] = in[size_t(c) * NIN + k];
  const Group<L> g{grp * L};
  if (WHICH == 0) {
    st3(res, quat_to_euler_zyx_grouped<L>(ldq(li), g, leg));
    st3(res + NRES, quat_to_euler(ldq(li), false));
  } else {
    stq(res, euler_to_quat_zyx_grouped<L>(ld3(li), g, leg));
    stq(res + NRES, euler_to_quat(ld3(li), false));
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < 2 * NRES; ++k) out[(size_t(c) * L + leg) * (2 * NRES) + k] = res[k];
  }
}

struct OpEntry {
  const char *name;
  int nin, nout;
  void (*host)(const double *, int, double *);
  void (*launch)(const double *, int, double *);
};
template <class Op>
void launch_op(const double *in, int n, double *out) {
  hipLaunchKernelGGL(probe_kernel<Op>, dim3((n + 63) / 64), dim3(64), 0, 0, in, n, out);
}
#define X(NAME, NI, NO, BODY) {#NAME, NI, NO, &host_loop<Op_##NAME>, &launch_op<Op_##NAME>},
const OpEntry kOps[] = {SHC_PROBE_OPS(X)};
#undef X
constexpr int kOpCount = int(sizeof(kOps) / sizeof(kOps[0]));

// device round trip shared by both entry points: 0, or the hipError_t that stopped it
template <class Launch>
int on_device(const double *in, size_t in_doubles, double *out, size_t out_doubles, Launch launch) {
  double *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, in_doubles * 8);
  if (e == hipSuccess) e = hipMalloc(&dout, out_doubles * 8);
  if (e == hipSuccess) e = hipMemcpy(din, in, in_doubles * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xff, out_doubles * 8); // a case nobody wrote reads back as NaN
  if (e == hipSuccess) {
    launch(din, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, out_doubles * 8, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return int(e);
}

template <int WHICH>
void launch_grouped(int L, const double *in, int n, double *out) {
  const auto go = [&](auto kernel, int l) { hipLaunchKernelGGL(kernel, dim3((n + 64 / l - 1) / (64 / l)), dim3(64), 0, 0, in, n, out); };
  switch (L) {
  case 3: go(grouped_kernel<3, WHICH>, 3); break;
  case 4: go(grouped_kernel<4, WHICH>, 4); break;
  case 5: go(grouped_kernel<5, WHICH>, 5); break;
  case 6: go(grouped_kernel<6, WHICH>, 6); break;
  case 7: go(grouped_kernel<7, WHICH>, 7); break;
  case 8: go(grouped_kernel<8, WHICH>, 8); break;
  }
}

} // namespace

extern "C" {

int shc_probe_op_count() { return kOpCount; }
const char *shc_probe_op_name(int op) { return op >= 0 && op < kOpCount ? kOps[op].name : nullptr; }
int shc_probe_op_widths(int op, int *nin, int *nout) {
  if (op < 0 || op >= kOpCount) return -1;
  *nin = kOps[op].nin, *nout = kOps[op].nout;
  return 0;
}

// in: n * nin doubles, out: n * nout doubles.  0 on success, -1 for a bad argument, otherwise the hipError_t.
int shc_probe_run(int op, const double *in, int n, double *out, int device) {
  if (op < 0 || op >= kOpCount || n < 0 || !in || !out) return -1;
  if (n == 0) return 0;
  const OpEntry &e = kOps[op];
  if (!device) {
    e.host(in, n, out);
    return 0;
  }
  return on_device(in, size_t(n) * e.nin, out, size_t(n) * e.nout, [&](const double *di, double *dout) { e.launch(di, n, dout); });
}

// which 0: quat_to_euler (in n * 4, out n * L * 6), which 1: euler_to_quat (in n * 3, out n * L * 8); L = 3 ... 8; device only.
int shc_probe_run_grouped(int which, int L, const double *in, int n, double *out) {
  if ((which != 0 && which != 1) || L < 3 || L > 8 || n < 0 || !in || !out) return -1;
  if (n == 0) return 0;
  const int nin = which == 0 ? 4 : 3, nout = which == 0 ? 6 : 8;
  return on_device(in, size_t(n) * nin, out, size_t(n) * L * nout, [&](const double *di, double *dout) {
    if (which == 0) launch_grouped<0>(L, di, n, dout);
    else launch_grouped<1>(L, di, n, dout);
  });
}

} // extern "C"
