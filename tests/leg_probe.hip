// leg_probe.hip — test code, not product: the per-leg kinematics of csrc/shc_leg.hpp (with apply_ik_core of shc_leg_api.hpp and bearing_bracket of
// shc_cycle.hpp) behind a small C interface, so that tests/test_leg_primitives.py and tests/test_gpu_leg_primitives.py can call each function on
// chosen legs and joint states.  Same rules as math_probe.hip: the product headers are included unchanged and this file holds no arithmetic of its
// own - every op below only unpacks doubles, calls the product function and packs the result.
//
// A case carries the raw parameters of one leg as the reference names them (NP = 5 + 7 NJ doubles):
//   base link d, theta, r, alpha | per link d, r, alpha, theta | per joint min, max, max_vel | leg_dof
// and the dynamic inputs of the op.  The parameters go into a shc_params (leg 0) and through the product's own hostinit::fill_leg_const<NJ> on the
// host, so the derived members of LegConst (centres, cost weights, r1 / p1, the padding defaults) are part of what is tested; the kernel reads each
// case's LegConst from global memory into registers.  One case per lane in 64-lane blocks, or a host loop over the same functor.
//
// Built by the tests with engine.compile_with_product_flags (the shipped kernels' flags, so fp-contraction matches).
#include "../syropod_highlevel_controller_amd/csrc/shc_host_init.hpp"

// shc_leg_api.hpp is included by shc_engine.hip behind the engine's two state-plane index helpers; its kernels name them.  Declared only: nothing
// here instantiates a kernel that indexes the engine's planes (apply_ik_core works on registers).
__device__ int64_t rob_index(int64_t r, int f, int rpw, int nf);
__device__ int64_t slot_of(int64_t rob, int leg, int L);
#include "../syropod_highlevel_controller_amd/csrc/shc_leg_api.hpp"

#include <cstring>
#include <vector>

using namespace shc;

namespace {

SHC_HD V3 ld3(const double *p) { return V3{p[0], p[1], p[2]}; }
SHC_HD void st3(double *o, V3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; }
template <int NJ>
SHC_HD void ldn(const double *p, double (&a)[NJ]) {
#pragma unroll
  for (int k = 0; k < NJ; ++k) a[k] = p[k];
}
template <int NJ>
SHC_HD void stn(double *o, const double (&a)[NJ]) {
#pragma unroll
  for (int k = 0; k < NJ; ++k) o[k] = a[k];
}

constexpr int n_params(int nj) { return 5 + 7 * nj; }

template <int NJ>
void params_of(const double *x, shc_params &p) {
  std::memset(&p, 0, sizeof p);
  p.leg_count = 1;
  p.leg_dof[0] = int(x[n_params(NJ) - 1]);
  p.link[0][0] = shc_link_params{x[0], x[1], x[2], x[3]};
  for (int k = 0; k < NJ; ++k) {
    const double *l = x + 4 + 4 * k, *j = x + 4 + 4 * NJ + 3 * k;
    p.link[0][k + 1] = shc_link_params{l[0], l[3], l[1], l[2]}; // (d, r, alpha, theta) -> {d, theta, r, alpha}
    p.joint[0][k] = shc_joint_params{j[0], j[1], 0.0, 0.0, j[2]};
  }
}

// r1 9, p1 3, link_sa NJ, link_ca NJ, jcentre NJ, jw_range NJ, jw_vrange NJ, jactive NJ
template <int NJ>
SHC_HD void pack_leg_const(const LegConst<NJ> &lc, double *o) {
  for (int k = 0; k < 9; ++k) o[k] = lc.r1[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = lc.p1[k];
  stn<NJ>(o + 12, lc.link_sa), stn<NJ>(o + 12 + NJ, lc.link_ca), stn<NJ>(o + 12 + 2 * NJ, lc.jcentre), stn<NJ>(o + 12 + 3 * NJ, lc.jw_range);
  stn<NJ>(o + 12 + 4 * NJ, lc.jw_vrange), stn<NJ>(o + 12 + 5 * NJ, lc.jactive);
}

// ------------------------------------------------------------------------------------------------ the ops (dynamic inputs -> outputs)

template <int NJ>
struct OpFkChain { // q -> z[], p[], pe, xe
  static constexpr int NIN = NJ, NOUT = 6 * NJ + 6;
  static constexpr bool HOST = true;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ];
    ldn<NJ>(in, q);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    for (int k = 0; k < NJ; ++k) st3(out + 3 * k, c.z[k]), st3(out + 3 * NJ + 3 * k, c.p[k]);
    st3(out + 6 * NJ, c.pe), st3(out + 6 * NJ + 3, c.xe);
  }
};

template <int NJ>
struct OpJacobian { // q -> lin[]
  static constexpr int NIN = NJ, NOUT = 3 * NJ;
  static constexpr bool HOST = true;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ];
    ldn<NJ>(in, q);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    V3 lin[NJ];
    jacobian_columns<NJ>(c, lin);
    for (int k = 0; k < NJ; ++k) st3(out + 3 * k, lin[k]);
  }
};

template <int NJ>
struct OpFkTipPose { // q -> position 3, quaternion w x y z
  static constexpr int NIN = NJ, NOUT = 7;
  static constexpr bool HOST = true;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ];
    ldn<NJ>(in, q);
    const Pose t = fk_tip_pose<NJ>(lc, q);
    st3(out, t.p);
    out[3] = t.r.w, out[4] = t.r.x, out[5] = t.r.y, out[6] = t.r.z;
  }
};

template <int NJ, bool EXACT>
struct OpIkStep { // q, qd, desired (robot frame) -> dq
  static constexpr int NIN = 2 * NJ + 3, NOUT = NJ;
  static constexpr bool HOST = EXACT;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], qd[NJ], dq[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, qd);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    ik_step<NJ, EXACT>(lc, c, q, qd, ld3(in + 2 * NJ), dq);
    stn<NJ>(out, dq);
  }
};

template <int NJ, bool EXACT>
struct OpIkStepRotation { // q, qd, rot_delta (joint-1 frame) -> dq
  static constexpr int NIN = 2 * NJ + 3, NOUT = NJ;
  static constexpr bool HOST = EXACT;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], qd[NJ], dq[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, qd);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    V3 lin[NJ];
    jacobian_columns<NJ>(c, lin);
    ik_step_rotation<NJ, EXACT>(lc, c, lin, q, qd, ld3(in + 2 * NJ), dq);
    stn<NJ>(out, dq);
  }
};

template <int NJ, bool EXACT>
struct OpSolveIkDelta { // q, qd, dp, dw, solve_rotation -> dq
  static constexpr int NIN = 2 * NJ + 7, NOUT = NJ;
  static constexpr bool HOST = EXACT;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], qd[NJ], dq[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, qd);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    V3 lin[NJ];
    jacobian_columns<NJ>(c, lin);
    solve_ik_delta<NJ, EXACT>(lc, c, lin, q, qd, ld3(in + 2 * NJ), ld3(in + 2 * NJ + 3), in[2 * NJ + 6] != 0.0, dq);
    stn<NJ>(out, dq);
  }
};

template <int NJ>
struct OpUpdateJoints { // q, qd, dq, dt, 1 / dt (as the callers pass it), clamp_vel, clamp_pos -> q, qd, proximity
  static constexpr int NIN = 3 * NJ + 4, NOUT = 2 * NJ + 1;
  static constexpr bool HOST = true;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], qd[NJ], dq[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, qd), ldn<NJ>(in + 2 * NJ, dq);
    out[2 * NJ] = update_joints<NJ>(lc, dq, in[3 * NJ], in[3 * NJ + 1], in[3 * NJ + 2] != 0.0, in[3 * NJ + 3] != 0.0, q, qd);
    stn<NJ>(out, q), stn<NJ>(out + NJ, qd);
  }
};

template <int NJ>
struct OpTipForce { // q, tau -> raw force (robot frame)
  static constexpr int NIN = 2 * NJ, NOUT = 3;
  static constexpr bool HOST = true;
  SHC_HD static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], tau[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, tau);
    Chain<NJ> c;
    fk_chain<NJ>(lc, q, c);
    st3(out, tip_force_raw<NJ>(lc, c, tau));
  }
};

template <int NJ>
struct OpApplyIk { // q, qd, desired, constrained, desired_dir, clamp_vel, clamp_pos, dt -> q, qd, success, failed, retried, tip (robot frame)
  static constexpr int NIN = 2 * NJ + 10, NOUT = 2 * NJ + 6;
  static constexpr bool HOST = false;
  __device__ static void run(const LegConst<NJ> &lc, const double *in, double *out) {
    double q[NJ], qd[NJ];
    ldn<NJ>(in, q), ldn<NJ>(in + NJ, qd);
    const double *d = in + 2 * NJ;
    Chain<NJ> ch;
    bool retried = false;
    const IkOutcome ik = apply_ik_core<NJ>(
        lc, q, qd, ld3(d), d[3] != 0.0, ld3(d + 4), d[7] != 0.0, d[8] != 0.0, d[9], ch, []() {}, [&](const Chain<NJ> &, bool r) { retried = r; });
    stn<NJ>(out, q), stn<NJ>(out + NJ, qd);
    out[2 * NJ] = ik.success, out[2 * NJ + 1] = ik.failed ? 1.0 : 0.0, out[2 * NJ + 2] = retried ? 1.0 : 0.0;
    st3(out + 2 * NJ + 3, tip_robot_frame(lc, ch.pe));
  }
};

template <int NJ, bool WRITTEN_OUT>
struct OpBearingBracket { // y, x -> sector (the leg is not read)
  static constexpr int NIN = 2, NOUT = 1;
  static constexpr bool HOST = false;
  __device__ static void run(const LegConst<NJ> &, const double *in, double *out) { out[0] = double(bearing_bracket<WRITTEN_OUT>(in[0], in[1])); }
};

template <int NJ> using OpIkStepFast = OpIkStep<NJ, false>;
template <int NJ> using OpIkStepExact = OpIkStep<NJ, true>;
template <int NJ> using OpIkStepRotationFast = OpIkStepRotation<NJ, false>;
template <int NJ> using OpIkStepRotationExact = OpIkStepRotation<NJ, true>;
template <int NJ> using OpSolveIkDeltaFast = OpSolveIkDelta<NJ, false>;
template <int NJ> using OpSolveIkDeltaExact = OpSolveIkDelta<NJ, true>;
template <int NJ> using OpBearingPlain = OpBearingBracket<NJ, false>;
template <int NJ> using OpBearingWrittenOut = OpBearingBracket<NJ, true>;

// ------------------------------------------------------------------------------------------------ running them

template <class Op, int NJ>
__global__ void __launch_bounds__(64) leg_kernel(const LegConst<NJ> *__restrict__ lcs, const double *__restrict__ in, int n, double *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const LegConst<NJ> lc = lcs[i];
  double li[Op::NIN], lo[Op::NOUT];
#pragma unroll
  for (int k = 0; k < Op::NIN; ++k) li[k] = in[size_t(i) * Op::NIN + k];
  Op::run(lc, li, lo);
#pragma unroll
  for (int k = 0; k < Op::NOUT; ++k) out[size_t(i) * Op::NOUT + k] = lo[k];
}

// fill_leg_const in its device form: each lane builds its LegConst from its case's shc_params
template <int NJ>
__global__ void __launch_bounds__(64) leg_const_kernel(const shc_params *__restrict__ ps, int n, double *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  LegConst<NJ> lc;
  hostinit::fill_leg_const<NJ>(ps[i], 0, lc);
  double lo[12 + 6 * NJ];
  pack_leg_const<NJ>(lc, lo);
  for (int k = 0; k < 12 + 6 * NJ; ++k) out[size_t(i) * (12 + 6 * NJ) + k] = lo[k];
}

template <int NJ>
std::vector<LegConst<NJ>> leg_consts(const double *params, int n) {
  std::vector<LegConst<NJ>> lcs(n);
  shc_params p;
  for (int i = 0; i < n; ++i) {
    params_of<NJ>(params + size_t(i) * n_params(NJ), p);
    hostinit::fill_leg_const<NJ>(p, 0, lcs[i]);
  }
  return lcs;
}

template <class Op, int NJ>
int host_run(const double *params, const double *in, int n, double *out) {
  if constexpr (!Op::HOST) {
    return -2; // a device-only form
  } else {
    const std::vector<LegConst<NJ>> lcs = leg_consts<NJ>(params, n);
    for (int i = 0; i < n; ++i) {
      double li[Op::NIN], lo[Op::NOUT];
      for (int k = 0; k < Op::NIN; ++k) li[k] = in[size_t(i) * Op::NIN + k];
      Op::run(lcs[i], li, lo);
      for (int k = 0; k < Op::NOUT; ++k) out[size_t(i) * Op::NOUT + k] = lo[k];
    }
    return 0;
  }
}

// device round trip: consts (a plain array of records) + inputs up, outputs down; 0, or the hipError_t that stopped it
template <class Launch>
int on_device(const void *consts, size_t const_bytes, const double *in, size_t in_doubles, double *out, size_t out_doubles, Launch launch) {
  void *dc = nullptr;
  double *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&dc, const_bytes);
  if (e == hipSuccess) e = hipMalloc(&din, (in_doubles ? in_doubles : 1) * 8);
  if (e == hipSuccess) e = hipMalloc(&dout, out_doubles * 8);
  if (e == hipSuccess) e = hipMemcpy(dc, consts, const_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && in_doubles) e = hipMemcpy(din, in, in_doubles * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xff, out_doubles * 8); // a case nobody wrote reads back as NaN
  if (e == hipSuccess) {
    launch(dc, din, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, out_doubles * 8, hipMemcpyDeviceToHost);
  if (dc) (void)hipFree(dc);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return int(e);
}

template <class Op, int NJ>
int dev_run(const double *params, const double *in, int n, double *out) {
  const std::vector<LegConst<NJ>> lcs = leg_consts<NJ>(params, n);
  return on_device(lcs.data(), lcs.size() * sizeof(LegConst<NJ>), in, size_t(n) * Op::NIN, out, size_t(n) * Op::NOUT, [&](void *dc, double *din, double *dout) {
    hipLaunchKernelGGL((leg_kernel<Op, NJ>), dim3((n + 63) / 64), dim3(64), 0, 0, static_cast<const LegConst<NJ> *>(dc), din, n, dout);
  });
}

template <int NJ>
struct OpLegConst { // no dynamic input -> the derived members of LegConst
  static constexpr int NIN = 0, NOUT = 12 + 6 * NJ;
  static constexpr bool HOST = true;
};
template <int NJ>
int leg_const_host(const double *params, const double *, int n, double *out) {
  const std::vector<LegConst<NJ>> lcs = leg_consts<NJ>(params, n);
  for (int i = 0; i < n; ++i) pack_leg_const<NJ>(lcs[i], out + size_t(i) * OpLegConst<NJ>::NOUT);
  return 0;
}
template <int NJ>
int leg_const_dev(const double *params, const double *, int n, double *out) {
  std::vector<shc_params> ps(n);
  for (int i = 0; i < n; ++i) params_of<NJ>(params + size_t(i) * n_params(NJ), ps[i]);
  return on_device(ps.data(), ps.size() * sizeof(shc_params), nullptr, 0, out, size_t(n) * OpLegConst<NJ>::NOUT, [&](void *dc, double *, double *dout) {
    hipLaunchKernelGGL((leg_const_kernel<NJ>), dim3((n + 63) / 64), dim3(64), 0, 0, static_cast<const shc_params *>(dc), n, dout);
  });
}

typedef int (*RunFn)(const double *, const double *, int, double *);
struct OpEntry {
  const char *name;
  bool host;
  int nin[3], nout[3]; // NJ = 3, 4, 5
  RunFn on_host[3], on_dev[3];
};
#define SHC_LEG_OP(NAME, OP)                                                                                                             \
  {NAME, OP<3>::HOST, {OP<3>::NIN, OP<4>::NIN, OP<5>::NIN}, {OP<3>::NOUT, OP<4>::NOUT, OP<5>::NOUT},                                    \
   {&host_run<OP<3>, 3>, &host_run<OP<4>, 4>, &host_run<OP<5>, 5>}, {&dev_run<OP<3>, 3>, &dev_run<OP<4>, 4>, &dev_run<OP<5>, 5>}}
const OpEntry kOps[] = {
    {"leg_const", true, {0, 0, 0}, {OpLegConst<3>::NOUT, OpLegConst<4>::NOUT, OpLegConst<5>::NOUT},
     {&leg_const_host<3>, &leg_const_host<4>, &leg_const_host<5>}, {&leg_const_dev<3>, &leg_const_dev<4>, &leg_const_dev<5>}},
    SHC_LEG_OP("fk_chain", OpFkChain),
    SHC_LEG_OP("jacobian_columns", OpJacobian),
    SHC_LEG_OP("fk_tip_pose", OpFkTipPose),
    SHC_LEG_OP("ik_step_fast", OpIkStepFast),
    SHC_LEG_OP("ik_step_exact", OpIkStepExact),
    SHC_LEG_OP("ik_step_rotation_fast", OpIkStepRotationFast),
    SHC_LEG_OP("ik_step_rotation_exact", OpIkStepRotationExact),
    SHC_LEG_OP("solve_ik_delta_fast", OpSolveIkDeltaFast),
    SHC_LEG_OP("solve_ik_delta_exact", OpSolveIkDeltaExact),
    SHC_LEG_OP("update_joints", OpUpdateJoints),
    SHC_LEG_OP("tip_force_raw", OpTipForce),
    SHC_LEG_OP("apply_ik", OpApplyIk),
    SHC_LEG_OP("bearing_bracket_plain", OpBearingPlain),
    SHC_LEG_OP("bearing_bracket_written_out", OpBearingWrittenOut),
};
constexpr int kOpCount = int(sizeof(kOps) / sizeof(kOps[0]));

} // namespace

extern "C" {

int shc_leg_probe_op_count() { return kOpCount; }
const char *shc_leg_probe_op_name(int op) { return op >= 0 && op < kOpCount ? kOps[op].name : nullptr; }
// widths of op at NJ = nj: leg parameters, dynamic inputs, outputs (doubles per case); whether the op has a host form
int shc_leg_probe_op_widths(int op, int nj, int *nparams, int *nin, int *nout, int *host) {
  if (op < 0 || op >= kOpCount || nj < 3 || nj > 5) return -1;
  *nparams = n_params(nj), *nin = kOps[op].nin[nj - 3], *nout = kOps[op].nout[nj - 3], *host = kOps[op].host ? 1 : 0;
  return 0;
}
// params: n * nparams doubles, in: n * nin, out: n * nout.  0 on success, -1 for a bad argument, -2 for the host form of a device-only op,
// otherwise the hipError_t.
int shc_leg_probe_run(int op, int nj, const double *params, const double *in, int n, double *out, int device) {
  if (op < 0 || op >= kOpCount || nj < 3 || nj > 5 || n < 0 || !params || !in || !out) return -1;
  if (n == 0) return 0;
  for (int i = 0; i < n; ++i) { // the leg the kernels index by: 3 <= leg_dof <= NJ
    const double dof = params[size_t(i) * n_params(nj) + n_params(nj) - 1];
    if (!(dof >= 3 && dof <= nj)) return -1;
  }
  const OpEntry &e = kOps[op];
  return device ? e.on_dev[nj - 3](params, in, n, out) : e.on_host[nj - 3](params, in, n, out);
}

} // extern "C"
