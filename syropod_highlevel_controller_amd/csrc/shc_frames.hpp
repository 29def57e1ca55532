// shc_frames.hpp — StateController::publishFrameTransforms (state_controller.cpp:963-1047) for a range of instances in one device pass:
// shc_engine_get_frame_transforms.  Included by shc_engine.hip (uses its rob_index, load_leg_fields of shc_leg_msgs.hpp and the
// entry-point macros).
//
// The arithmetic of the payload lives in two host + device functions, leg_frames (every joint frame and the tip frame of one leg in one
// pass down its chain) and body_frames (the per-robot record); frame_transforms_kernel calls them and a host path may too.
#pragma once

#include <cstddef>

constexpr int kFrameJoints = SHC_FRAME_JOINTS;
constexpr int kLegFrameDoubles = 7 * kFrameJoints + 7, kBodyFrameDoubles = 20;
static_assert(sizeof(shc_leg_frames) == kLegFrameDoubles * 8, "shc_leg_frames is 42 doubles without padding");
static_assert(sizeof(shc_body_frames) == kBodyFrameDoubles * 8, "shc_body_frames is 20 doubles without padding");
static_assert(offsetof(shc_leg_frames, tip) == 7 * kFrameJoints * 8, "the tip follows the joint frames");
static_assert(kLegFrameDoubles % 2 == 0 && kBodyFrameDoubles % 2 == 0, "records are written in 16-byte chunks");

SHC_HD void put_pose(double *o, const Pose &p) {
  o[0] = p.p.x, o[1] = p.p.y, o[2] = p.p.z;
  o[3] = p.r.w, o[4] = p.r.x, o[5] = p.r.y, o[6] = p.r.z;
}

// Pose::Identity().transform(T1 * [X Y Z | P]) (pose.h:135-146): position T1 * P, rotation (Quaterniond(R1 * [X Y Z]) * identity).normalized()
template <class LC>
SHC_HD Pose chain_frame_pose(const LC &lc, const double (&X)[3], const double (&Y)[3], const double (&Z)[3], const double (&P)[3]) {
  double m[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    m[i * 3 + 0] = lc.r1[i * 3] * X[0] + lc.r1[i * 3 + 1] * X[1] + lc.r1[i * 3 + 2] * X[2];
    m[i * 3 + 1] = lc.r1[i * 3] * Y[0] + lc.r1[i * 3 + 1] * Y[1] + lc.r1[i * 3 + 2] * Y[2];
    m[i * 3 + 2] = lc.r1[i * 3] * Z[0] + lc.r1[i * 3 + 1] * Z[1] + lc.r1[i * 3 + 2] * Z[2];
  }
  return Pose{tip_robot_frame(lc, V3{P[0], P[1], P[2]}), normalized(quat_from_matrix(m))};
}

// The children of base_link one leg contributes (state_controller.cpp:1009-1046), rec = shc_leg_frames as 42 doubles.  One pass down the
// chain: the running frame (X, Y, Z, P) of fk_tip_pose IS joint k's frame before link k is applied (Joint::getTransformFromJoint, model.h:
// 594-599: the product of the DH matrices of the links before the joint, the base link first), and the tip's after the last link.
//   joint k: position = that frame's origin; rotation = its quaternion * AngleAxisd(q_k, UnitZ) (:1023-1024)
//   tip:     Tip::getPoseRobotFrame (:1034) - the value fk_tip_pose returns
// The slots of joints the leg does not have (LegConst::jactive = 0: identity links behind its tip) stay zero, and the tip is its own.
template <int NJ, class LC>
SHC_HD void leg_frames(const LC &lc, const double (&q)[NJ], double (&rec)[kLegFrameDoubles]) {
  static_assert(NJ <= kFrameJoints, "shc_leg_frames has room for SHC_FRAME_JOINTS joints");
#pragma unroll
  for (int k = 0; k < kLegFrameDoubles; ++k) rec[k] = 0.0;
  double X[3] = {1, 0, 0}, Y[3] = {0, 1, 0}, Z[3] = {0, 0, 1}, P[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const Pose f = chain_frame_pose(lc, X, Y, Z, P);
    double sh, ch;
    sincos_joint(0.5 * q[k], &sh, &ch);
    const Pose jf{f.p, f.r * Quat{ch, 0.0, 0.0, sh}};
    if (lc.jactive[k] != 0.0) put_pose(&rec[7 * k], jf);
    double s, co;
    sincos_joint(lc.link_th[k] + q[k], &s, &co);
    const double sa = lc.link_sa[k], ca = lc.link_ca[k], r = lc.link_r[k], d = lc.link_d[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) { // the DH step of fk_tip_pose
      const double xn = X[a] * co + Y[a] * s, t = Y[a] * co - X[a] * s;
      const double yn = t * ca + Z[a] * sa, zn = Z[a] * ca - t * sa;
      P[a] = P[a] + xn * r + Z[a] * d;
      X[a] = xn, Y[a] = yn, Z[a] = zn;
    }
  }
  put_pose(&rec[7 * kFrameJoints], chain_frame_pose(lc, X, Y, Z, P));
}

// odom_to_base_link.addPose(child) (pose.h:167-173) of every frame of a leg record that is in use: SHC_FRAME_ODOM_IDEAL
SHC_HD void leg_frames_to_world(const Pose &odom_to_base_link, double (&rec)[kLegFrameDoubles]) {
#pragma unroll
  for (int k = 0; k <= kFrameJoints; ++k) {
    double *o = &rec[7 * k];
    const Quat r{o[3], o[4], o[5], o[6]};
    if (r.w == 0.0 && r.x == 0.0 && r.y == 0.0 && r.z == 0.0) continue; // a joint slot the leg does not have
    put_pose(o, add_pose(odom_to_base_link, Pose{V3{o[0], o[1], o[2]}, r}));
  }
}

// The per-robot record, rec = shc_body_frames as 20 doubles; returns odom_to_base_link.
//   odom_to_base_link       = getOdometryIdeal().addPose(getCurrentPose())      (state_controller.cpp:965-967, :984-990)
//   base_link_to_walk_plane = ~getCurrentPose()                                 (:995-1005; pose.h:112-115)
//   pose_euler              = quaternionToEulerAngles(current_pose.rotation_)   (:919-921)
//   desired_velocity        = (vx, vy, omega)                                   (:900-905)
// (the members the observation pass evaluates on their own - shc_observe.hpp - are functions of their own)
SHC_HD Pose body_odom_to_base_link(const Pose &odometry, const Pose &current) { return add_pose(odometry, current); }
SHC_HD V3 body_pose_euler(const Pose &current) { return quat_to_euler(current.r, false); }
SHC_HD Pose body_frames(const Pose &odometry, const Pose &current, V3 velocity, double (&rec)[kBodyFrameDoubles]) {
  const Pose o2b = body_odom_to_base_link(odometry, current);
  put_pose(&rec[0], o2b);
  const Quat rc = conj(current.r);
  put_pose(&rec[7], Pose{rotate(rc, -current.p), rc});
  const V3 e = body_pose_euler(current);
  rec[14] = e.x, rec[15] = e.y, rec[16] = e.z;
  rec[17] = velocity.x, rec[18] = velocity.y, rec[19] = velocity.z;
  return o2b;
}

// ---- the batched form
// The robot-level inputs of body_frames out of the wavefront's robot tile (frame_transforms_kernel, observe_kernel)
__device__ __forceinline__ Pose frames_current_pose(const DevState &st, int64_t rob, int rpw) {
  using R = RobotFields;
  auto rd = [&](int f) { return st.robd[rob_index(rob, f, rpw, R::COUNT)]; };
  return Pose{V3{rd(R::CPOSE), rd(R::CPOSE + 1), rd(R::CPOSE + 2)}, Quat{rd(R::CPOSE + 3), rd(R::CPOSE + 4), rd(R::CPOSE + 5), rd(R::CPOSE + 6)}};
}
__device__ __forceinline__ Pose frames_odometry(const DevState &st, int64_t rob, int rpw, int have_odom) {
  using R = RobotFields;
  auto rd = [&](int f) { return st.robd[rob_index(rob, f, rpw, R::COUNT)]; };
  if (!have_odom) return pose_identity();
  return Pose{V3{rd(R::ODOM), rd(R::ODOM + 1), 0.0}, Quat{rd(R::ODOM + 2), 0.0, 0.0, rd(R::ODOM + 3)}}; // stored as x, y, qw, qz
}
__device__ __forceinline__ V3 frames_desired_velocity(const DevState &st, int64_t rob, int rpw) {
  using R = RobotFields;
  return V3{st.robd[rob_index(rob, R::VLIN, rpw, R::COUNT)], st.robd[rob_index(rob, R::VLIN + 1, rpw, R::COUNT)], st.robd[rob_index(rob, R::VANG, rpw, R::COUNT)]};
}
// The geometry of shc_rows.hpp (RowGroup) for [first, first + count); the joint-angle planes are read as contiguous double2 per lane.
//
// Output: a lane's leg record is 336 B = 21 chunks of 16 B.  The lanes write their records into LDS at a stride of 336 B (84 dwords = 20 mod
// 32 banks, an odd multiple of 4: the eight contiguous lanes a ds_write_b128 serves per LDS cycle start on banks {0, 20, 8, 28, 16, 4, 24, 12}
// and cover all 32 once - no conflict).  The records of a wavefront are consecutive in `legs_out` (consecutive instances, consecutive
// legs), so the staged block and the output block are the same bytes: the wavefront copies it linearly, chunk c by lane c mod 64 - every
// ds_read_b128 group reads 16 distinct 16-byte slots of 256 consecutive bytes (no conflict on the 64-bank rule) and every global store is
// 64 x 16 B contiguous.  21 KiB per wavefront: 7 wavefronts per CU.  The body records (160 B, written by each group's first lane) go
// through the same block afterwards: a wavefront's robots are consecutive in `body_out` too.
template <int L, int NJ>
__global__ __launch_bounds__(64) void frame_transforms_kernel(double2 *__restrict__ legs_out, double2 *__restrict__ body_out, DevState st,
                                                              const SharedConsts<L, NJ> *__restrict__ gc, int world, int have_odom, int64_t first,
                                                              int64_t count) {
  using FD = Fields<NJ>;
  constexpr int rpw = 64 / L;
  constexpr int kLegChunks = kLegFrameDoubles / 2, kBodyChunks = kBodyFrameDoubles / 2;
  __shared__ double2 strip[64 * kLegChunks];
  const RowGroup<L> rg(first, first + count);
  const int lane = rg.lane, gi = rg.gi, leg = rg.leg, g0 = rg.g0, n_rob = rg.n_rob;
  const int64_t rob = rg.rob;
  // lanes [lane0, lane0 + n_rec) hold the leg records legs_out[rec0 ..] of this block, groups [g0, g0 + n_rob) the body records
  const int lane0 = g0 * L, n_rec = n_rob * L;
  const int64_t rec0 = (rg.rob_lo - first) * L, brec0 = rg.rob_lo - first;

  double rec[kLegFrameDoubles], brec[kBodyFrameDoubles];
#pragma unroll
  for (int k = 0; k < kLegFrameDoubles; ++k) rec[k] = 0.0;
#pragma unroll
  for (int k = 0; k < kBodyFrameDoubles; ++k) brec[k] = 0.0;
  if (rg.live) {
    Pose o2b = pose_identity();
    if (body_out != nullptr || world) { // every lane of a robot's group forms the robot's record for itself, as the cycle does
      o2b = body_frames(frames_odometry(st, rob, rpw, have_odom), frames_current_pose(st, rob, rpw), frames_desired_velocity(st, rob, rpw), brec);
    }
    if (legs_out != nullptr) {
      double q[NJ]; // Joint::desired_position_: the chain applyFK() left behind
      load_leg_fields<FD::Q, NJ>(reinterpret_cast<const double2 *>(st.legd), st.n_slots, rg.slot, q);
      leg_frames<NJ>(gc->leg[leg], q, rec);
      if (world) leg_frames_to_world(o2b, rec);
    }
  }
  if (legs_out != nullptr) {
#pragma unroll
    for (int k = 0; k < kLegChunks; ++k) strip[lane * kLegChunks + k] = double2{rec[2 * k], rec[2 * k + 1]};
    __syncthreads();
    for (int c = lane; c < n_rec * kLegChunks; c += 64) legs_out[rec0 * kLegChunks + c] = strip[lane0 * kLegChunks + c];
  }
  if (body_out != nullptr) {
    if (legs_out != nullptr) __syncthreads(); // the leg records have been read out of the block
    if (leg == 0 && gi < rpw) {
#pragma unroll
      for (int k = 0; k < kBodyChunks; ++k) strip[gi * kBodyChunks + k] = double2{brec[2 * k], brec[2 * k + 1]};
    }
    __syncthreads();
    for (int c = lane; c < n_rob * kBodyChunks; c += 64) body_out[brec0 * kBodyChunks + c] = strip[g0 * kBodyChunks + c];
  }
}

extern "C" int shc_engine_get_frame_transforms(shc_engine *e, int64_t first, int64_t count, int frame, shc_leg_frames *legs, shc_body_frames *body,
                                               int on_device) {
  SHC_ENTER_JOINED(e);
  if (!legs && !body) return fail(SHC_ERR_INVALID_ARG, "legs and body are both NULL");
  if (frame != SHC_FRAME_BASE_LINK && frame != SHC_FRAME_ODOM_IDEAL) return fail(SHC_ERR_INVALID_ARG, "unknown frame");
  if (first < 0 || count < 0 || first > e->n || count > e->n - first) return fail(SHC_ERR_INVALID_ARG, "instance range out of bounds");
  if (on_device && ((reinterpret_cast<uintptr_t>(legs) | reinterpret_cast<uintptr_t>(body)) & 15))
    return fail(SHC_ERR_INVALID_ARG, "device buffers must be 16-byte aligned");
  const int world = frame == SHC_FRAME_ODOM_IDEAL;
  if (!e->cp.odometry && (body || world)) return fail(SHC_ERR_UNSUPPORTED, "SHC_FEAT_ODOMETRY is off: odom_to_base_link needs the ideal odometry");
  if (count == 0) return SHC_OK;
  HIP_TRY(hipSetDevice(e->device));
  HostCall hc(e);
  shc_leg_frames *d_legs = legs;
  shc_body_frames *d_body = body;
  if (!on_device) { // one device block for both outputs (a leg record is a multiple of 16 bytes): neither fits the arena of a large batch, and one temporary will do
    const size_t n_legs = legs ? size_t(count) * e->L : 0;
    char *d = hc.scratch<char>(n_legs * sizeof(shc_leg_frames) + (body ? size_t(count) * sizeof(shc_body_frames) : 0));
    if (const int rc = hc.status()) return rc;
    d_legs = legs ? reinterpret_cast<shc_leg_frames *>(d) : nullptr, d_body = body ? reinterpret_cast<shc_body_frames *>(d + n_legs * sizeof(shc_leg_frames)) : nullptr;
    hc.back(legs, d_legs, n_legs), hc.back(body, d_body, size_t(count));
  }
  const unsigned grid = row_grid(e->L, first, first + count);
  const int rc = dispatch_morphology(e, [&](auto l, auto nj) -> int {
    constexpr int L = decltype(l)::value, NJ = decltype(nj)::value;
    frame_transforms_kernel<L, NJ><<<dim3(grid), dim3(64), 0, e->stream>>>(reinterpret_cast<double2 *>(d_legs), reinterpret_cast<double2 *>(d_body), e->st, (const SharedConsts<L, NJ> *)e->d_consts, world,
                                                                          e->cp.odometry ? 1 : 0, first, count);
    return SHC_OK;
  });
  return rc != SHC_OK ? rc : hc.finish();
}
