/*
 * shc_step_plan.h - the step plan pass of libshc_batch.so: part of the C ABI of shc_batch.h, which includes this file (either may be included
 * first).  Everything here uses the handles, SHC_OBS_F64 / SHC_OBS_F32, the error codes and the row rules declared there.
 */
#ifndef SHC_STEP_PLAN_H
#define SHC_STEP_PLAN_H
#include "shc_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Step plan pass: what every LegStepper is doing with its target - the three quartic Bezier curves, stride vector, swing clearance, default and
 * target tip, and the tip path of the rest of the running swing or stance period - as one dense [rows][D] array in one device pass.  It closes the
 * planner's read side (footholds in, reach probe, step plan out): these are the getters DebugVisualiser reads (getSwing1ControlNode,
 * getSwing2ControlNode, getStanceControlNode, getStrideVector, getDefaultTipPose, getTargetTipPose, getSwingClearance, getWalkPlane:
 * debug_visualiser.cpp:136-166, 236-310, 312-365, 499-530), and PATH is what a swing-clearance check against terrain needs.  The engine does not
 * store the control nodes - the cycle regenerates them in registers - so the pass regenerates them from the stored state by the cycle's arithmetic.
 * ROW.  The rule of the observation pass: fields in the order of `fields`; a per-leg field of `width` columns takes legs x width columns, leg-major
 * (leg l, component k at l * width + k); a per-robot field takes its width.  Widths: 15 for the three node fields (node i, component k at 3 i + k),
 * 3 for the vectors, 1 for the two counters, 3 H for SHC_PLAN_PATH (sample h = 1 .. H, component k at 3 (h - 1) + k).  `pad`, converted to the
 * element type once on the host, is written where the robot has no such leg and wherever the definition says "pad"; columns [width, row_stride)
 * are untouched.  Every position is in the frame of SHC_OBS_WALKER_TIP.  Values are unchanged for SHC_OBS_F64, static_cast<float> for SHC_OBS_F32.
 * DEFINITION.  The pass is a function of the stored state - what shc_engine_get_state returns, the external-target records of rough terrain mode,
 * parameters and tables - and equals the reference's members as the last cycle left them, provided no setter, gait change or parameter
 * adjustment has run since that cycle.  All line numbers are walk_controller.cpp's.
 * updateWalk runs updateTipPosition (:637) BEFORE iteratePhase (:639), so the stored phase and step state are one iteration past what the last
 * updateTipPosition saw.  What it saw follows from the stored record, with `period` etc. the step cycle's members:
 *   phase   = mod(stored phase - 1, period)
 *   ran     = walk_state != STOPPED, the leg is WALKING, step_state != FORCE_STOP, and the last cycle was not the STOPPED -> STARTING cycle, which
 *             returns before the steppers (:545) and leaves walk_state == STARTING, !at_correct_phase and stored phase == the leg's phase offset
 *   swing   = ran, swing_start <= phase < swing_end, and not (walk_state == STARTING and !at_correct_phase): such a leg is held in FORCE_STANCE
 *             (:585-592) until its phase reaches swing_end
 *   stance  = ran and not swing (STANCE and FORCE_STANCE take the same branch, :1149)
 * (walk_state != STOPPED and WALKING is the cycle's `stepping` predicate; a leg with ran false has no curves.)
 * SHC_PLAN_DEFAULT_TIP, _TARGET_TIP, _STRIDE_VECTOR are the stored members, always defined.  SHC_PLAN_WALK_PLANE / _NORMAL are
 * shc_instance_state.stepper_walk_plane / stepper_walk_plane_normal.
 * SHC_PLAN_SWING_CLEARANCE is swing_height x normalized(stepper walk plane normal) (:944; on the exact normal (0, 0, 1) the normalisation is
 * skipped, as in the cycle); for a swing leg in rough terrain mode with a defined external target, normalized(that) x the target's own
 * clearance (:1071).  Always defined.
 * Period quantities are those of updateTipPosition (:1025-1041): standard_stance_period = swing || completed_first_step; modified_stance_start =
 * standard ? stance_start : phase offset; modified_stance_period; swing_iterations (rounded to even) and swing_delta_t = 1 / (swing_iterations
 * / 2); stance_iterations = int((modified_stance_period / period) / (frequency x time_delta)) and stance_delta_t = 1 / stance_iterations.
 * Swing leg: ITERATION = phase - swing_start + 1 (:1050), ITERATIONS = swing_iterations.  SWING_1_NODES and SWING_2_NODES are
 * generatePrimarySwingControlNodes and generateSecondarySwingControlNodes(ground_contact && !first_half) (:1238-1291), first_half = ITERATION <=
 * swing_iterations / 2, followed with force_normal_touchdown and no ground contact by forceNormalTouchdown (:1314-1329), from the stored swing
 * origin, origin velocity, target and stride and the clearance above; ground_contact = rough terrain mode and the stored step plane defined
 * (:1110).  In the ground-contact second half the reference builds the secondary nodes from the tip BEFORE that cycle's update (:1285-1289):
 * that tip is walker_tip - walker_tip_velocity x time_delta.  STANCE_NODES are pad (the reference's are stale there).
 * Stance leg: ITERATION = mod(phase + period - modified_stance_start, period) + 1 (:1153), ITERATIONS = stance_iterations.  STANCE_NODES are
 * generateStanceControlNodes(stride_scaler) (:1167, :1295-1310) from the stored stance origin and stride; both swing curves are pad.
 * Every other leg: the three curves, ITERATION, ITERATIONS and PATH are pad.
 * SHC_PLAN_PATH is the walker tip after h further cycles if the curves stayed exactly as they are now: p_0 = the stored walker tip and, for
 * h = 1 .. H with j = ITERATION + h, while j <= ITERATIONS: p_h = p_(h-1) + delta_t x quarticBezierDot(curve_j, t_j), with curve_j, t_j and
 * delta_t as :1121-1130 choose them for a swing (primary curve and t = swing_delta_t x j for j <= swing_iterations / 2, else the secondary
 * curve and t = swing_delta_t x (j - swing_iterations / 2)) and :1172-1173 for a stance (t = j x stance_delta_t).  Samples with j > ITERATIONS are
 * pad: the pass does not guess across a period boundary.  At constant commanded velocity on a fixed walk plane the curves do stay, and sample h
 * is the walker tip h cycles on.
 * ARITHMETIC.  The cycle's operation order and the functions of shc_math.hpp (the same quartic_bezier_dot, every product of the node formulas
 * rounded on its own).
 * NOTHING IS WRITTEN into an engine: state records and auxiliary blobs stay byte for byte what they were.
 * CALLS.  on_device, stream ordering, the join of split steps, count = 0 (a no-op), the host form on_device = 0 and the fleet form - one kernel
 * per part on the part's stream through the part's caller ids, no staging, shc_fleet_io_bytes unchanged - are those of
 * shc_engine_get_observations / shc_fleet_get_observations_device (shc_batch.h).  A row too wide for the passes' LDS tile (only specs with legs above the
 * robot's own) is served by further launches of the same kernel, each for a run of whole fields.
 * REFUSALS.  Those of the observation pass (SHC_ERR_INVALID_ARG: NULL handle, spec or out; n_fields outside 1 .. SHC_PLAN_FIELD_COUNT; an
 * unknown or repeated field; an unknown dtype; reserved != 0; legs below the engine's or the fleet's shape or above SHC_MAX_LEGS; row_stride
 * non-zero and below the width; a range outside [0, n); a buffer not aligned to the element size.  SHC_ERR_BUSY: resident mode.
 * SHC_ERR_UNSUPPORTED: a fleet that spans devices), and SHC_ERR_INVALID_ARG for horizon outside 0 .. 16 and for horizon 0 with SHC_PLAN_PATH named.
 */
enum { /* per-leg fields, leg-major, for `legs` legs */
  SHC_PLAN_SWING_1_NODES,   /* 15: node i component k at 3 i + k   (LegStepper::getSwing1ControlNode)  */
  SHC_PLAN_SWING_2_NODES,   /* 15                                   (getSwing2ControlNode)              */
  SHC_PLAN_STANCE_NODES,    /* 15                                   (getStanceControlNode)              */
  SHC_PLAN_DEFAULT_TIP,     /* 3: default_tip_pose_.position_                                            */
  SHC_PLAN_TARGET_TIP,      /* 3: target_tip_pose_.position_                                             */
  SHC_PLAN_STRIDE_VECTOR,   /* 3: stride_vector_                                                         */
  SHC_PLAN_SWING_CLEARANCE, /* 3: swing_clearance_                                                       */
  SHC_PLAN_ITERATION,       /* 1: iteration of the running period, as updateTipPosition counts it        */
  SHC_PLAN_ITERATIONS,      /* 1: iterations of that period                                              */
  SHC_PLAN_PATH,            /* 3 H: sample h = 1 .. H, component k at 3 (h - 1) + k                      */
  /* per-robot fields */
  SHC_PLAN_WALK_PLANE,        /* 3: the stepping LegSteppers' copy (shc_instance_state.stepper_walk_plane) */
  SHC_PLAN_WALK_PLANE_NORMAL, /* 3: ... stepper_walk_plane_normal                                          */
  SHC_PLAN_FIELD_COUNT
};
#define SHC_PLAN_MAX_HORIZON 16
typedef struct shc_plan_spec {       /* 88 bytes */
  int32_t n_fields, fields[SHC_PLAN_FIELD_COUNT]; /* column order = this order; a field may appear once                 */
  int32_t dtype;                                /* SHC_OBS_F64 / SHC_OBS_F32                                           */
  int32_t legs;                                 /* row geometry; engine: >= its legs; fleet: >= shc_fleet_shape's legs */
  int32_t horizon;                              /* H: 0 .. 16; >= 1 when SHC_PLAN_PATH is named, ignored otherwise     */
  int32_t reserved;                             /* 0 */
  int64_t row_stride;                           /* elements between rows; 0 = dense (= shc_plan_width)                 */
  double pad;                                   /* written where a robot has no such leg and where the definition says pad */
} shc_plan_spec;
int64_t shc_plan_width(const shc_plan_spec *spec);                        /* columns of a row; < 0 for an invalid spec; no device needed */
int shc_plan_column(const shc_plan_spec *spec, int field, int leg, int k); /* column of component k of `field` (leg ignored for robot fields); -1 if absent */
int shc_engine_get_step_plan(shc_engine *e, int64_t first, int64_t count, const shc_plan_spec *spec, void *out, int on_device);
int shc_fleet_get_step_plan_device(shc_fleet *f, const shc_plan_spec *spec, void *out /* [n][row_stride], caller's order */);

#ifdef __cplusplus
}
#endif
#endif /* SHC_STEP_PLAN_H */
