/*
 * shc_batch.h — C ABI of the MI355X batched leg-control engine (libshc_batch.so).
 *
 * The reference (csiro-robotics/syropod_highlevel_controller, OpenSHC v0.5.11) has NO plugin / FFI
 * boundary: it is one executable whose per-cycle work is the C++ call sequence
 *     PoseController::updateCurrentPose   (src/state_controller.cpp:167)
 *     AdmittanceController::updateStiffness / updateAdmittance   (:177, :179)
 *     WalkController::updateWalk          (:429)
 *     PoseController::updateStance        (:442)
 *     Model::updateModel                  (:445)
 * on ONE robot.  This header is the boundary a maintainer would bind instead: the same
 * quantities, batched over `n_instances` independent robots, plain pointers and sizes only.
 * Each entry point cites the reference interface it replaces.
 *
 * All floating point is IEEE double (the reference is `double` throughout).  All arrays passed
 * through this ABI are HOST or DEVICE pointers as stated per call; layouts are instance-major
 * ("AoS over instances"): element (i, leg, k) of an array with per-leg width K lives at
 * [(i * leg_count + leg) * K + k].  Internally the engine keeps structure-of-arrays state in HBM
 *  and transposes at this boundary.
 */
#ifndef SHC_BATCH_H
#define SHC_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHC_MAX_LEGS 8      /* reference bound: parameters_and_states.h:298 (joint_parameters[8][6]) */
#define SHC_MAX_JOINTS 6    /* reference bound: parameters_and_states.h:298 */
#define SHC_MAX_LINKS 7     /* reference bound: parameters_and_states.h:299 (base link + one per joint) */
#define SHC_MAX_AUTO_POSERS 8
#define SHC_N_BEARINGS 9    /* 0..360 step 45 (model.h:22 BEARING_STEP) */

/* Status codes (the reference has no error returns: ROS_FATAL + shutdown). */
enum {
  SHC_OK = 0,
  SHC_ERR_INVALID_ARG = 1,
  SHC_ERR_NO_DEVICE = 2,      /* no HIP device / kernel image: the product path never falls back to CPU */
  SHC_ERR_HIP = 3,
  SHC_ERR_UNSUPPORTED = 4,    /* outside the accelerated path: gravity_aligned_tips on a robot whose legs differ in DOF, sequences with
                                 own-clock auto posing, resident mode for a batch that does not fit the chip */
  SHC_ERR_UNSTABLE = 5,       /* reserved: the reference aborts when the IMU correction's norm exceeds 100 rad
                                 (pose_controller.cpp:1228-1232); after its own clamps (:1222-1226) that needs
                                 max_rotation > 100 rad, so no entry point returns this code today */
  SHC_ERR_BUSY = 6,           /* the engine is in resident mode (shc_engine_resident_begin): only the shc_engine_resident_*
                                 calls, shc_engine_instances and shc_engine_get_tables are valid until shc_engine_resident_end */
  SHC_ERR_TIMEOUT = 7         /* a bounded wait ran out (resident mode: the device loop stopped by itself or did not answer) */
};

/* parameters_and_states.h:99 */
enum { SHC_WALK_STARTING = 0, SHC_WALK_MOVING = 1, SHC_WALK_STOPPING = 2, SHC_WALK_STOPPED = 3 };
/* parameters_and_states.h:111 */
enum { SHC_STEP_SWING = 0, SHC_STEP_STANCE = 1, SHC_STEP_FORCE_STANCE = 2, SHC_STEP_FORCE_STOP = 3 };
/* parameters_and_states.h:123 */
enum { SHC_POSING = 0, SHC_STOP_POSING = 1, SHC_POSING_COMPLETE = 2 };
/* parameters_and_states.h:150 PoseResetMode */
enum {
  SHC_NO_RESET = 0, SHC_Z_AND_YAW_RESET = 1, SHC_X_AND_Y_RESET = 2, SHC_PITCH_AND_ROLL_RESET = 3,
  SHC_ALL_RESET = 4, SHC_IMMEDIATE_ALL_RESET = 5
};
enum { SHC_VEL_THROTTLE = 0, SHC_VEL_REAL = 1 }; /* default.yaml:89 velocity_input_mode */

/* One joint: config/default.yaml:31 "<LEG>_<joint>_joint_parameters" (model.cpp:1032-1036). */
typedef struct shc_joint_params {
  double min, max, offset, unpacked, max_vel;
} shc_joint_params;

/* One link: config/default.yaml:51 "<LEG>_<link>_link_parameters" (model.cpp:998-1001). */
typedef struct shc_link_params {
  double d, theta, r, alpha;
} shc_link_params;

/*
 * The subset of `struct Parameters` (parameters_and_states.h:271-381) + gait.yaml + auto_pose.yaml
 * that the accelerated path reads.  One morphology + one gait for the whole batch (mixed
 * batches = several engines / bins).
 */
typedef struct shc_params {
  /* control parameters (default.yaml:9-15) */
  double time_delta;
  int32_t manual_posing, auto_posing, rough_terrain_mode, admittance_control, inclination_posing, imu_posing;
  /* model (default.yaml:25-78) */
  int32_t leg_count;
  int32_t leg_dof[SHC_MAX_LEGS];   /* 3..5 per leg; legs may differ: joint arrays of the ABI are then [legs][longest leg's DOF], a shorter leg's
                                      extra entries read 0 and are ignored on input (the engine pads it behind its tip with locked joints) */
  shc_joint_params joint[SHC_MAX_LEGS][SHC_MAX_JOINTS];
  shc_link_params link[SHC_MAX_LEGS][SHC_MAX_LINKS]; /* link[l][0] = base link */
  int32_t clamp_joint_positions, clamp_joint_velocities;
  /* walker (default.yaml:82-106) */
  double body_clearance, step_frequency, swing_height, swing_width, step_depth, stance_span_modifier;
  double touchdown_threshold, liftoff_threshold; /* default.yaml:107-108 (rough_terrain_mode: Leg::touchdownDetection, model.cpp:712) */
  int32_t velocity_input_mode;
  double stance_position[SHC_MAX_LEGS][2];
  int32_t overlapping_walkspaces, force_normal_touchdown, gravity_aligned_tips;
  int32_t leg_manipulation_mode; /* default.yaml:120: SHC_MANIPULATION_TIP_CONTROL / _JOINT_CONTROL (WalkController::updateManual) */
  /* poser (default.yaml:110-118) */
  double time_to_start;
  double rotation_pid_gains[3];  /* p, i, d */
  double max_translation[3];     /* x, y, z */
  double max_rotation[3];        /* roll, pitch, yaw */
  double max_translation_velocity, max_rotation_velocity;
  /* admittance (default.yaml:122-130) */
  int32_t dynamic_stiffness, use_joint_effort;
  double integrator_step_time, virtual_mass, virtual_stiffness, virtual_damping_ratio, force_gain;
  double load_stiffness_scaler, swing_stiffness_scaler;
  /* gait (gait.yaml) */
  int32_t stance_phase, swing_phase, phase_offset;
  int32_t offset_multiplier[SHC_MAX_LEGS];
  /* auto pose (auto_pose.yaml) */
  double pose_frequency;
  int32_t pose_phase_length;
  int32_t n_auto_posers;
  int32_t pose_phase_starts[SHC_MAX_AUTO_POSERS], pose_phase_ends[SHC_MAX_AUTO_POSERS];
  int32_t pose_negation_phase_starts[SHC_MAX_LEGS], pose_negation_phase_ends[SHC_MAX_LEGS];
  double negation_transition_ratio[SHC_MAX_LEGS];
  double roll_amplitudes[SHC_MAX_AUTO_POSERS], pitch_amplitudes[SHC_MAX_AUTO_POSERS],
      yaw_amplitudes[SHC_MAX_AUTO_POSERS];
  double x_amplitudes[SHC_MAX_AUTO_POSERS], y_amplitudes[SHC_MAX_AUTO_POSERS], z_amplitudes[SHC_MAX_AUTO_POSERS],
      gravity_amplitudes[SHC_MAX_AUTO_POSERS];
} shc_params;

/* walk_controller.h:23-33 StepCycle */
typedef struct shc_step_cycle {
  double frequency;
  int32_t period, swing_period, stance_period, stance_end, swing_start, swing_end, stance_start;
} shc_step_cycle;

/*
 * Per-(morphology, gait) tables produced once by the init chain
 * (state_controller.cpp:263-272: directStartup -> updateDefaultConfiguration ->
 *  Model::generateWorkspaces -> WalkController::generateWalkspace -> generateLimits)
 * and consumed every cycle by WalkController::getLimit (walk_controller.cpp:414).
 */
typedef struct shc_tables {
  shc_step_cycle step;
  int32_t phase_offset[SHC_MAX_LEGS];                      /* walk_controller.cpp:277 */
  double default_joint_position[SHC_MAX_LEGS][SHC_MAX_JOINTS]; /* model.cpp:593 after direct start-up */
  double walkspace[SHC_N_BEARINGS];                        /* walk_controller.cpp:57 */
  double max_linear_speed[SHC_N_BEARINGS];                 /* walk_controller.cpp:344-359 */
  double max_angular_speed[SHC_N_BEARINGS];
  double max_linear_acceleration[SHC_N_BEARINGS];
  double max_angular_acceleration[SHC_N_BEARINGS];
  double workspace_radius[SHC_MAX_LEGS][SHC_N_BEARINGS];   /* model.cpp:309 (simple workspace, plane z = 0) */
  int32_t pose_phase_length, pose_normaliser;              /* pose_controller.cpp:62-63 */
  int32_t auto_pose_reference_leg;                         /* pose_controller.cpp:75-78 */
} shc_tables;

typedef struct shc_engine shc_engine; /* opaque */

/* Feature bits of the fused cycle kernel (compile-time specialisations are picked from these). */
enum {
  SHC_FEAT_TIP_FORCE = 1 << 0, /* Leg::calculateTipForce every cycle (model.cpp:938); needs joint_effort input */
  SHC_FEAT_ODOMETRY = 1 << 1,  /* WalkController::odometry_ideal_ integration (walk_controller.cpp:643, :783-791) */
  /* Diagnostic: run the runtime-flag kernel (every feature compiled in, selected per launch) even where a compile-time
   * specialisation for the parameter set exists.  Both produce identical bits (tests/test_gpu_parity.py). */
  SHC_FEAT_GENERIC_KERNEL = 1 << 30,
  /* Diagnostic: resident mode with ONE wavefront per robot group even where the batch is small enough for the two-wavefront
   * (walker / model) pipeline.  Both produce identical bits (tests/test_gpu_resident.py). */
  SHC_FEAT_RESIDENT_ONE_WAVE = 1 << 29,
  /* Diagnostic: launch every step as ONE kernel on the engine's stream even for batches large enough for the two-stream split
   * (see shc_engine_step).  Both produce identical bits. */
  SHC_FEAT_SINGLE_STREAM = 1 << 28,
  /* Diagnostic: shc_engine_step_k runs its K cycles as K single launches (row k through the setters, one shc_engine_step, q / qd into slot k of the
   * output ring) even where the configuration has a batch kernel - the form every configuration WITHOUT one takes (manual-leg kernels; the
   * runtime-flag families unless the library was built with SHC_GENERIC_LOOP_FORMS=1).  Both produce identical bits (tests/test_gpu_step_k.py). */
  SHC_FEAT_STEP_K_SERIAL = 1 << 27,
  SHC_FEAT_ALL = 0x07ffffff
};

/*
 * Library/device introspection.  shc_device_count() returns the number of visible HIP devices
 * (0 when none; never an error) so a caller can fail loudly before creating an engine.
 */
int shc_abi_version(void); /* 6: shc_engine_adjust_parameter (the nine run-time adjustable parameters); 5: shc_engine_step_k / shc_engine_get_step_k_joint_state (K cycles per launch, each with its own inputs); 4: shc_cycle_inputs.direct + shc_engine_resident_bind_inputs (launch-free posts); 3: resident mode, join, auxiliary state */
/* sizeof(shc_params) / sizeof(shc_tables) as compiled into the library: lets a foreign-language binding check its layout */
int64_t shc_sizeof_params(void);
int64_t shc_sizeof_tables(void);
int shc_device_count(void);
const char *shc_last_error(void);
/* Diagnostics: `reps` launches of a plain plane copy (16-byte loads and stores per lane, the cycle kernel's access shape) of
 * `n_doubles` (even) doubles; the known byte count calibrates rocprofv3's FETCH_SIZE / WRITE_SIZE (MI355X_MICROARCH.md, HBM). */
int shc_debug_plane_copy(int device, int64_t n_doubles, int reps);

/*
 * The same init chain for `count` morphologies at once, ON THE GPU: one thread per
 * (morphology, leg) runs the direct start-up solve and the workspace search (thousands of sequential DLS steps each,
 * model.cpp:309-510, pose_controller.cpp:463-517), one thread per morphology the walkspace and limits
 * (walk_controller.cpp:57-361).  params / out are host arrays; status[i] (may be NULL) receives SHC_OK or the reason
 * morphology i was rejected (its tables are zeroed).  Results match shc_generate_tables up to FP contraction.
 */
int shc_generate_tables_batch(const shc_params *params, int64_t count, shc_tables *out, int32_t *status, int device);
/* shc_engine_create with tables computed beforehand (shc_generate_tables / _batch) instead of running the init chain. */
int shc_engine_create_with_tables(const shc_params *params, const shc_tables *tables, int64_t n_instances, int device,
                                  void *stream, shc_engine **out);

/* HIP stream helpers for hosts without their own HIP binding (the ctypes tests, a cgo / JNI host): a non-blocking
 * stream on `device` to pass to shc_engine_create / shc_engine_set_stream.  Engines of different morphology bins run
 * concurrently when each has its own stream (BASELINE.json configs[4]). */
int shc_stream_create(int device, void **stream);
int shc_stream_destroy(int device, void *stream);

/*
 * Host-side init chain = StateController::init + initModel + direct start-up + workspace /
 * walkspace / limit generation (state_controller.cpp:127-153, 263-272).  Pure host function
 * (no device needed); fills `out`.  Product code (shares the device math headers), NOT the oracle.
 */
int shc_generate_tables(const shc_params *params, shc_tables *out);

/*
 * Create an engine for `n_instances` robots on HIP device `device` (replaces
 * StateController::StateController + init(), state_controller.cpp:13-153, for a batch).
 * Every instance starts in the post-start-up RUNNING state: joints at the default
 * configuration, walk state STOPPED.  `stream` is a hipStream_t (0 = default stream).
 */
int shc_engine_create(const shc_params *params, int64_t n_instances, int device, void *stream, shc_engine **out);
int shc_engine_destroy(shc_engine *e);
int shc_engine_set_stream(shc_engine *e, void *stream);
int shc_engine_set_features(shc_engine *e, uint32_t features);
int shc_engine_get_tables(const shc_engine *e, shc_tables *out);
int64_t shc_engine_instances(const shc_engine *e);

/*
 * Inputs that arrive between cycles in the reference (ROS callbacks, state_controller.cpp).
 * `on_device` != 0: pointers are device pointers in the same layouts (no host round trip).
 * NULL pointer = leave that input unchanged.
 */
/* StateController::bodyVelocityInputCallback (state_controller.cpp:1127): lin [n][2], ang [n]. */
int shc_engine_set_velocity(shc_engine *e, const double *linear_xy, const double *angular, int on_device);
/* imuCallback -> Model::setImuData (state_controller.cpp:1552, model.h:146): quat [n][4] (w,x,y,z), gyro [n][3]. */
int shc_engine_set_imu(shc_engine *e, const double *orientation_wxyz, const double *angular_velocity, int on_device);
/* tipStatesCallback -> Leg::setTipForceMeasured (state_controller.cpp:1618): [n][legs][3]. */
int shc_engine_set_tip_force(shc_engine *e, const double *tip_force, int on_device);
/* jointStatesCallback -> Joint::current_effort_ (state_controller.cpp:1590): [n][legs][dof].
 * Until the first effort arrives Leg::calculateTipForce filters zero torques into a zero state (model.cpp:680-707), so the
 * engine runs the kernels without the estimate; the FIRST call (or the injection of a non-zero filter state) switches to the
 * kernels that evaluate it and synchronises the stream once - make it before capturing the per-cycle path in a hipGraph. */
int shc_engine_set_joint_effort(shc_engine *e, const double *joint_effort, int on_device);
/* bodyPoseInputCallback (state_controller.cpp:1142): translation / rotation velocity inputs [n][3] each. */
int shc_engine_set_pose_input(shc_engine *e, const double *translation_velocity, const double *rotation_velocity,
                              int on_device);
/* poseResetCallback -> PoseController::setPoseResetMode (pose_controller.h:105): mode [n], SHC_NO_RESET .. SHC_IMMEDIATE_ALL_RESET. */
int shc_engine_set_pose_reset_mode(shc_engine *e, const int32_t *mode, int on_device);

/*
 * Advance every instance by `n_cycles` control cycles (StateController::loop with robot_state
 * RUNNING, state_controller.cpp:162-193 + runningState :379-447).  Inputs are held for all
 * n_cycles.  Asynchronous on the engine's stream.
 */
int shc_engine_step(shc_engine *e, int n_cycles);
int shc_engine_synchronize(shc_engine *e);
/*
 * Batches of 4 096 wavefronts and more (40 960 hexapods, 32 768 octopods): shc_engine_step launches the two halves of the batch on
 * two INTERNAL streams (one pair per device, shared by every engine of the process on that device) and does NOT join them between consecutive steps (a robot's next cycle depends
 * on its own last cycle only; one half's partly filled last round of wavefronts then overlaps the other half's full rounds:
 * +20 ... 30 % control cycles per second).  Every other shc_engine_* / shc_leg_* entry point orders the engine's stream after both
 * halves before it enqueues anything, so getters, host-array setters and shc_engine_synchronize behave as before.  Setters given
 * DEVICE arrays (on_device) while split steps are in flight do not join: each half's own stream scatters its share of the array (after
 * waiting for the engine's stream, where the caller made the array ready), and the engine's stream is then ordered after both reads by
 * events - so the caller may overwrite or free the array on the engine's stream right after the setter returns, as before, without a
 * host wait and without draining the steps.  Only a caller that enqueues ITS OWN work on the engine's stream right after shc_engine_step
 * (a kernel reading shc_engine_joint_buffer, an event, a graph capture) calls shc_engine_join first: it makes the engine's stream wait
 * for the internal ones (no host wait).
 * SHC_FEAT_SINGLE_STREAM turns the split off.
 */
int shc_engine_join(shc_engine *e);

/*
 * Resident mode: the node's control loop kept on the chip.
 *
 * The reference runs `while (ros::ok()) { state.loop(); ...publish...; ros::spinOnce(); rate.sleep(); }` (src/main.cpp:106-131):
 * every iteration takes whatever the callbacks delivered since the last one (velocity :1127, body pose :1142, IMU :1552, joint
 * states :1566, tip states :1618 of src/state_controller.cpp), runs one control cycle (StateController::loop :162-193) and
 * publishes the desired joint state (:777-805).  shc_engine_step is one iteration per kernel launch: at batch sizes that fit the
 * chip once (<= 8 wavefronts per compute unit, e.g. up to ~20 000 hexapods on one MI355X) launch + state load + state store cost
 * as much as the cycle itself.  In resident mode ONE launch stays on the device for up to `max_cycles` iterations; per-leg state
 * lives in registers and per-robot state in LDS from one cycle to the next, and every iteration
 *   - waits for the loop tick: a cycle counter ("doorbell") that shc_engine_resident_publish advances,
 *   - takes the inputs posted for that cycle (shc_engine_resident_post; groups that were not posted keep their last value,
 *     exactly like a callback that did not fire), and
 *   - writes that cycle's desired joint positions and velocities to an output ring (shc_engine_resident_get_joint_state).
 * Results are bit-identical to the same cycles run through shc_engine_step(e, 1) with the same inputs set in between.
 *
 *   shc_engine_resident_begin(e, ring_depth, max_cycles, idle_timeout_ms)
 *       starts the loop (on a stream of the engine's own, ordered after everything queued on the engine's stream: the kernel does
 *       not end by itself, so it must not sit on a stream others use - the legacy default stream least of all).  ring_depth (2..255): input sets that may be posted ahead of the cycle that
 *       consumes them = cycles whose outputs stay readable; max_cycles (1..2^31-2): hard bound of this launch; idle_timeout_ms
 *       (0 = 5 000): the device loop stops by itself when everything released has run and the doorbell has not moved for this long
 *       (a host that went away cannot leave the GPU spinning; every device-side wait is bounded).  SHC_ERR_UNSUPPORTED: the batch does not fit the chip once, or
 *       the configuration runs on a manual-leg kernel (a leg toggled, planner mode), or a shc_engine_adjust_parameter of swing_height /
 *       virtual_mass / virtual_stiffness / virtual_damping_ratio / force_gain waits for its cycle (call shc_engine_step(e, 1) first: the
 *       resident kernel runs every cycle on one parameter block, the posing part of that cycle needs the old one).  Rough terrain mode, tip rotations and the tip-align
 *       pose (gravity_aligned_tips on <= 3-DOF legs, since round 5) have a resident form: one wavefront per robot group, up to ~990 wavefronts.  Until shc_engine_resident_end every other
 *       entry point that touches the engine's state returns SHC_ERR_BUSY.
 *   shc_engine_resident_post(e, inputs, cycle)
 *       the inputs "the callbacks delivered" for the next unposted cycle (*cycle receives its index, counted from 0 at begin):
 *       arrays as for shc_engine_set_velocity / set_imu / set_pose_input / set_pose_reset_mode / set_tip_force /
 *       set_joint_effort, NULL = not received this iteration.  linear_xy + angular, the two IMU arrays and the two pose arrays are
 *       posted in pairs.  Joint efforts / pose inputs can only be posted to an engine that was given one (shc_engine_set_joint_effort /
 *       shc_engine_set_pose_input) before shc_engine_resident_begin - the first one selects the kernels that evaluate them.
 *       Asynchronous (an internal input stream); blocks only when ring_depth input sets of a group are still waiting to be consumed.
 *       Posting does not release the cycle: shc_engine_resident_publish does.
 *   shc_engine_resident_publish(e, n_cycles)
 *       moves the doorbell: the device may run n_cycles more iterations (cycles nothing was posted for run with the inputs held).
 *   shc_engine_resident_wait(e, cycles, timeout_ms)
 *       returns once `cycles` iterations have completed on every instance and their outputs are visible (SHC_ERR_TIMEOUT otherwise).
 *   shc_engine_resident_get_joint_state(e, cycle, q, qd, on_device)
 *       desired joint positions / velocities [n][legs][dof] of iteration `cycle` (completed, and at most ring_depth - 1 iterations
 *       older than the newest published one) - what publishDesiredJointState sends after that loop iteration.  Blocking for host AND
 *       device buffers: q / qd are complete when the call returns (the copy runs on the engine's private input stream, which a
 *       caller cannot order anything after; the stream-ordered form is the _async call below).
 *   shc_engine_resident_get_joint_state_async(e, cycle, q, qd, timeout_ms)
 *       the same into DEVICE buffers, stream-ordered instead of host-ordered: returns at once having queued, on the engine's
 *       stream, a device-side wait for iteration `cycle` (which may still be unpublished; bounded by timeout_ms, 0 = 5 s) and the copy.
 *       Work the caller queues on that stream afterwards - the all-gather of the fleet's joint buffer - starts the moment the
 *       iteration's outputs exist, its launch latency hidden behind the iterations still running.  At most ring_depth - 1 newer
 *       iterations may be published before the copy has run.  A wait that gave up is reported by shc_engine_resident_end (SHC_ERR_TIMEOUT).
 *   shc_engine_resident_status(e, published, completed, running)
 *   shc_engine_resident_end(e, cycles_run)
 *       stops the loop after the published cycles, waits for it, and leaves the engine exactly as the same cycles through
 *       shc_engine_step would have (state planes, held inputs).  SHC_ERR_TIMEOUT: the loop had already stopped by itself
 *       (idle timeout) before everything published had run - the state is that of *cycles_run iterations, consistent across
 *       instances, and the engine is usable again.  If the loop does not ANSWER the stop request in time the call also returns
 *       SHC_ERR_TIMEOUT, but the engine stays in resident mode (the kernel may still be running: nothing else may touch the state,
 *       shc_engine_destroy waits for the kernel before it frees anything); call shc_engine_resident_end again.
 */
typedef struct shc_cycle_inputs {
  const double *linear_xy;                  /* [n][2]            velocity command (state_controller.cpp:1127) */
  const double *angular;                    /* [n]                                                            */
  const double *imu_orientation_wxyz;       /* [n][4]            sensor_msgs/Imu (:1552), normalised on entry */
  const double *imu_angular_velocity;       /* [n][3]                                                         */
  const double *pose_translation_velocity;  /* [n][3]            body pose input (:1142)                      */
  const double *pose_rotation_velocity;     /* [n][3]                                                         */
  const int32_t *pose_reset_mode;           /* [n]               SHC_NO_RESET ..                              */
  const double *tip_force;                  /* [n][legs][3]      tip wrench (:1618)                           */
  const double *joint_effort;               /* [n][legs][dof]    joint states (:1566)                         */
  int32_t on_device;                        /* the arrays are device pointers                                 */
  int32_t publish;                          /* != 0: release this cycle (and unpublished cycles before it) as soon as its inputs are in
                                               place - post + shc_engine_resident_publish(…, 1) in one kernel launch */
  int32_t direct;                           /* k = 1 .. 4: a DIRECT post from bound input set k - 1 (shc_engine_resident_bind_inputs): no kernel
                                               launch, no copy - the non-NULL members above only say WHICH groups are fresh this cycle (velocity,
                                               IMU, tip force, joint effort); the device loop reads them from the set's arrays when the cycle
                                               runs, and the cycle is released at once (publish is implied).  A few host stores per call. */
  int32_t reserved_;
} shc_cycle_inputs;
enum { SHC_RESIDENT_RUNNING = 0, SHC_RESIDENT_STOPPED = 1, SHC_RESIDENT_IDLE_TIMEOUT = 2, SHC_RESIDENT_MAX_CYCLES = 3, SHC_RESIDENT_FAULT = 4 };
int shc_engine_resident_begin(shc_engine *e, int ring_depth, int64_t max_cycles, int idle_timeout_ms);
/* Bind device arrays as input set `set` (0 .. 3) for direct posts; call it while the loop is NOT running (the addresses travel with the launch
 * of the loop kernel); NULL members = the set does not carry that group; arrays as for the setters ([n][2], [n], [n][4], [n][3],
 * [n][legs][3], [n][legs][dof]).  Contract of a direct post of set k for cycle c: the arrays hold the cycle's inputs (visible device-wide)
 * when shc_engine_resident_post is called.
 *  - Velocity and IMU arrays are sampled into the loop's own state when cycle c starts: they may be rewritten once a LATER cycle has
 *    completed (shc_engine_resident_wait(c + 2)).
 *  - Per-leg arrays (tip force, joint effort) are NOT copied: the set's arrays are the input IN FORCE - read again in every cycle, and once
 *    more when the loop ends (carried into the engine's own planes) - until a later post of THAT GROUP (direct from another set, or an
 *    ordinary post) has replaced them and the cycle it was made for has completed.  Until then they must not be written: a write changes
 *    the held input of the cycles in between, and a read that races it may be torn.
 * A host loop therefore alternates between two sets, as the node's callbacks fill one message while the controller reads the other, and
 * refills a set's per-leg arrays only after the other set's post of the same group has run. */
int shc_engine_resident_bind_inputs(shc_engine *e, int set, const shc_cycle_inputs *arrays);
int shc_engine_resident_post(shc_engine *e, const shc_cycle_inputs *inputs, int64_t *cycle);
int shc_engine_resident_publish(shc_engine *e, int64_t n_cycles);
int shc_engine_resident_wait(shc_engine *e, int64_t cycles, int timeout_ms);
int shc_engine_resident_get_joint_state(shc_engine *e, int64_t cycle, double *q, double *qd, int on_device);
int shc_engine_resident_get_joint_state_async(shc_engine *e, int64_t cycle, double *q, double *qd, int timeout_ms);
int shc_engine_resident_status(shc_engine *e, int64_t *published, int64_t *completed, int32_t *running);
int shc_engine_resident_end(shc_engine *e, int64_t *cycles_run);
/*
 * Resident tensors: the resident loop driven from the dense DEVICE arrays of the action and observation passes (shc_act_spec / shc_obs_spec,
 * declared with those passes below) - what a policy on the GPU emits and takes per tick, without a conversion on the way.
 * shc_engine_resident_post_actions: shc_engine_resident_post for the next unposted cycle (*cycle receives its index) from one array
 * [n][row_stride] of float64 or float32.  The spec, row and column rules are those of shc_engine_set_actions, legs / dof at least the engine's.
 * DEFINITION.  The loop runs the posted cycle, every later cycle and the state shc_engine_resident_end leaves byte for byte as after a
 * shc_engine_resident_post with on_device = 1 and the same `publish`, given dense float64 arrays that hold static_cast<double> of the named
 * columns and NULL for every group the spec does not name (those are held, like a callback that did not fire).  The IMU quaternion is
 * normalised in double after the conversion.  Columns of legs or joints the morphology lacks and columns [width, row_stride) are ignored; a
 * shorter leg's joints on a mixed-DOF robot get what the ordinary post stores there.  One kernel launch per call: it reads the array and stores
 * into the loop's input rings, writes the cycle's header and - with publish - rings the doorbell; nothing is staged.  Ring positions, the
 * back-pressure (ring_depth input sets of a group, 1 024 headers) and the rules of direct posts are the ordinary post's own.
 * STREAMS.  `actions` must be ready on the ENGINE's stream when the call is made (the rule of shc_engine_set_actions): the input stream follows
 * that stream before the post kernel, and the engine's stream follows the post kernel behind it, so work queued on the engine's stream after
 * the call may overwrite the array.  No host wait but the back-pressure.  A stream-ordered read (shc_engine_resident_get_joint_state_async, the
 * observation call below) parks the engine's stream until its cycle has run; while the highest cycle such a read was queued for is still
 * unpublished the call is refused - publish (or post the ordinary way with publish) first.
 * shc_engine_resident_get_observations_async: shc_engine_resident_get_joint_state_async as one array [n][row_stride]: the rules of
 * shc_engine_get_step_k_kinematics for any subset of SHC_OBS_Q, SHC_OBS_QD, SHC_OBS_MODEL_TIP.  The q / qd columns hold what
 * shc_engine_resident_get_joint_state returns for `cycle` - unchanged for SHC_OBS_F64, static_cast<float> for SHC_OBS_F32 -, model_tip is
 * Leg::applyFK on the ring's own q, `pad` where the robot has no such leg or joint, columns beyond the width untouched.  On the engine's stream
 * it queues the bounded device-side wait for `cycle` (which may still be unpublished; timeout_ms, 0 = 5 s) and ONE read kernel; nothing is
 * written into the engine.  A wait that gave up is reported by shc_engine_resident_end.
 * REFUSALS (decided before anything changes).  SHC_ERR_INVALID_ARG: NULL handle, spec or array; an engine not in resident mode; whatever
 * shc_engine_set_actions / shc_engine_get_step_k_kinematics refuse of a spec; SHC_ACT_LINEAR_XY without SHC_ACT_ANGULAR, one IMU or pose field
 * without its partner; a misaligned array; a cycle already published without inputs; a post or a `cycle` past max_cycles; a read whose slot may
 * have been overwritten; the stream rule above.  SHC_ERR_UNSUPPORTED: pose fields or joint efforts on an engine that was not given one before
 * shc_engine_resident_begin; an observation field outside the three.  SHC_ERR_TIMEOUT: the ordinary post's cases.
 * No fleet form (fleets have no resident mode), no host-array form.
 */
struct shc_act_spec;
struct shc_obs_spec;
int shc_engine_resident_post_actions(shc_engine *e, const struct shc_act_spec *spec, const void *actions /* device, [n][row_stride] */, int publish, int64_t *cycle);
int shc_engine_resident_get_observations_async(shc_engine *e, int64_t cycle, const struct shc_obs_spec *spec, void *out /* device, [n][row_stride] */, int timeout_ms);

/*
 * K loop iterations in ONE launch, each with its own inputs - for batches of any size (resident mode needs the whole batch on the chip at
 * once; this does not).  What `for (k = 0; k < K; ++k) { callbacks deliver inputs[k]; StateController::loop(); publish the desired joint state; }`
 * (src/main.cpp:106-131, src/state_controller.cpp:162-193, :777-805) does, with the state loaded once, kept in registers / LDS for the K cycles and
 * stored once: per cycle only that cycle's inputs are read and its q / qd written.
 *   inputs (may be NULL = every input held): DEVICE arrays (on_device = 1) of K rows each - linear_xy [K][n][2] + angular [K][n],
 *     imu_orientation_wxyz [K][n][4] + imu_angular_velocity [K][n][3], tip_force [K][n][legs][3], joint_effort [K][n][legs][dof]; a NULL member
 *     is held at what the engine has.  Row k is what shc_engine_set_velocity / set_imu / set_tip_force / set_joint_effort would have been given
 *     before cycle k (in rough terrain mode Leg::touchdownDetection runs on the fresh tip force inside the loop, model.cpp:712-722).  Pose
 *     inputs / reset modes are not carried (set them before the call; they are held).  The arrays are read while the launch runs: keep them
 *     valid and unchanged until shc_engine_join (or any synchronising call: shc_engine_synchronize, shc_engine_get_step_k_joint_state, the next
 *     shc_engine_step / step_k) has been ISSUED after this one and the engine's stream has passed that point.  An event recorded on the engine's
 *     stream right after shc_engine_step_k is NOT enough for batches of >= 4 096 wavefronts: those launch on the engine's two internal half-streams
 *     and the engine's own stream is ordered behind them only by the next join (the same holds for a caching allocator that would reuse the
 *     arrays' memory).  After the call the last row is the engine's held input.
 *   The result is bit-identical to K x { setters with row k; shc_engine_step(e, 1) } - state record and the q / qd of every cycle.
 *   shc_engine_get_step_k_joint_state(e, k, q, qd, on_device): q / qd [n][legs][dof] of cycle k (0 .. K - 1) of the latest launch
 *     (stream-ordered; the ring is overwritten by the next shc_engine_step_k).  shc_engine_get_joint_state returns cycle K - 1 as usual.
 * Configurations without a batch kernel - a manual-leg kernel (a leg toggled, planner mode: manual inputs and the plan are held for the K cycles like
 * the pose inputs) and, unless the library was built with SHC_GENERIC_LOOP_FORMS=1, the runtime-flag kernel families (any posing set other than
 * default.yaml's / BASELINE config 3's) - run the same K cycles as K single launches inside the call: same results, same output ring, no launch saved.
 * 1 <= K <= 4096, and K x n x legs x dof x 16 B must stay below 2 GiB.
 */
int shc_engine_step_k(shc_engine *e, int n_cycles, const shc_cycle_inputs *inputs);
int shc_engine_get_step_k_joint_state(shc_engine *e, int k, double *q, double *qd, int on_device);

/*
 * One process per GPU: the exchange of the final joint buffer as peer copies over xGMI, without a collective library (the alternative to the
 * RCCL all-gather the one-process-per-GPU host runs; shc_fleet_all_gather_joints is the same exchange inside one process).  Every rank
 * allocates its gathered buffer with shc_peer_alloc (which also exports it: a 64-byte handle the ranks exchange by whatever means they have),
 * opens every peer's buffer (shc_peer_open) and, after its last step, writes its shard into every buffer at its own offset:
 * shc_peer_scatter(device, shard, bytes, destinations, n, stream) - one copy per destination on a stream of its own (the N - 1 links of a GPU
 * carry N - 1 copies at once), ordered after `stream`, and `stream` ordered after them.  A barrier of the caller's - every rank's copies have
 * completed - closes the exchange.  Nothing orders an exchange after the peers' READS of the previous one: a rank that gathers again while another rank is
 * still consuming its gathered buffer overwrites a slot under that reader, so a barrier of the caller's belongs BEFORE every exchange as well (or one
 * gathered buffer per exchange in flight).  shc_peer_close(device, ptr, opened): opened != 0 for a peer's buffer, 0 frees one's own and releases the
 * copy streams / events shc_peer_scatter keeps for that device.
 */
int shc_peer_alloc(int device, int64_t bytes, void **device_ptr, unsigned char *handle64);
int shc_peer_open(int device, const unsigned char *handle64, void **device_ptr);
int shc_peer_close(int device, void *device_ptr, int opened);
int shc_peer_scatter(int device, const void *src, int64_t bytes, void *const *dst, int n_dst, void *stream);

/*
 * Outputs read after the cycle (state_controller.cpp:777-805 publishDesiredJointState).
 * q/qd: [n][legs][dof] desired joint position / velocity.  Either may be NULL.
 */
int shc_engine_get_joint_state(shc_engine *e, double *q, double *qd, int on_device);
/*
 * Device view of the engine's own joint-position planes (paired structure-of-arrays):
 * the raw buffer a multi-GPU caller may all-gather without a transpose.  `*n_doubles` = 2 * ceil(dof / 2) * n_slots, n_slots =
 * 64 per wavefront of ⌊64 / legs⌋ robots + 192 slots of plane-stride padding
 * (for an odd DOF the last plane also carries the first joint velocity); use shc_engine_joint_index to address it.
 */
int shc_engine_joint_buffer(shc_engine *e, double **device_ptr, int64_t *n_doubles);
/* Map instance-major (i, leg, j) to an index into the buffer above. */
int64_t shc_engine_joint_index(const shc_engine *e, int64_t instance, int leg, int joint);

/* LegState-style per-leg outputs (state_controller.cpp:809-893): any pointer may be NULL.
 *   walker_tip   [n][legs][3]  LegStepper::current_tip_pose_.position_
 *   poser_tip    [n][legs][3]  LegPoser::current_tip_pose_.position_ (posed, body frame)
 *   model_tip    [n][legs][3]  Leg::current_tip_pose_.position_ (FK)
 *   tip_force    [n][legs][3]  Leg::tip_force_calculated_
 *   admittance   [n][legs][3]  Leg::admittance_delta_
 *   leg_status   [n][legs]     packed: bits 0-1 step state, bit 2 ik failure (model.cpp:921), bits 8.. phase
 */
int shc_engine_get_leg_state(shc_engine *e, double *walker_tip, double *poser_tip, double *model_tip,
                             double *tip_force, double *admittance, int32_t *leg_status, int on_device);
/* Per-robot outputs: body pose [n][7] (x,y,z,qw,qx,qy,qz) = Model::current_pose_ (state_controller.cpp:911),
 * desired velocity [n][3] (vx,vy,omega), walk_state [n]. */
int shc_engine_get_body_state(shc_engine *e, double *pose, double *velocity, int32_t *walk_state, int on_device);
/*
 * StateController::changeGait (state_controller.cpp:513-538; gaitSelectionCallback :1206): the gait members of `new_gait`
 * (stance_phase, swing_phase, phase_offset, offset_multiplier and, with auto_posing, the auto-pose tables) replace the
 * engine's; step cycle, velocity / acceleration limits and auto-pose phases are regenerated as generateStepCycle +
 * generateLimits + setAutoPoseParams do.  A batch shares one gait, so the change happens only when EVERY instance is
 * STOPPED; otherwise the velocity inputs of all instances are zeroed (the reference "forces the Syropod to stop") and
 * *still_walking receives the number of instances not yet STOPPED: step on and call again, as the reference retries on
 * every loop while gait_change_flag_ is set.  Synchronises the engine's stream.
 */
int shc_engine_change_gait(shc_engine *e, const shc_params *new_gait, int64_t *still_walking);
/*
 * StateController::adjustParameter (state_controller.cpp:451-509), reached from parameterSelectionCallback / parameterAdjustCallback (:1419-1463, the
 * adjustable_map of :1884-1892) and from dynamicParameterCallback (:1467-1548): one of the nine run-time adjustable parameters takes `value` (the callbacks'
 * clamping to the parameter's min / max is the caller's - the node's - as are adjust_step and the selection).  `which` numbers them as enum
 * ParameterSelection does (parameters_and_states.h:165-178).  A batch shares its parameters: the change is for every instance.
 *   The eight parameters the cycle reads as they are (swing_height, swing_width, step_depth, stance_span_modifier, virtual_mass, virtual_stiffness,
 *   virtual_damping_ratio, force_gain) are in force from the next control cycle: a new launch-uniform block, no table regenerated, no state touched
 *   (stance_span_modifier moves the default tips when calculateStanceSpanChange next runs - at a stop, or at swing / stance start in rough terrain).
 *   step_frequency: as in the reference the new value is stored at once (:454: sequence / transition timings read it from then on) and the maximum-speed maps
 *   and the legs' phase offsets of the NEW step cycle replace the current ones at once (:458-463, generateLimits' setPhaseOffset walk_controller.cpp:277) -
 *   the walker slows down to them.  The step cycle itself and all four limit maps are regenerated (generateStepCycle + generateLimits, :491-492) only when the
 *   desired body velocity is inside what the velocity input maps to under the new limits (:464-489) - here: for EVERY instance; otherwise *pending (may be
 *   NULL) receives the number of instances still outside and the caller calls again after the next cycle, as runningState retries on every loop while
 *   parameter_adjust_flag_ is set (:411-414).  On acceptance (*pending = 0) the legs of walking robots are mapped onto the new cycle
 *   (LegStepper::updatePhase, walk_controller.cpp:862-867) INSIDE the next control cycle, between its posing part and updateWalk, where the reference's
 *   loop has it; that cycle runs alone in its launch on the runtime-flag kernels.  The posing part of that next cycle (updateStiffness / updateAdmittance)
 *   still runs on the old swing_height, virtual_mass / stiffness / damping_ratio and force_gain, and a leg toggle, plan step or sequence step that is
 *   that next loop runs its own kernels on the old values too (adjustParameter stores them after legStateToggle / executePlan, :396-414).  The loops
 *   that consume the change for every instance are those that reach runningState in the reference: shc_engine_step, shc_engine_step_k (its first
 *   cycle runs as one shc_engine_step), shc_engine_toggle_leg_state, shc_engine_execute_plan, shc_engine_execute_sequence(SHUT_DOWN).
 *   execute_sequence(START_UP) (from READY) and shc_engine_step_to_new_stance run on the old values and leave the change pending.
 *   shc_engine_get_state / set_state do not: a record shows the phases still in the old period, and injected phases are mapped inside the next loop.
 *   Resident mode maps a pending step-cycle change's phases before it starts (the one-loop ordering against the posing part is then not kept) and
 *   refuses to start (SHC_ERR_UNSUPPORTED) while old posing values are held: step once first.  The auto-pose phase tables keep the old step period
 *   (setAutoPoseParams is not called by adjustParameter).  SHC_ERR_UNSUPPORTED for step_frequency in rough_terrain_mode, with gravity_aligned_tips or with a
 *   non-zero stance_span_modifier (the posing part / the limit generation read stepper state there that this ordering cannot reproduce); the other eight
 *   parameters have no such restriction.  Synchronises the engine's stream; SHC_ERR_BUSY in resident mode.
 */
enum {
  SHC_PARAM_STEP_FREQUENCY = 1, SHC_PARAM_SWING_HEIGHT = 2, SHC_PARAM_SWING_WIDTH = 3, SHC_PARAM_STEP_DEPTH = 4, SHC_PARAM_STANCE_SPAN_MODIFIER = 5,
  SHC_PARAM_VIRTUAL_MASS = 6, SHC_PARAM_VIRTUAL_STIFFNESS = 7, SHC_PARAM_VIRTUAL_DAMPING = 8, SHC_PARAM_FORCE_GAIN = 9
};
int shc_engine_adjust_parameter(shc_engine *e, int which, double value, int64_t *pending);
/* WalkController::getOdometryIdeal() (walk_controller.h:112; integrated at walk_controller.cpp:643 from
 * calculateOdometry :783-791): [n][7] (x,y,z,qw,qx,qy,qz).  Needs SHC_FEAT_ODOMETRY (on by default). */
int shc_engine_get_odometry(shc_engine *e, double *pose, int on_device);
/* Leg::getVirtualStiffness() (model.h:264) as left by AdmittanceController::updateStiffness
 * (admittance_controller.cpp:96-134; only published, state_controller.cpp:889): [n][legs].  Updated while
 * admittance_control && dynamic_stiffness && walk state != STOPPED (state_controller.cpp:172-178); 0 before the
 * first update (the reference leaves the member uninitialised).  SHC_ERR_UNSUPPORTED without admittance_control. */
int shc_engine_get_virtual_stiffness(shc_engine *e, double *stiffness, int on_device);

/*
 * ROS message surface.  Numeric payload of syropod_highlevel_controller/LegState.msg as
 * StateController::publishLegState fills it (msg/LegState.msg; state_controller.cpp:809-893), one record per leg of ONE
 * instance: the node copies the fields into its message and adds stamps, frame ids and the leg name.
 * Tip orientations of the walker / poser tips are not part of the payload (UNDEFINED (0,0,0,0) unless gravity_aligned_tips).
 */
typedef struct shc_leg_state_msg {
  double walker_tip_position[3]; /* walker_tip_pose.pose.position   :822-824 (frame walk_plane) */
  double target_tip_position[3]; /* target_tip_pose.pose.position   :826-828 */
  double poser_tip_position[3];  /* poser_tip_pose.pose.position    :830-832 (frame base_link) */
  double model_tip_position[3];  /* model_tip_pose.pose.position    :834-836 */
  double actual_tip_pose[7];     /* actual_tip_pose.pose :837-839 = Leg::applyFK(false, true): FK of the MEASURED joint positions
                                    (x,y,z,qw,qx,qy,qz); until shc_engine_set_joint_states_msg supplies them these are the initial default
                                    positions Leg::init(true) copied (model.cpp:292-296) */
  double model_tip_velocity[3];  /* model_tip_velocity.twist.linear :845-849: always 0 - publishLegState calls applyFK() on
                                    unchanged joints just before (:840), which resets Leg::current_tip_velocity_ to
                                    (tip - tip) / dt (model.cpp:980) */
  double joint_positions[SHC_MAX_JOINTS];  /* Joint::desired_position_ :854 */
  double joint_velocities[SHC_MAX_JOINTS]; /* Joint::desired_velocity_ :855 */
  double joint_efforts[SHC_MAX_JOINTS];    /* Joint::desired_effort_   :856 = the last measured effort (jointStatesCallback :1590) */
  double stance_progress, swing_progress;  /* :860-861, -1 when not in that state (walk_controller.cpp:871-897) */
  double time_to_swing_end;                /* :862-874 */
  double pose_delta[7];                    /* calculateOdometry(time_to_swing_end) :875: x,y,z,qw,qx,qy,qz */
  double auto_pose[7];                     /* LegPoser::auto_pose_ :877-880 (x,y,z,qw,qx,qy,qz): the identity pose when
                                              auto_posing is off (never assigned, pose_controller.cpp:1716); with auto posing
                                              the per-leg pose of the last cycle (negation applied), re-derived from the
                                              stored poser latches and master phase */
  double tip_force[3];                     /* tip_force_calculated_ * force_gain :883-885 */
  double admittance_delta[3];              /* :886-888 */
  double virtual_stiffness;                /* :889 */
} shc_leg_state_msg;
/* Fills legs[0 .. leg_count) for `instance`.  Synchronises the engine's stream. */
int shc_engine_read_leg_state_msg(shc_engine *e, int64_t instance, shc_leg_state_msg *legs);
/* publishLegState for instances [first, first + count) in one device pass: msgs[(i - first) * legs + l], the record layout of
 * shc_leg_state_msg - 64 doubles, no padding: a dense [count][legs][64] double array - every field as documented above; the joint
 * slots a robot does not use are zero.  on_device = 1: msgs is a device buffer (16-byte aligned), the call is ordered on the engine's
 * stream and does not synchronise the host; on_device = 0: msgs is host memory, the call synchronises the stream.  Refreshes the
 * derived model / poser tips as shc_engine_get_leg_state does and changes no other state.  count = 0 is a no-op.
 * SHC_ERR_INVALID_ARG for a NULL msgs or a range outside [0, n); SHC_ERR_BUSY in resident mode. */
int shc_engine_get_leg_state_msgs(shc_engine *e, int64_t first, int64_t count, shc_leg_state_msg *msgs, int on_device);

/*
 * StateController::publishFrameTransforms (state_controller.cpp:963-1047), batched: the numeric payload of every TransformStamped the node
 * broadcasts per loop - odom_ideal -> base_link, base_link -> walk_plane, base_link -> every joint and every tip of every leg.  The node adds
 * stamps, frame ids and child names (joint->id_name_, tip->id_name_).  tf LOOKUPS (generateExternalTargetTransforms :703-773) stay with the
 * caller (shc_engine_set_external_transform).  Every pose is (x, y, z, qw, qx, qy, qz); the records are doubles without padding.
 */
#define SHC_FRAME_JOINTS 5 /* joint frames per leg record: the longest leg the engine has kernels for (leg_dof 3..5) */
enum {
  SHC_FRAME_BASE_LINK = 0,  /* the leg frames as publishFrameTransforms sends them: children of base_link */
  SHC_FRAME_ODOM_IDEAL = 1  /* every joint / tip frame composed with odom_to_base_link (odom_to_base_link.addPose(child), pose.h:167-173):
                             * world poses for consumers that do not run a tf tree */
};
typedef struct shc_leg_frames { /* one per leg: 42 doubles, 336 bytes */
  double joint[SHC_FRAME_JOINTS][7]; /* joint j: position = Joint::getPoseRobotFrame().position_ (:1015-1022; model.h:594-608: the chain's DH
                                      * product up to the joint, pose.h:135-146); rotation = joint_robot_frame.rotation_ *
                                      * AngleAxisd(desired_position_, UnitZ()) (:1023-1028).  The frames of the DESIRED joint positions (the
                                      * chain applyFK() left behind).  Slots past the leg's own joint count are all zero */
  double tip[7];                     /* Tip::getPoseRobotFrame() (:1032-1045; model.h:684-688) of the leg's own chain */
} shc_leg_frames;
typedef struct shc_body_frames { /* one per robot: 20 doubles, 160 bytes */
  double odom_to_base_link[7];       /* getOdometryIdeal().addPose(getCurrentPose()) (:965-967, :984-990; pose.h:167-173) */
  double base_link_to_walk_plane[7]; /* ~getCurrentPose() (:995-1005; pose.h:112-115) */
  double pose_euler[3];              /* quaternionToEulerAngles(current_pose.rotation_): the angular part of publishPose (:911-923;
                                      * standard_includes.h:248-291) */
  double desired_velocity[3];        /* (vx, vy, omega) of publishVelocity (:897-907) */
} shc_body_frames;
/* The frames of instances [first, first + count) in one device pass: legs[(i - first) * leg_count + l], body[i - first]; either may be NULL
 * (not both).  frame = SHC_FRAME_BASE_LINK or SHC_FRAME_ODOM_IDEAL selects the parent of the leg frames; the body records are the same for
 * both.  on_device = 1: legs / body are device buffers (16-byte aligned), the call is ordered on the engine's stream and does not synchronise
 * the host; on_device = 0: host memory, the call synchronises the stream.  Changes no engine state.  count = 0 is a no-op.
 * SHC_ERR_INVALID_ARG for a range outside [0, n), both pointers NULL or an unknown frame; SHC_ERR_UNSUPPORTED without SHC_FEAT_ODOMETRY when
 * body records or SHC_FRAME_ODOM_IDEAL are asked for; SHC_ERR_BUSY in resident mode. */
int shc_engine_get_frame_transforms(shc_engine *e, int64_t first, int64_t count, int frame, shc_leg_frames *legs /* [count][legs] */,
                                    shc_body_frames *body /* [count] */, int on_device);

/*
 * The other ROS messages of the path, batched: payloads in, payloads out; the node adds names,
 * stamps and frame ids.
 */
/* jointStatesCallback (state_controller.cpp:1566-1594), sensor_msgs/JointState as the motors report it: position rows
 * [n][legs][dof] are RAW motor positions - the callback stores position - Joint::offset_ as Joint::current_position_ (:1581; used by
 * Leg::applyFK(.., use_actual) for LegState.actual_tip_pose) - and effort rows [n][legs][dof] become Joint::current_effort_ /
 * desired_effort_ (:1589-1590, what Leg::calculateTipForce and LegState.joint_efforts read).  velocity is stored by the
 * reference but never read on this path: accepted for symmetry, ignored.  Any pointer may be NULL. */
int shc_engine_set_joint_states_msg(shc_engine *e, const double *position, const double *velocity, const double *effort, int on_device);
/* tipStatesCallback (state_controller.cpp:1617-1679), syropod_highlevel_controller/TipState: wrench force rows [n][legs][3]
 * (= shc_engine_set_tip_force: stores the force, switches touchdown detection on, runs Leg::touchdownDetection) and / or the
 * range sensors' step_plane rows [n][legs][3] = (x, y, z): z = distance to the step surface along the tip's x axis, or
 * UNASSIGNED_VALUE (2147483647) when the sensor lost contact -> Leg::step_plane_pose_ (:1661-1672).  Either may be NULL. */
int shc_engine_set_tip_states_msg(shc_engine *e, const double *wrench_force, const double *step_plane, int on_device);
/* publishDesiredJointState (state_controller.cpp:777-805): the combined sensor_msgs/JointState payload (Leg::
 * generateDesiredJointStateMsg, model.cpp:605-617: desired_position_, desired_velocity_, desired_effort_) and the per-joint
 * std_msgs/Float64 position commands desired_position_ + offset_ (:798).  All [n][legs][dof]; any pointer may be NULL. */
int shc_engine_get_joint_commands(shc_engine *e, double *position, double *velocity, double *effort, double *position_command, int on_device);

/*
 * Per-leg methods of class Leg (model.h:448-492), batched.  The reference's cold paths call them on their own - workspace
 * search (model.cpp:309-510), start-up / shut-down sequences (pose_controller.cpp:145-805), leg manipulation
 * (state_controller.cpp:590-700); the fused cycle runs the same arithmetic in registers.  They act on the engine's joint state:
 * a cycle launched afterwards continues from the joints these calls left.
 * Selection: instances [first, first + count), leg = -1 for every leg or one leg id.  Arrays hold one row per selected
 * (instance, leg) in instance-major order: [count][legs or 1][K].  Host pointers unless on_device != 0.
 */
/* Leg::setDesiredTipPose(tip_pose, apply_delta) (model.h:448, model.cpp:653): tip_pose rows are (x,y,z,qw,qx,qy,qz), an
 * all-zero quaternion = UNDEFINED_ROTATION (position-only IK); tip_pose == NULL = the default argument Pose::Undefined() =
 * "take the poser's tip pose"; apply_delta adds Leg::admittance_delta_. */
int shc_leg_set_desired_tip_pose(shc_engine *e, int64_t first, int64_t count, int leg, const double *tip_pose, int apply_delta, int on_device);
/* Leg::solveIK(delta, solve_rotation) (model.h:470, model.cpp:726): delta rows are the 6-vector (position delta, rotation
 * delta) in the leg (joint 1) frame; joint_delta rows [dof].  Reads the joint state, changes nothing. */
int shc_leg_solve_ik(shc_engine *e, int64_t first, int64_t count, int leg, const double *delta, int solve_rotation, double *joint_delta,
                     int on_device);
/* Leg::updateJointPositions(delta, simulation) (model.h:477, model.cpp:799): integrates joint_delta (velocity clamp unless
 * simulation, position clamp per parameters); limit_proximity rows [1] (may be NULL) receive the returned minimum proximity. */
int shc_leg_update_joint_positions(shc_engine *e, int64_t first, int64_t count, int leg, const double *joint_delta, int simulation,
                                   double *limit_proximity, int on_device);
/* Leg::applyIK(simulation) (model.h:485, model.cpp:861) towards the stored desired tip pose: position solve, rotation solve
 * when the desired rotation is defined, unconstrained retry, 5 mm deviation check, calculateTipForce.  ik_result rows [1]
 * (may be NULL): limit proximity, 0 on failure. */
int shc_leg_apply_ik(shc_engine *e, int64_t first, int64_t count, int leg, int simulation, double *ik_result, int on_device);
/* Leg::applyFK(set_current, use_actual) (model.h:492, model.cpp:945): tip pose rows (x,y,z,qw,qx,qy,qz) in the robot frame from
 * the desired joint positions, or from joint_position rows [dof] when given (use_actual: the measured positions of
 * jointStatesCallback, which the engine does not store - this is what LegState.actual_tip_pose needs, state_controller.cpp:839). */
int shc_leg_apply_fk(shc_engine *e, int64_t first, int64_t count, int leg, const double *joint_position, double *tip_pose, int on_device);

/*
 * Sequences: the LegPoser building blocks of PoseController's start-up / shut-down / stance-change
 * procedures, batched with the same (first, count, leg) selection as the per-leg methods, and the direct start-up built on them.
 */
/* LegPoser::stepToPosition(target_tip_pose, target_pose, lift_height, time_to_step, apply_delta) (pose_controller.h:506,
 * pose_controller.cpp:1571-1712), ONE iteration: the tip follows two quartic Bezier curves from where the leg stood when the
 * sequence began to target_tip_pose (rows (x,y,z,qw,qx,qy,qz); NULL = Pose::Undefined() = stay, rotation undefined) while the
 * body pose eases from the identity to target_pose ([count][7], one row per instance).  tip_pose rows receive
 * LegPoser::current_tip_pose_ - hand them to shc_leg_set_desired_tip_pose + shc_leg_apply_ik as stepToNewStance (:521) and
 * directStartup (:463) do; progress rows (int32, may be NULL) the returned percentage (100 = complete, the next call starts a
 * new sequence). */
int shc_leg_step_to_position(shc_engine *e, int64_t first, int64_t count, int leg, const double *target_tip_pose, const double *target_pose,
                             double lift_height, double time_to_step, int apply_delta, double *tip_pose, int32_t *progress, int on_device);
/* LegPoser::transitionConfiguration(transition_time) towards desired_configuration rows [dof] (pose_controller.h:498,
 * pose_controller.cpp:1476-1567), ONE iteration: every joint follows a cubic Bezier from the configuration it had when the
 * transition began. */
int shc_leg_transition_configuration(shc_engine *e, int64_t first, int64_t count, int leg, const double *desired_configuration,
                                     double transition_time, int32_t *progress, int on_device);
/* PoseController::directStartup (pose_controller.cpp:463-517) for the batch.  shc_engine_begin_direct_startup puts every
 * instance where StateController::init + initModel(true) leave a robot (joints at clamped(0, min, max), model.cpp:286-305,
 * :1038; robot state PACKED "undefined", state_controller.cpp:213-222); each shc_engine_direct_startup call is one
 * StateController::loop() of the PACKED -> READY transition: every joint advances along its transition to the default
 * configuration (the joints the init chain's simulated start-up solve ended on).  *progress = 1..100; the call that returns
 * 100 also runs the loop that enters RUNNING, after which the engine is exactly where shc_engine_create leaves it and the
 * joints published on the way are the reference's start-up trajectory. */
int shc_engine_begin_direct_startup(shc_engine *e);
int shc_engine_direct_startup(shc_engine *e, int32_t *progress);
/*
 * Start-up / shut-down SEQUENCES (start_up_sequence: true): PoseController::executeSequence (pose_controller.cpp:145-459) and
 * PoseController::stepToNewStance (:521-557) for the batch, every instance with its own PoseController state (transition step,
 * leg group, the transition poses its first START_UP learns, pose_controller.h:273-304, :591-593).
 *   shc_engine_begin_sequence_startup  StateController::init() + initModel(false) (main.cpp:99-100, model.cpp:286-305): fresh
 *       walker / poser state, every joint where the motors report it.  joint_positions: [legs][dof] rows shared by all instances,
 *       or [n][legs][dof] with per_instance = 1 (host array, offsets removed); NULL = the READY configuration (every joint at its
 *       `unpacked` position, state_controller.cpp:217).
 *   shc_engine_execute_sequence        ONE call of executeSequence(sequence) per instance.  progress rows [n] (host, may be NULL):
 *       -1 while a first START_UP is still generating its sequence, 0..99, 100 = complete, -2 = gave up (more than
 *       TRANSITION_STEP_THRESHOLD transitions: the reference shuts down).  An instance that has completed `sequence` is left
 *       alone by further calls with the same `sequence` (robots that learnt different sequences finish after different numbers
 *       of calls; the caller loops until every row reads 100).  The node calls it where
 *       transitionRobotState does (:301, :334: once per loop for START_UP, twice per loop for SHUT_DOWN through runningState :384-388).
 *       The body pose is Model::current_pose_ as the last control cycle left it (the sequences run with the robot stopped).
 *   shc_engine_finish_sequence_startup what follows a completed START_UP (:305-313): walker_->init(), the configuration the
 *       sequence ended on becomes the default configuration, workspaces / walkspace / limits are regenerated from it (instance 0
 *       stands for the batch: the tables belong to the engine), robot state RUNNING and the first control cycle of the same loop.
 *       Auto posing on its own clock (pose_frequency != -1) keeps posing through the sequence; the PoseController's phase counter, poser latches and
 *       Model::current_pose_ carry over into RUNNING and the workspace is searched at the pose of the completing loop (model.cpp:338) - which every
 *       instance must share (SHC_ERR_UNSUPPORTED when they completed START_UP in different phases of the auto pose, with IMU posing on top, or on
 *       tip-align robots).  The sequence calls of such robots run their posing part as a pose-only pass of the manual-leg cycle kernels; that
 *       leaves no trace: shc_engine_step keeps its kernels, shc_engine_step_k and resident mode stay available afterwards.
 *   shc_engine_step_to_new_stance      ONE call of stepToNewStance per instance (progress as the reference returns it).
 *   shc_engine_pack_legs / unpack_legs PoseController::packLegs / unpackLegs (:615-707), ONE call per loop: every joint follows its
 *       cubic Bezier (LegPoser::transitionConfiguration) to the packed positions of the current pack step / back to the previous
 *       step's and finally the `unpacked` positions.  packed_positions = Joint::packed_positions_ as [n_pack_steps][legs][dof]
 *       (default.yaml "packed" may list several steps per joint).  *progress as the reference returns it (0 between pack steps,
 *       100 when done); the pack step and "transition executing" flag are PoseController members, kept per engine (every
 *       instance runs the same number of iterations).
 */
enum { SHC_MANIPULATION_TIP_CONTROL = 0, SHC_MANIPULATION_JOINT_CONTROL = 1 };
enum { SHC_SEQUENCE_START_UP = 0, SHC_SEQUENCE_SHUT_DOWN = 1 }; /* enum SequenceSelection (parameters_and_states.h:183-188) */
int shc_engine_begin_sequence_startup(shc_engine *e, const double *joint_positions, int per_instance);
int shc_engine_execute_sequence(shc_engine *e, int sequence, int32_t *progress);
int shc_engine_finish_sequence_startup(shc_engine *e);
int shc_engine_step_to_new_stance(shc_engine *e, int32_t *progress);
/*
 * Manual leg manipulation: StateController::legStateToggle (state_controller.cpp:541-646) with PoseController::
 * poseForLegManipulation (pose_controller.cpp:561-611), and WalkController::updateManual (walk_controller.cpp:652-744, both overloads)
 * inside the control cycle.
 *   shc_engine_toggle_leg_state   ONE StateController::loop() for EVERY instance, with a toggle request pending for the leg
 *       leg_selection[i] designates (host [n]; -1 = no request).  result rows [n]: 1 = transition complete (WALKING <-> MANUAL:
 *       the node clears its toggle flag), 0 = in progress, 2 = refused (MAX_MANUAL_LEGS = 2 already manual), -1 = the robot is
 *       still walking: its velocity inputs are zeroed (:641-645) and its loop is one ordinary control cycle, -3 = no request: one
 *       ordinary control cycle (the call launches the cycle kernel for those two groups only).  While a robot has a leg that is not WALKING its walker
 *       is frozen (updateWalk returns at walk_controller.cpp:503); MANUAL / WALKING_TO_MANUAL legs are not posed (updateStance).
 *       Every posing mode (walk-plane, manual, inclination, IMU, auto) keeps running for the robots that stand during the call - the
 *       posing part of their loop (state_controller.cpp:165-181) is a pose-only pass of the cycle kernel.  With the experimental
 *       tip-align pose (gravity_aligned_tips on <= 3-DOF legs): SHC_ERR_UNSUPPORTED.
 *   shc_engine_set_manual_inputs  primary / secondary leg selection [n] (-1 = LEG_UNDESIGNATED) with their tip velocity inputs
 *       [n][3] (updateManual(.., tip_velocity_input, ..): tip_control moves the tip, joint_control the coxa / tibia joints of
 *       3-DOF legs - whose stepper then holds the FK tip pose WITH its rotation, so that applyIK runs rotation-constrained on them
 *       (walk_controller.cpp:677-690) - and nothing on longer legs, params.leg_manipulation_mode) and tip position inputs [n][3] (updateManual(.., Pose, ..); a zero vector
 *       = none).  Host arrays, any may be NULL.
 *   shc_engine_get_leg_manipulation_state  enum LegState per (instance, leg): 0 WALKING, 1 MANUAL, -1 WALKING_TO_MANUAL,
 *       -2 MANUAL_TO_WALKING.
 */
int shc_engine_toggle_leg_state(shc_engine *e, const int32_t *leg_selection, int32_t *result);
int shc_engine_set_manual_inputs(shc_engine *e, const int32_t *primary_leg, const double *primary_tip_velocity, const double *primary_tip_position,
                                 const int32_t *secondary_leg, const double *secondary_tip_velocity, const double *secondary_tip_position);
int shc_engine_get_leg_manipulation_state(shc_engine *e, int32_t *states);
int shc_engine_pack_legs(shc_engine *e, const double *packed_positions, int n_pack_steps, double time_to_pack, int32_t *progress);
int shc_engine_unpack_legs(shc_engine *e, const double *packed_positions, int n_pack_steps, double time_to_unpack, int32_t *progress);

/*
 * Full controller state of one instance (checkpoint / restore, state injection).  Everything the next control cycle reads
 * that is not an input set through the shc_engine_set_* calls above: restoring a snapshot and replaying the same inputs
 * reproduces the run bit for bit.  Members are named after the reference members they hold.
 */
typedef struct shc_leg_snapshot {
  double joint_position[SHC_MAX_JOINTS];   /* Joint::desired_position_  (model.h:635) */
  double joint_velocity[SHC_MAX_JOINTS];   /* Joint::desired_velocity_  (model.h:636) */
  double walker_tip[3];                    /* LegStepper::current_tip_pose_.position_ (walk_controller.h:520) */
  double walker_tip_velocity[3];           /* LegStepper::current_tip_velocity_       (:527) */
  double swing_origin_tip[3];              /* swing_origin_tip_position_              (:529) */
  double swing_origin_tip_velocity[3];     /* swing_origin_tip_velocity_              (:530) */
  double stance_origin_tip[3];             /* stance_origin_tip_position_             (:531) */
  double default_tip[3];                   /* default_tip_pose_.position_             (:519) */
  double target_tip[3];                    /* target_tip_pose_.position_              (:522) */
  double stride_vector[3];                 /* stride_vector_                          (:512) */
  /* Tip rotations (gravity_aligned_tips, > 3 DOF): every consumer of LegStepper::current_tip_pose_.rotation_ /
   * origin_tip_pose_.rotation_ reads only the rotated x axis (walk_controller.cpp:1217-1224, pose_controller.cpp:129-130,
   * model.cpp:884-893), so the state is that unit vector + whether the current rotation is defined (!= UNDEFINED_ROTATION) */
  double walker_tip_direction[3];
  double origin_tip_direction[3];
  double admittance_state[2];              /* Leg::admittance_state_    (model.h:518) */
  double admittance_delta[3];              /* Leg::admittance_delta_    (model.h:365) */
  double virtual_stiffness;                /* Leg::virtual_stiffness_   (model.h:264) */
  double tip_force_calculated[3];          /* Leg::tip_force_calculated_ (model.cpp:706, low-pass filter state) */
  double swing_progress, stance_progress;  /* LegStepper::swing_progress_ / stance_progress_ (walk_controller.h:498-499) */
  int32_t step_state;                      /* SHC_STEP_* */
  int32_t phase;                           /* LegStepper::phase_ */
  int32_t at_correct_phase, completed_first_step; /* walk_controller.h:493-494 */
  int32_t negate_auto_pose;                /* LegPoser::negate_auto_pose_ (pose_controller.h:575) */
  int32_t ik_failed;                       /* the 5 mm deviation warning of the last applyIK (model.cpp:921) */
  int32_t tip_rotation_defined;            /* current_tip_pose_.rotation_ != UNDEFINED_ROTATION */
  int32_t step_plane_defined;              /* Leg::step_plane_pose_ != Pose::Undefined() (touchdown detection, model.cpp:712-722) */
  double step_plane_position[3];           /* Leg::step_plane_pose_.position_ (robot frame; only its position is read, walk_controller.cpp:1088) */
  /* LegStepper::target_tip_pose_.rotation_ (> 3 DOF): the identity tip rotation with gravity_aligned_tips, UNDEFINED otherwise - until an
   * externally requested target (rough terrain mode) assigns its own, which then stays (walk_controller.cpp:1070 assigns the whole
   * pose, :1044 only the position).  Kept, like the other tip rotations, as the rotated x axis + "defined". */
  double target_tip_direction[3];
  int32_t target_rotation_defined;
  int32_t pad_;
} shc_leg_snapshot;

typedef struct shc_instance_state {
  double desired_linear_velocity[2], desired_angular_velocity; /* walk_controller.h:257-258 */
  double walk_plane[3], walk_plane_normal[3];                   /* WalkController::walk_plane_ / walk_plane_normal_ (:255-256) */
  double stepper_walk_plane[3], stepper_walk_plane_normal[3];   /* the copies the stepping LegSteppers took last cycle (:509-510) */
  double origin_walk_plane_pose[7];   /* PoseController::origin_walk_plane_pose_ (x,y,z,qw,qx,qy,qz) */
  double manual_pose[7];              /* PoseController::manual_pose_ */
  double translation_velocity_input[3], rotation_velocity_input[3]; /* pose_controller.h:285-286 (rewritten by the reset modes) */
  double rotation_absement_error[3], rotation_velocity_error[3];    /* IMU PID state (pose_controller.h:315-317) */
  double auto_pose_rotation[4];       /* PoseController::auto_pose_.rotation_ of the last cycle (w,x,y,z) */
  double current_pose[7];             /* Model::current_pose_ */
  double odometry[7];                 /* WalkController::odometry_ideal_ */
  double tip_align_pose[7], origin_tip_align_pose[7]; /* PoseController::tip_align_pose_ / origin_tip_align_pose_ (pose_controller.h:286-287) */
  int32_t walk_state;                 /* SHC_WALK_* */
  int32_t legs_at_correct_phase, legs_completed_first_step, return_to_default_attempted; /* walk_controller.h:266-268 */
  int32_t auto_posing_state;          /* SHC_POSING .. SHC_POSING_COMPLETE */
  int32_t pose_phase;                 /* PoseController::pose_phase_ (auto posing on its own clock) */
  /* AutoPoser latches, one word per poser: bit 0 start_check_, bit 1 end_check_.first, bit 2 end_check_.second, bit 3 allow_posing_ */
  int32_t auto_poser_flags[SHC_MAX_AUTO_POSERS];
  int32_t touchdown_detection;        /* LegStepper::touchdown_detection_ (walk_controller.h:495): tip-state messages have arrived */
  int32_t pad_;                       /* explicit: the record has no implicit padding (byte-comparable) */
  shc_leg_snapshot leg[SHC_MAX_LEGS];
} shc_instance_state;

/*
 * Auxiliary state: what only the calls AROUND the control cycle keep and shc_instance_state therefore does not carry - the pose
 * reset mode in force, manual leg manipulation (per-leg LegState, the leg selections and their inputs, Leg::desired_tip_pose_ as
 * the next WalkController::updateManual reads it back), externally requested targets / default poses / planner targets
 * (ExternalTarget records with their defined flags), the PoseController / LegPoser members of the start-up, shut-down and planner
 * sequences (transition steps, learnt transition poses, plan step, target configuration / body pose), the LegPoser origin poses of
 * stepToPosition / transitionConfiguration, and the measured joint positions of the last joint-state message.
 * One opaque, versioned blob per instance (its layout is private to the library and tied to the engine's legs x joints;
 * shc_engine_aux_state_bytes gives the size).  A COMPLETE checkpoint of an engine - restore, or migration into another engine of
 * the same parameters - is shc_engine_get_state + shc_engine_get_aux_state (+ the engine-wide scalars the host chose itself:
 * planner mode, pack step); restoring only the first leaves a robot with a MANUAL leg, a pending external target or a half-run
 * sequence without that state.  Held inputs (velocity, IMU, forces, efforts) are inputs: the caller applies them again.
 */
int64_t shc_engine_aux_state_bytes(const shc_engine *e);
int shc_engine_get_aux_state(shc_engine *e, int64_t first, int64_t count, void *blobs);
int shc_engine_set_aux_state(shc_engine *e, int64_t first, int64_t count, const void *blobs);

/*
 * Externally requested tip targets / default stance poses of rough terrain mode: struct ExternalTarget (walk_controller.h:38-46)
 * as targetTipPoseCallback (state_controller.cpp:1706-1767) fills it from syropod_highlevel_controller/TargetTipPose and
 * generateExternalTargetTransforms (:703-773) refreshes its transform_ from the tf tree every loop.  While a leg swings, a
 * defined target replaces the stepper's default target: target_tip_pose_ = pose_.removePose(transform_), the swing clearance
 * takes the requested height, and a target given in the "odom_ideal" frame is led by the body's ideal odometry over the rest
 * of the swing (walk_controller.cpp:1068-1079); the request is dropped at the start of the next stance period (:1159).  A
 * defined default replaces the terrain-following default tip pose at every swing / stance start (:988-990) until another one
 * arrives.  Only rough_terrain_mode reads either.  The tf lookup itself stays with the node.
 */
typedef struct shc_external_target {
  double pose[7];          /* ExternalTarget::pose_ (x,y,z,qw,qx,qy,qz); an all-zero quaternion = UNDEFINED_ROTATION */
  double transform[7];     /* ExternalTarget::transform_; the callback stores the identity (:1732), the tf refresh updates it */
  double swing_clearance;  /* ExternalTarget::swing_clearance_ (0 for a default pose) */
  int32_t frame_is_odom_ideal; /* frame_id_ == "odom_ideal" (:1073) */
  int32_t defined;         /* ExternalTarget::defined_; 0 withdraws the request */
} shc_external_target;
enum { SHC_EXTERNAL_TARGET = 0, SHC_EXTERNAL_DEFAULT = 1, SHC_EXTERNAL_PLANNER_TARGET = 2 /* LegPoser::external_target_, see planner mode */ };
/* LegStepper::setExternalTarget / setExternalDefault for legs `leg` (-1 = all, rows [count][legs]) of instances [first, first +
 * count); rows is a HOST array.  As in the callback (:1734-1757), a LegStepper takes a request only while its robot is not
 * STOPPED; the TARGET of a robot that stands goes to its LegPoser for planner mode (and raises target_tip_pose_acquired_, see
 * shc_engine_execute_plan), a DEFAULT for it is dropped.  Dropped rows are counted in *ignored (may be NULL): defaults for
 * standing robots and stepper requests without rough_terrain_mode (no stepper reads them).  The stepper keeps only the x axis of tip rotations (see
 * shc_leg_snapshot), and legs with <= 3 joints none at all.  On > 3-DOF legs a requested target rotation becomes
 * LegStepper::target_tip_pose_.rotation_ (walk_controller.cpp:1070 assigns the whole pose): updateTipRotation blends the tip towards
 * it over the back half of the swing, Leg::applyIK solves for it (rotation-constrained pass + unconstrained retry) - and, as in the
 * reference, it STAYS the leg's target rotation after the request is dropped (:1044 re-assigns only the position), replacing the
 * identity tip rotation of gravity_aligned_tips; a request with UNDEFINED_ROTATION clears it.
 * which = SHC_EXTERNAL_PLANNER_TARGET addresses the LegPoser's record directly (set: whatever the walk state). */
int shc_engine_set_external_target(shc_engine *e, int which, int64_t first, int64_t count, int leg, const shc_external_target *rows,
                                   int64_t *ignored);
/* generateExternalTargetTransforms: new transform_ rows (x,y,z,qw,qx,qy,qz) for requests that are currently defined. */
int shc_engine_set_external_transform(shc_engine *e, int which, int64_t first, int64_t count, int leg, const double *transform);
/* The requests as the steppers hold them now (defined_ cleared where a swing has consumed the target). */
int shc_engine_get_external_target(shc_engine *e, int which, int64_t first, int64_t count, int leg, shc_external_target *rows);

/*
 * Planner mode: StateController::executePlan (state_controller.cpp:653-698), the branch of runningState (:401-405) that replaces
 * the walking cycle while planner_mode_ is on.  The planner answers the node's request for plan step N with either a joint
 * configuration (target_configuration -> PoseController::transitionConfiguration(5.0), pose_controller.cpp:710-763: every named
 * leg moves on LegPoser::transitionConfiguration's cubic Bezier) or tip targets and / or a body pose (TargetTipPose for a robot that
 * stands, target_body_pose -> PoseController::transitionStance(5.0), :767-807: LegPoser::stepToPosition to the target while the
 * body eases to the pose, Leg::setDesiredTipPose + applyIK every iteration).  Requires what manual leg manipulation requires of
 * the posing modes; gravity_aligned_tips is SHC_ERR_UNSUPPORTED.
 */
enum { SHC_PLAN_WALKING = -1, SHC_PLAN_WAITING = -2 };
/* plannerModeCallback (:1262-1281): switching it on resets plan_step_ of every instance. */
int shc_engine_set_planner_mode(shc_engine *e, int on);
/* targetConfigurationCallback (:1683-1687) for instances [first, first + count): rows [count][legs][dof] (HOST); a leg whose first
 * entry is NaN is not named in the message and stays where it is.  (A leg the message names partly takes UNASSIGNED_VALUE for the
 * joints it omits in the reference; name whole legs.) */
int shc_engine_set_target_configuration(shc_engine *e, int64_t first, int64_t count, const double *configuration);
/* targetBodyPoseCallback (:1691-1702): rows [count][7] (x,y,z,qw,qx,qy,qz), HOST.  (The reference leaves target_body_pose_
 * uninitialised until the first plan step has completed; here it starts as the identity.) */
int shc_engine_set_target_body_pose(shc_engine *e, int64_t first, int64_t count, const double *pose);
/* One StateController::loop() in planner mode for EVERY instance.  A robot that stands runs executePlan: progress[i] = 0 .. 100 of
 * the plan step being executed (100: plan_step_ advances, the acquired flags and the target body pose are reset), or
 * SHC_PLAN_WAITING when nothing has been acquired (the node republishes its request for plan_step[i]; Model::updateModel runs,
 * :666).  A robot that is still walking gets SHC_PLAN_WALKING, its velocity inputs are zeroed (:691-697) and its loop is one
 * ordinary control cycle, launched by this call for those robots only.  progress / plan_step: HOST [n], may be NULL. */
int shc_engine_execute_plan(shc_engine *e, int32_t *progress, int32_t *plan_step);

int64_t shc_sizeof_instance_state(void);
/* Instances [first, first + count) -> states[0 .. count) (host array).  Synchronises the engine's stream.  Read-only: a change made by
 * shc_engine_adjust_parameter that waits for the next loop stays pending (the legs' phases and progress are reported in the step cycle they still
 * count in), so a snapshot taken between the two does not change the run. */
int shc_engine_get_state(shc_engine *e, int64_t first, int64_t count, shc_instance_state *states);
/* states[0 .. count) (host array) -> instances [first, first + count).  Inputs (velocity, IMU, forces, efforts, pose
 * inputs' reset mode) are not part of the state and stay as set.  A pending shc_engine_adjust_parameter stays pending: injected phases
 * count in the old step period and are mapped onto the new one inside the next loop, as those of the replaced state would have been. */
int shc_engine_set_state(shc_engine *e, int64_t first, int64_t count, const shc_instance_state *states);

/*
 * Device checkpoints: the state of every instance kept in device memory, and an indexed restore from it - reset any subset of the batch to a
 * known state, or clone one instance onto many, while the others keep walking.  Everything runs on the engine's stream.
 * The host route above defines the result: after a restore with source[i] = j, shc_engine_get_state(i) and shc_engine_get_aux_state(i) return
 * what they would return had the caller read instance j's records at capture time and written them to i with shc_engine_set_state /
 * shc_engine_set_aux_state at restore time, and every later cycle is that engine's bit for bit.  Held inputs (velocity, IMU, forces, efforts)
 * are inputs: a restored instance keeps the command it is being given now.  The engine-wide facts the host route derives from injected records
 * (manual pose live, touchdown detection, manual legs, external targets, joint efforts live, "the LegPoser tips of the last plan call are
 * current") are taken from the checkpoint as captured; nothing is read back from the device.
 * A checkpoint belongs to the engine that made it (another engine's: SHC_ERR_INVALID_ARG) and to the gait and parameters it was captured
 * under: after shc_engine_change_gait or shc_engine_adjust_parameter, and while an adjusted parameter waits for its loop, a restore is
 * SHC_ERR_UNSUPPORTED and changes nothing - step, then shc_engine_checkpoint_update.  shc_engine_destroy releases the device memory of the
 * engine's checkpoints; their handles stay valid only for shc_checkpoint_destroy (every other use: SHC_ERR_INVALID_ARG).
 * Split steps are joined first; SHC_ERR_BUSY in resident mode.  Fleets have the same calls in the caller's instance order
 * (shc_fleet_checkpoint_*, shc_fleet_restore_instances, shc_fleet_scan_and_restore below); migration between engines stays on the host route.
 */
typedef struct shc_checkpoint shc_checkpoint;
/* Allocates the checkpoint's device arrays (the size of the engine's state planes and records), then captures as shc_engine_checkpoint_update. */
int shc_engine_checkpoint_create(shc_engine *e, shc_checkpoint **out);
/* Captures the engine's state as of this point of its stream into the same storage: device-to-device copies on the engine's stream, no host
 * wait, no allocation - unless the engine has grown a record array since (first leg toggle, first external request, first sequence call):
 * then the checkpoint grows with it, once. */
int shc_engine_checkpoint_update(shc_engine *e, shc_checkpoint *ck);
/* Waits for the engine's stream (a capture or restore may be in flight), then frees the checkpoint.  NULL: SHC_ERR_INVALID_ARG. */
int shc_checkpoint_destroy(shc_checkpoint *ck);
/* Instance i <- the checkpoint's instance source[i], one kernel launch.  source[i] < 0 or >= n: instance i is left exactly as it is.
 * source: [n] int64, HOST (on_device = 0; validated first: an entry >= n is SHC_ERR_INVALID_ARG and nothing is changed; synchronises the
 * engine's stream) or DEVICE (on_device = 1; read on the engine's stream - the caller's writes to it must be ordered before this call on
 * that stream - no host wait, no allocation; an entry >= n leaves its instance alone).  NULL = the identity (restore everything).
 * A map is not a list of pairs: it cannot name one destination twice.  Reset from a device-side mask is where(done, arange(n), -1).
 * Only NULL or a host map without negative entries counts as a restore of the whole batch for "the LegPoser tips are current"
 * (see shc_engine_set_aux_state: a partial restore never raises it). */
int shc_engine_restore_instances(shc_engine *e, const shc_checkpoint *ck, const int64_t *source, int on_device);
/* Device bytes the checkpoint holds (0 for NULL, and once its engine has been destroyed). */
int64_t shc_checkpoint_bytes(const shc_checkpoint *ck);
/* Development: the class of leg field `field` of joints-per-leg `nj` (is_robot = 0) or of robot field `field` (is_robot = 1) in the
 * checkpoint's classification - 0 state, 1 input (not restored), 2 output, 3 LDS-only (not restored) - or -1 for an index outside the
 * field list or not classified exactly once.  No device needed. */
int shc_debug_checkpoint_field_class(int nj, int is_robot, int field);

/*
 * Health scan: what the reference reports as throttled ROS_WARN lines of ONE robot - "IK Clamping Event/s" (Leg::updateJointPositions,
 * model.cpp:811-853), "Inverse kinematics deviation!" (Leg::applyIK, :914-929) and the limit proximity the two return (:843-849, :903, :940) -
 * as one record per robot, and the robots that meet a caller's criteria as a restore map and an ascending list: step -> scan -> restore
 * (shc_engine_restore_instances, on_device = 1) without a host round trip.  Everything is a function of the stored state; joints are a
 * leg's own (a leg shorter than the robot's longest has no others).
 */
enum {
  SHC_HEALTH_IK_DEVIATION = 1,   /* a leg carries the 5 mm deviation warning of its last applyIK (model.cpp:916-929): leg_status bit 2 of
                                    shc_engine_get_leg_state, shc_leg_snapshot.ik_failed */
  SHC_HEALTH_POSITION_LIMIT = 2, /* a joint of non-zero range stands with desired_position_ <= min or >= max: what a position clamp leaves
                                    behind (model.cpp:827-841) */
  SHC_HEALTH_SPEED_LIMIT = 4,    /* max_speed_ratio >= 1: what a velocity clamp leaves behind (model.cpp:812-821) */
  SHC_HEALTH_NEAR_LIMIT = 8,     /* min_limit_proximity < criteria.near_limit_proximity */
  SHC_HEALTH_TIP_DEVIATION = 16, /* max_tip_deviation > criteria.tip_deviation */
  SHC_HEALTH_NONFINITE = 32      /* a joint angle or rate, walker / poser / model tip, admittance delta or component of
                                    Model::current_pose_ is NaN or +-Inf; the three doubles of such a record are unspecified */
};
typedef struct shc_health_criteria {
  uint32_t select;             /* SHC_HEALTH_* bits: a robot is selected when flags & select != 0 */
  uint32_t reserved;           /* 0 */
  double near_limit_proximity; /* threshold of SHC_HEALTH_NEAR_LIMIT, in the units of Leg::updateJointPositions' return value (1 = mid-range, 0 = on a limit) */
  double tip_deviation;        /* threshold of SHC_HEALTH_TIP_DEVIATION, metres (the reference warns above IK_TOLERANCE = 0.005, model.h:17) */
} shc_health_criteria;
typedef struct shc_robot_health { /* 32 bytes, no padding */
  double min_limit_proximity; /* Leg::updateJointPositions' return value (model.cpp:843-849) evaluated on the stored desired_position_: the minimum over
                                 legs and joints of min(|min - q|, |max - q|) / ((max - min) / 2); a zero-range joint contributes 1.0 (:848) */
  double max_tip_deviation;   /* the maximum over legs and axes of |current_tip_pose_ - desired_tip_pose_| (model.cpp:918) with desired_tip_pose_ =
                                 poser tip + admittance_delta_ (setDesiredTipPose, :660-661; no delta for MANUAL / WALKING_TO_MANUAL legs, :656): the
                                 model_tip, poser_tip and admittance rows of shc_engine_get_leg_state */
  double max_speed_ratio;     /* the maximum over legs and joints of |desired_velocity_| / max_angular_speed_ (model.cpp:814) */
  uint32_t flags;             /* SHC_HEALTH_* */
  uint32_t leg_masks;         /* byte 0: legs with the IK deviation bit, 1: on a position limit, 2: on the speed limit, 3: non-finite; bit l = leg l */
} shc_robot_health;
/* Instances [first, first + count) in one device pass.  Any output may be NULL (not all four):
 *   health       [count]  the records
 *   restore_map  [n]      i for a selected robot of the range, -1 for every other i of [0, n): the source map of
 *                         shc_engine_restore_instances(.., on_device = 1)
 *   selected     [count]  the selected instance ids in ascending order; entries past the count are left untouched
 *   n_selected   [1]      their number
 * criteria is HOST memory; NULL = select 0, thresholds unused (NEAR_LIMIT / TIP_DEVIATION are never raised).
 * on_device = 1: the outputs are device buffers (health 16-byte aligned, the int64 buffers 8-byte aligned), the call is ordered on the engine's
 * stream and does not wait on the host; on_device = 0: host memory, the call synchronises the stream.  Split steps are joined first.  Refreshes
 * the derived model / poser tips as shc_engine_get_leg_state does and changes no other state.  count = 0 writes *n_selected = 0 and a
 * restore_map of -1.  The pass keeps one small count buffer per engine, allocated by the engine's first scan (like
 * shc_engine_checkpoint_create, that call allocates device memory; later device-form calls do not) and freed by shc_engine_destroy.
 * SHC_ERR_INVALID_ARG for a range outside [0, n), all outputs NULL, reserved != 0, select bits outside the six, misaligned device buffers;
 * SHC_ERR_BUSY in resident mode. */
int shc_engine_scan_health(shc_engine *e, int64_t first, int64_t count, const shc_health_criteria *criteria, shc_robot_health *health /* [count] */,
                           int64_t *restore_map /* [n] */, int64_t *selected /* [count] */, int64_t *n_selected /* [1] */, int on_device);
/* Development: the record of ONE robot of parameters `params` from host arrays in the layouts of the getters - q, qd [legs][longest leg's DOF],
 * poser_tip, model_tip, admittance [legs][3], leg_status [legs] (bit 2 = IK deviation), pose7 = Model::current_pose_ (x,y,z,qw,qx,qy,qz) - through the
 * functions the scan kernel runs (the walker tip and the manual leg states are not part of it: finite, WALKING).  criteria may be NULL.  No device needed. */
int shc_debug_robot_health(const shc_params *params, const shc_health_criteria *criteria, const double *q, const double *qd, const double *poser_tip,
                           const double *model_tip, const double *admittance, const int32_t *leg_status, const double *pose7, shc_robot_health *out);

/*
 * Fleets: mixed morphologies (BASELINE.json configs[4]) and several GPUs of one node (configs[3]) behind one handle, for hosts
 * that drive all devices from ONE process (a one-process-per-GPU host creates one engine per rank and exchanges with RCCL, see
 * bench.py).  morph_id[i] in [0, n_morphologies) assigns instance i to params[morph_id[i]] (NULL = all 0).  Instances are binned
 * by morphology - the cycle kernel keeps one morphology's tables in LDS and maps one leg to one lane - and every bin is split
 * into contiguous shards over device_ids[0 .. n_devices) (NULL / 0 = device 0); each (bin, device) part is an engine on its own
 * HIP stream.  Nothing is exchanged while stepping.  All arrays are HOST arrays in the CALLER's instance order; per-leg arrays
 * are padded to [n][max_legs][max_k] (shc_fleet_shape), outputs are NaN where a morphology has no such leg / joint.  The same calls
 * with DEVICE arrays, for a caller that lives on the GPU: shc_fleet_set_inputs_device / shc_fleet_get_outputs_device below.
 */
typedef struct shc_fleet shc_fleet;
int shc_fleet_create(const shc_params *params, int n_morphologies, const int32_t *morph_id, int64_t n_instances, const int *device_ids,
                     int n_devices, shc_fleet **out);
int shc_fleet_destroy(shc_fleet *f);
int64_t shc_fleet_instances(const shc_fleet *f);
int shc_fleet_shape(const shc_fleet *f, int *max_legs, int *max_dof);
/* The parts (one engine per (morphology bin, device)): for device-resident I/O through the shc_engine_* calls. */
int shc_fleet_part_count(const shc_fleet *f);
int shc_fleet_part(const shc_fleet *f, int k, shc_engine **engine, int *morphology, int *device, int64_t *n_instances);
int shc_fleet_part_instances(const shc_fleet *f, int k, int64_t *ids /* [n_instances of part k]: caller's instance ids, ascending */);
int shc_fleet_set_velocity(shc_fleet *f, const double *linear_xy /* [n][2] */, const double *angular /* [n] */);
int shc_fleet_set_imu(shc_fleet *f, const double *orientation_wxyz /* [n][4] */, const double *angular_velocity /* [n][3] */);
int shc_fleet_set_pose_input(shc_fleet *f, const double *translation_velocity /* [n][3] */, const double *rotation_velocity /* [n][3] */);
int shc_fleet_set_tip_force(shc_fleet *f, const double *tip_force /* [n][max_legs][3] */);
int shc_fleet_set_joint_effort(shc_fleet *f, const double *joint_effort /* [n][max_legs][max_dof] */);
int shc_fleet_step(shc_fleet *f, int n_cycles);
int shc_fleet_synchronize(shc_fleet *f);
int shc_fleet_get_joint_state(shc_fleet *f, double *q, double *qd /* [n][max_legs][max_dof], either may be NULL */);
int shc_fleet_get_walk_state(shc_fleet *f, int32_t *walk_state /* [n] */);
/* publishLegState of every robot of the fleet, in the caller's instance order: msgs[i * max_legs + l] (host memory); the records of
 * legs a robot does not have are all zero.  Synchronises every part's stream. */
int shc_fleet_get_leg_state_msgs(shc_fleet *f, shc_leg_state_msg *msgs);
/* publishFrameTransforms of every robot of the fleet, in the caller's instance order (host memory): legs[i * max_legs + l], the records of
 * legs a robot does not have all zero, and body[i]; either may be NULL (not both).  Synchronises every part's stream. */
int shc_fleet_get_frame_transforms(shc_fleet *f, int frame, shc_leg_frames *legs /* [n][max_legs] */, shc_body_frames *body /* [n] */);
/* shc_engine_scan_health of every robot of the fleet: the records in the caller's instance order (host memory; criteria may be NULL).  Records only -
 * shc_fleet_scan_and_restore below resets the selected robots in the same pass; selected lists are per engine (shc_fleet_part).  Synchronises
 * every part's stream. */
int shc_fleet_scan_health(shc_fleet *f, const shc_health_criteria *criteria, shc_robot_health *health /* [n] */);
/*
 * Fleet checkpoints: the device checkpoints of every part behind one handle, and maps in the CALLER's instance order.  A fleet checkpoint is one
 * shc_checkpoint per part, made, captured and restored through the shc_engine_* calls above on the part's own stream: everything said there
 * about what a restore moves, about held inputs and about the engine-wide facts holds part by part.  The fleet's FIRST shc_fleet_checkpoint_create
 * also allocates what the calls below work with - per part a small block on its device (its caller ids, its restore map, health records, a count)
 * and, when one device holds every part, the tables caller id -> (part, id within the part) on that device - and uploads it synchronously; no
 * later call allocates anything but a new checkpoint's own arrays.
 * A handle belongs to its fleet: with another fleet, or once its fleet has been destroyed, every use but shc_fleet_checkpoint_destroy is
 * SHC_ERR_INVALID_ARG.  shc_fleet_destroy releases the device memory of the fleet's checkpoints, as shc_engine_destroy does for an engine's.
 * Errors of the parts pass through unchanged - SHC_ERR_UNSUPPORTED after shc_engine_change_gait / shc_engine_adjust_parameter on a part (step,
 * then shc_fleet_checkpoint_update), SHC_ERR_BUSY while a part is in resident mode - and every part is asked before the first launch: when one
 * part refuses, no part has changed, whichever robots the call named.
 */
typedef struct shc_fleet_checkpoint shc_fleet_checkpoint;
int shc_fleet_checkpoint_create(shc_fleet *f, shc_fleet_checkpoint **out);
/* shc_engine_checkpoint_update of every part, on its stream: no host wait. */
int shc_fleet_checkpoint_update(shc_fleet *f, shc_fleet_checkpoint *ck);
/* shc_checkpoint_destroy of every part's checkpoint (waits for the part's stream while the fleet lives), then frees the handle.  NULL: SHC_ERR_INVALID_ARG. */
int shc_fleet_checkpoint_destroy(shc_fleet_checkpoint *ck);
/* Device bytes the parts' checkpoints hold (0 for NULL, and once the fleet has been destroyed). */
int64_t shc_fleet_checkpoint_bytes(const shc_fleet_checkpoint *ck);
/* Instance i <- the checkpoint's instance source[i], both in the caller's order; source[i] < 0 leaves instance i exactly as it is; NULL = the
 * identity (restore everything, either form).  The result is the engine route's: instance i's slot of its part reads back
 * (shc_engine_get_state / shc_engine_get_aux_state) as after the part's own shc_engine_restore_instances with the translated map.
 * A source must be of its destination's part.  Another morphology is another layout; another part of the same morphology (another device's
 * shard of the bin) would need a peer copy of checkpoint rows, which is not implemented.
 * HOST map (on_device = 0): validated as a whole first - an entry >= n or of another morphology is SHC_ERR_INVALID_ARG, an entry of another
 * part of the same morphology SHC_ERR_UNSUPPORTED, and nothing has changed - then split into the parts' maps on the host and restored with
 * one launch per part that has a non-negative entry (the engine's host form: that part's stream is synchronised); a part the map does not
 * name is not touched and its stream is not waited for.
 * DEVICE map (on_device = 1): [n] int64 on the device that holds EVERY part of the fleet; a fleet that spans devices answers
 * SHC_ERR_UNSUPPORTED (use the host form).  Each part translates its slice on its own stream directly before its restore: no host wait, no
 * allocation.  The parts' streams are the fleet's own and nothing orders them behind a stream of the caller's: the caller's writes to `source`
 * must be COMPLETE before the call (synchronise the stream that wrote it), and the buffer must stay untouched until the parts have read it
 * (shc_fleet_synchronize, or any later synchronising call).  An entry that is out of range, of another morphology or of another part leaves
 * its destination alone, as an entry >= n does in the engine's device form. */
int shc_fleet_restore_instances(shc_fleet *f, const shc_fleet_checkpoint *ck, const int64_t *source /* [n], CALLER's instance ids */, int on_device);
/* step -> scan -> restore for a fleet, no map crossing the host: on every part's stream shc_engine_scan_health(.., restore_map = the part's own map
 * buffer, on_device = 1), then shc_engine_restore_instances(.., that buffer, on_device = 1) - the robots that meet `criteria` are reset to the
 * checkpoint, the others keep walking.  criteria = NULL (or select = 0) selects nobody: a scan and nothing else.  health ([n], HOST, caller's order,
 * may be NULL) receives the records as shc_fleet_scan_health fills them - the records BEFORE the restore; n_restored (HOST, may be NULL) the sum
 * of the parts' selected counts.  Asking for either synchronises every part's stream; with both NULL the call returns without waiting.
 * The scan refreshes the derived model / poser tips as shc_engine_scan_health does - from the state BEFORE the restore: a restored robot's
 * are refreshed by the next getter or scan, as after shc_engine_restore_instances. */
int shc_fleet_scan_and_restore(shc_fleet *f, const shc_fleet_checkpoint *ck, const shc_health_criteria *criteria,
                               shc_robot_health *health /* [n] host, caller order, may be NULL */, int64_t *n_restored /* host, may be NULL */);
/*
 * Fleet device I/O: the setters and getters above with DEVICE arrays in the CALLER's instance order, for a simulator or learner whose commands
 * and observations never leave the GPU.  Nothing crosses the host: per part and direction one kernel on the part's own stream permutes between
 * the caller's padded order and the part's dense order, and the engine's own device forms (shc_engine_set_*(.., on_device = 1), shc_engine_get_*
 * (.., on_device = 1)) stand between that and the state.
 * shc_fleet_set_inputs_device leaves every robot's state, and every engine-side fact a setter touches (touchdown detection and its step planes
 * in rough terrain mode, the first-effort switch, the manual-posing switch, quaternion normalisation), exactly as shc_fleet_set_velocity /
 * _set_imu / _set_pose_input / _set_tip_force / _set_joint_effort with host copies of the same arrays do.  A NULL member holds that input.
 * shc_fleet_get_outputs_device writes, member by member, the bytes shc_fleet_get_joint_state / _get_walk_state / _get_leg_state_msgs /
 * _get_frame_transforms / _scan_health write to host arrays, padding included (the NaN of q / qd, all-zero records of legs a robot does not
 * have): every entry of every requested buffer is written by every call.  The derived model / poser tips are refreshed as those getters do.
 * Staging (per part: its rows of all inputs, or of one joint array, or one chunk of records) and the parts' caller ids on the device are
 * allocated by the fleet's first device I/O call and kept; no later call allocates.  Record outputs (leg messages, frames, health) walk each
 * part in chunks of shc_fleet_set_io_chunk robots (0 = the default, 8 192), so staging does not grow with the records of the whole fleet;
 * changing the chunk waits for the parts and lets the next call allocate again.  shc_fleet_io_bytes: the device bytes held - the staging, and the parts' ids from
 * the moment any of their three users (device I/O, checkpoints, the exchange step) has uploaded them; 0 before that.
 * Every part is asked before the first launch: SHC_ERR_BUSY while a part is in resident mode, and nothing has changed.  A fleet that spans
 * devices answers SHC_ERR_UNSUPPORTED to the four device entry points (the caller's arrays live on one device, as the device map of
 * shc_fleet_restore_instances; the host forms remain).  SHC_ERR_INVALID_ARG: NULL fleet or struct, every output NULL, reserved != 0, an unknown
 * frame, a record buffer that is not 16-byte aligned (as the engine forms require), criteria the scan refuses.  SHC_ERR_UNSUPPORTED passes
 * through from a part without SHC_FEAT_ODOMETRY when body_frames or SHC_FRAME_ODOM_IDEAL is asked for.  pose_reset_mode stays on the part
 * route (shc_fleet_part, shc_engine_set_pose_reset_mode).
 * STREAMS.  The parts' streams are the fleet's own.  Without the two ordering calls the rule is the one of shc_fleet_restore_instances' device
 * map: the caller's writes to the input arrays must be COMPLETE before the call, the arrays must stay untouched until the parts have read them
 * (shc_fleet_synchronize), and the outputs are complete after shc_fleet_synchronize.  With them no host wait is needed:
 *   shc_fleet_order_after_stream(f, s)   every part's stream waits for what is queued on `s` now (inputs written by kernels on s);
 *   shc_fleet_order_stream_after(f, s)   `s` waits for what is queued on every part's stream now; parts with split steps in flight are joined
 *                                        first (shc_engine_join).
 * i.e. order_after_stream(s) -> set inputs -> step -> get outputs -> order_stream_after(s) -> the caller's kernels on s.  Both are events only,
 * one per part and direction, created at first use with timing disabled.  stream = NULL is the default stream.
 */
typedef struct shc_fleet_inputs {              /* DEVICE arrays, CALLER's instance order; NULL member = that input is held */
  const double *linear_xy;                     /* [n][2] */
  const double *angular;                       /* [n] */
  const double *imu_orientation_wxyz;          /* [n][4], normalised on entry as shc_engine_set_imu does */
  const double *imu_angular_velocity;          /* [n][3] */
  const double *pose_translation_velocity;     /* [n][3] */
  const double *pose_rotation_velocity;        /* [n][3] */
  const double *tip_force;                     /* [n][max_legs][3];       entries beyond a robot's legs are ignored */
  const double *joint_effort;                  /* [n][max_legs][max_dof]; entries beyond a bin's (legs, dof) are ignored */
} shc_fleet_inputs;
int shc_fleet_set_inputs_device(shc_fleet *f, const shc_fleet_inputs *in);
typedef struct shc_fleet_outputs {             /* DEVICE buffers, CALLER's instance order; NULL member = not asked for (not all NULL) */
  double *q, *qd;                              /* [n][max_legs][max_dof]: exactly the array shc_fleet_get_joint_state fills, NaN padding included */
  int32_t *walk_state;                         /* [n] */
  shc_leg_state_msg *leg_state_msgs;           /* [n][max_legs]; records of legs a robot does not have all zero */
  shc_leg_frames *leg_frames;                  /* [n][max_legs]; same rule */
  shc_body_frames *body_frames;                /* [n] */
  int32_t frame;                               /* SHC_FRAME_* for leg_frames */
  int32_t reserved;                            /* 0 */
  shc_robot_health *health;                    /* [n] */
  const shc_health_criteria *criteria;         /* HOST, may be NULL: as shc_fleet_scan_health */
} shc_fleet_outputs;
int shc_fleet_get_outputs_device(shc_fleet *f, const shc_fleet_outputs *out);
int shc_fleet_order_after_stream(shc_fleet *f, void *stream);
int shc_fleet_order_stream_after(shc_fleet *f, void *stream);
int shc_fleet_set_io_chunk(shc_fleet *f, int64_t robots);      /* staging granularity of the record outputs, robots per part; 0 = default */
int64_t shc_fleet_io_bytes(const shc_fleet *f);                /* device bytes the I/O path holds (ids, staging); 0 before first use */
/*
 * Fleet step_k: shc_engine_step_k for a mixed fleet - K cycles per launch, cycle k with row k of K-deep DEVICE arrays in the CALLER's instance
 * order.  `rows` is a shc_fleet_inputs whose non-NULL members hold K rows, each padded exactly as for shc_fleet_set_inputs_device: linear_xy
 * [K][n][2], angular [K][n], imu_orientation_wxyz [K][n][4], imu_angular_velocity [K][n][3], tip_force [K][n][max_legs][3], joint_effort
 * [K][n][max_legs][max_dof].  A NULL member - or rows = NULL: every member - is held at what the parts have; the velocity pair and the IMU pair
 * are given together, as the engine requires; the two pose members must be NULL (SHC_ERR_UNSUPPORTED: set them beforehand, they are held for the
 * K cycles).
 * DEFINITION.  After the call every robot's state record, auxiliary blob and held inputs, and the q / qd of each of the K cycles, are byte for
 * byte what
 *   for k in 0 .. K - 1 { shc_fleet_set_inputs_device(row k); shc_fleet_step(f, 1); shc_fleet_get_outputs_device(q, qd) }
 * leaves and reads.  Per part and call one kernel gathers the part's rows of all K cycles into K-deep staging and one shc_engine_step_k runs them;
 * what that call documents is the part's own behaviour and passes through unchanged: the serial form for configurations without a batch kernel,
 * the first cycle through the serial form while an adjusted parameter is pending, touchdown detection on fresh tip forces inside the loop, the
 * first-effort switch, the last row becoming the held input.
 * shc_fleet_get_step_k_joints_device: q / qd of cycles [first_cycle, first_cycle + n_cycles) of the latest shc_fleet_step_k into DEVICE buffers
 * [n_cycles][n][max_legs][max_dof] (8-byte aligned; either may be NULL, not both) in the caller's order, NaN - the bit pattern
 * shc_fleet_get_joint_state writes - where a morphology has no such leg / joint.  Every entry of every requested buffer is written by every call:
 * per part and buffer one kernel reads the part's output ring where it lies.  Stream-ordered on the parts' streams (split launches are joined
 * first), no host wait.
 * STAGING.  The K-deep staging is a buffer of its own per part, sized K x the part's rows x the groups given; it is allocated by the first call
 * that needs it, grows when a call needs more (that call waits for the part), is kept, and is counted by shc_fleet_io_bytes: a later call with
 * the same or a smaller K and the same groups allocates nothing.  It does not depend on shc_fleet_set_io_chunk and stays across it.
 * STREAMS.  As for device I/O: order_after_stream(s) -> shc_fleet_step_k -> shc_fleet_get_step_k_joints_device -> order_stream_after(s).  The
 * caller's K-deep arrays are read by the gather kernel alone, on each part's stream, before the part's launch: they are free once that has run -
 * after order_stream_after(s) for work queued on s, or after shc_fleet_synchronize.  shc_engine_step_k's stricter rule (its arrays stay valid
 * until the engine is joined) applies to the fleet's own staging, not to the caller; a part whose launches run split on its two internal streams
 * is joined before the next call overwrites the staging.
 * REFUSALS.  Every part is asked before the first launch; when one refuses - the answers listed here - nothing has changed.  (A runtime error
 * of a part's own launch, SHC_ERR_HIP, can leave the parts before it stepped; the latest K then stays what it was.)  SHC_ERR_INVALID_ARG: NULL fleet; n_cycles
 * outside 1 .. 4096; half a pair; q and qd both NULL; a cycle range outside the latest call's K, or no call yet (or a part stepped through its own
 * shc_engine_step_k since); a misaligned buffer; a part whose output ring (the engine's bound) or whose K-deep staging would reach 2 GiB.
 * SHC_ERR_UNSUPPORTED: a fleet that spans devices (as the other device entry points), pose members, a part still starting up.  SHC_ERR_BUSY: a
 * part in resident mode.
 */
int shc_fleet_step_k(shc_fleet *f, int n_cycles, const shc_fleet_inputs *rows /* may be NULL: every input held */);
int shc_fleet_get_step_k_joints_device(shc_fleet *f, int first_cycle, int n_cycles, double *q, double *qd /* either may be NULL, not both */);
/*
 * Observation pass: chosen fields of every robot as one dense [rows][D] array of float64 or float32, for a learner that wants 40 - 120 numbers
 * per robot and not the whole records of the getters above.  One kernel per engine (per part of a fleet) evaluates only the fields asked for,
 * converts them to the element type and writes each robot's row where the caller's array wants it; nothing is staged.
 * ROW.  The fields of a spec follow each other in the order of `fields`.  A per-leg field of `width` columns per leg takes legs x width columns,
 * leg-major (leg l, component k at l * width + k; width = spec.dof for the joint fields); a per-robot field takes its width.  shc_obs_width is the
 * number of columns D, shc_obs_column the column of one component; neither needs a device.
 * DEFINITION.  Column c of robot i's row holds the double the getter named beside the field writes for that robot, leg and component - unchanged
 * for SHC_OBS_F64, static_cast<float> (round to nearest even) for SHC_OBS_F32.  `pad`, converted in the same way once on the host, is written
 * wherever the robot's morphology has no such leg or no such joint (leg >= its legs, joint >= its longest leg's DOF; the joints a shorter leg of a
 * mixed-DOF robot lacks hold what shc_engine_get_joint_state holds there).  Columns [width, row_stride) of a row are not touched.
 * SHC_OBS_MODEL_TIP / SHC_OBS_POSER_TIP are the values the derived-tip refresh of shc_engine_get_leg_state_msgs produces, derived inside the
 * pass from the same stored state by the same device functions, and only when one of the two is asked for; the pass WRITES NOTHING into an
 * engine: every robot's state record and auxiliary blob are byte for byte what they were.  SHC_OBS_ADMITTANCE_DELTA is zero with admittance
 * control off, as in shc_leg_state_msg.
 * shc_engine_get_observations: instances [first, first + count) into rows 0 .. count - 1 of `out` (host array, or device array with on_device =
 * 1, aligned to the element size).  on_device, stream ordering, the join of split steps and count = 0 (a no-op) are those of
 * shc_engine_get_leg_state_msgs.
 * shc_fleet_get_observations_device: every robot of the fleet into row i = its CALLER's instance id of the device array `out` ([n][row_stride]).
 * One kernel per part on the part's own stream reads the part's state and writes the caller's rows through the part's caller ids (the ids device
 * I/O keeps on the device): no staging, no allocation after the fleet's first device I/O call, shc_fleet_io_bytes unchanged.  The STREAMS rules
 * of device I/O and shc_fleet_order_after_stream / shc_fleet_order_stream_after apply as written there.
 * REFUSALS (nothing is launched; a fleet asks every part before the first launch).  SHC_ERR_INVALID_ARG: NULL handle, spec or out; n_fields
 * outside 1 .. SHC_OBS_MAX_FIELDS; an unknown or repeated field; an unknown dtype; reserved != 0; legs / dof below the engine's (legs, longest leg's
 * DOF) or the fleet's shc_fleet_shape, or above SHC_MAX_LEGS / SHC_MAX_JOINTS; row_stride non-zero and below the width; a range outside [0, n); a
 * buffer not aligned to the element size.  SHC_ERR_UNSUPPORTED: SHC_OBS_ODOM_TO_BASE_LINK on an engine or part without SHC_FEAT_ODOMETRY;
 * SHC_OBS_VIRTUAL_STIFFNESS with admittance control off (as shc_engine_get_virtual_stiffness); a fleet that spans devices.  SHC_ERR_BUSY: resident mode.
 */
enum { /* per-leg fields: `width` columns per leg, leg-major, for `legs` legs */
  SHC_OBS_Q, SHC_OBS_QD,            /* width dof: shc_engine_get_joint_state / shc_fleet_get_joint_state              */
  SHC_OBS_JOINT_EFFORT,             /* width dof: shc_leg_state_msg.joint_efforts                                     */
  SHC_OBS_WALKER_TIP, SHC_OBS_TARGET_TIP, SHC_OBS_POSER_TIP, SHC_OBS_MODEL_TIP,   /* 3: the *_tip_position members     */
  SHC_OBS_TIP_FORCE, SHC_OBS_ADMITTANCE_DELTA,                                      /* 3: tip_force (x force_gain), admittance_delta */
  SHC_OBS_VIRTUAL_STIFFNESS, SHC_OBS_STANCE_PROGRESS, SHC_OBS_SWING_PROGRESS, SHC_OBS_TIME_TO_SWING_END, /* 1 each: the shc_leg_state_msg members */
  SHC_OBS_STEP_STATE,               /* 1: bits 0-1 of shc_engine_get_leg_state's leg_status, as a number               */
  /* per-robot fields */
  SHC_OBS_BODY_POSE,                /* 7: shc_engine_get_body_state pose                                               */
  SHC_OBS_DESIRED_VELOCITY,         /* 3: shc_body_frames.desired_velocity                                             */
  SHC_OBS_POSE_EULER,               /* 3: shc_body_frames.pose_euler                                                   */
  SHC_OBS_ODOM_TO_BASE_LINK,        /* 7: shc_body_frames.odom_to_base_link (needs SHC_FEAT_ODOMETRY)                  */
  SHC_OBS_WALK_STATE,               /* 1: walk_state as a number                                                       */
  SHC_OBS_FIELD_COUNT
};
enum { SHC_OBS_F64 = 0, SHC_OBS_F32 = 1 };
#define SHC_OBS_MAX_FIELDS 32
typedef struct shc_obs_spec {
  int32_t n_fields, fields[SHC_OBS_MAX_FIELDS]; /* column order = this order; a field may appear once                 */
  int32_t dtype;                                /* SHC_OBS_F64 / SHC_OBS_F32                                           */
  int32_t legs, dof;                            /* row geometry; engine: >= its legs / longest leg's dof; fleet: >= shc_fleet_shape */
  int32_t reserved;                             /* 0 */
  int64_t row_stride;                           /* elements between rows; 0 = dense (= shc_obs_width); >= width otherwise */
  double pad;                                   /* written where a robot has no such leg or a leg no such joint        */
} shc_obs_spec;
int64_t shc_obs_width(const shc_obs_spec *spec);                       /* columns of a row; < 0 for an invalid spec; no device needed */
int shc_obs_column(const shc_obs_spec *spec, int field, int leg, int k); /* column of component k of `field` (leg ignored for robot fields); -1 if absent */
int shc_engine_get_observations(shc_engine *e, int64_t first, int64_t count, const shc_obs_spec *spec, void *out, int on_device);
int shc_fleet_get_observations_device(shc_fleet *f, const shc_obs_spec *spec, void *out /* [n][row_stride], caller's order */);
/*
 * Action pass: the observation pass turned round.  Chosen input groups of every robot taken from one dense [n][A] array of float64 or float32 -
 * what a policy emits - in one kernel per engine (per part of a fleet), which converts and scatters straight into the state; nothing is staged
 * and the array is never written.
 * ROW.  The rule of the observation pass: the fields of a spec follow each other in the order of `fields`; SHC_ACT_TIP_FORCE (width 3) and
 * SHC_ACT_JOINT_EFFORT (width spec.dof) take legs x width columns, leg-major; the other fields take their width (2, 1, 4, 3, 3, 3 in the order
 * of the enum).  The width of a row and the column of one component come from the two layout calls below; neither needs a device.
 * DEFINITION.  After the engine call the engine is byte for byte what the existing device setters (on_device = 1) leave when they are given
 * float64 arrays whose entries are static_cast<double> of the matching columns, and NULL for every group the spec does not name: every robot's
 * state record, auxiliary blob and held inputs, and every host-side fact a setter touches - the IMU quaternion normalised in double after the
 * conversion, the touchdown flag and (rough terrain mode) touchdown detection with its step planes, the switch to the tip-force estimate at the
 * first joint effort (with its one stream synchronisation), the manual-pose flag, the entries of a shorter leg's joints on a mixed-DOF robot.
 * One half of a pair may be named alone.  Columns of legs or joints the morphology lacks and columns [width, row_stride) are ignored.  The
 * pose reset mode stays on its own setter; resident mode takes such an array through shc_engine_resident_post_actions, the K-cycle launches through
 * shc_engine_step_k_actions below.
 * The fleet form is defined the same way against shc_fleet_set_inputs_device: robot r of a part reads row ids[r] - its CALLER's instance id -
 * of `actions` ([n][row_stride]) through the ids device I/O keeps on the device; one kernel per part on the part's own stream, no allocation
 * after the fleet's first device I/O call, the staging footprint unchanged.
 * STREAMS.  Those of the device setters: the engine's stream; while split steps are in flight the pass rides the two half streams, when every
 * group of the spec could (tip force in rough terrain mode, or a joint effort before the switch, join first as their setters do).  on_device = 0
 * copies the host rows into a temporary device buffer and synchronises.  The ordering calls of fleet device I/O apply as written there.
 * REFUSALS (decided before anything changes; a fleet asks every part before the first launch).  SHC_ERR_INVALID_ARG: NULL handle, spec or
 * array; n_fields outside 1 .. SHC_ACT_FIELD_COUNT; an unknown or repeated field; an unknown dtype; reserved != 0; legs / dof below the
 * engine's (legs, longest leg's DOF) or the fleet's shape, or above SHC_MAX_LEGS / SHC_MAX_JOINTS; row_stride non-zero and below the width; an
 * array not aligned to its element size.  SHC_ERR_BUSY: resident mode.  SHC_ERR_UNSUPPORTED: a fleet that spans devices.
 */
enum {
  SHC_ACT_LINEAR_XY,                 /* 2: shc_engine_set_velocity linear_xy               */
  SHC_ACT_ANGULAR,                   /* 1:                         angular                 */
  SHC_ACT_IMU_ORIENTATION,           /* 4: shc_engine_set_imu orientation_wxyz             */
  SHC_ACT_IMU_ANGULAR_VELOCITY,      /* 3:                    angular_velocity             */
  SHC_ACT_POSE_TRANSLATION_VELOCITY, /* 3: shc_engine_set_pose_input translation_velocity  */
  SHC_ACT_POSE_ROTATION_VELOCITY,    /* 3:                           rotation_velocity     */
  SHC_ACT_TIP_FORCE,                 /* per leg, width 3:   shc_engine_set_tip_force       */
  SHC_ACT_JOINT_EFFORT,              /* per leg, width dof: shc_engine_set_joint_effort    */
  SHC_ACT_FIELD_COUNT
};
typedef struct shc_act_spec {        /* 64 bytes */
  int32_t n_fields, fields[SHC_ACT_FIELD_COUNT]; /* column order = this order; a field may appear once               */
  int32_t dtype;                                 /* SHC_OBS_F64 / SHC_OBS_F32                                         */
  int32_t legs, dof;                             /* row geometry, as in shc_obs_spec                                  */
  int32_t reserved;                              /* 0 */
  int64_t row_stride;                            /* elements between rows; 0 = dense; >= the width otherwise          */
} shc_act_spec;
int64_t shc_act_width(const shc_act_spec *spec);                       /* columns of a row; < 0 for an invalid spec; no device needed */
int shc_act_column(const shc_act_spec *spec, int field, int leg, int k); /* column of component k of `field` (leg ignored for robot fields); -1 if absent */
int shc_engine_set_actions(shc_engine *e, const shc_act_spec *spec, const void *actions, int on_device);
int shc_fleet_set_actions_device(shc_fleet *f, const shc_act_spec *spec, const void *actions /* [n][row_stride], caller's order */);
/*
 * Rollout tensors: the two passes above for the K-cycle launches.  shc_engine_step_k_actions runs K cycles in one launch, cycle k with the rows
 * of cycle k of one dense DEVICE array [K][n][A] of float64 or float32 - what a policy emits for a rollout; shc_engine_get_step_k_observations
 * hands q / qd of a range of those cycles back as one dense DEVICE array [cycles][n][D].  The specs, rows and column rules are those of the
 * action and observation passes; there is no host form, as shc_engine_step_k has none.
 * cycle_stride: elements between the rows of consecutive cycles - row i of cycle k lies at array + k * cycle_stride + i * row stride; 0 = n x
 * the row stride, otherwise at least that.  A view big[:, :, 5:5 + A] of a wider 3-D array is row_stride = its columns, cycle_stride = n x that
 * or more.
 * DEFINITION, actions.  After the call the engine is byte for byte what shc_engine_step_k(e, K, in) leaves - every robot's state record and
 * auxiliary blob, every slot of the K-deep output ring, the held inputs and every host-side fact - when each member of `in` is a dense float64
 * device array holding static_cast<double> of the matching columns, and NULL for every group the spec does not name.  Columns of legs or joints
 * the morphology lacks and columns [width, row_stride) are ignored.  One kernel converts the named columns of all K cycles into K-deep float64
 * arrays the engine owns, and shc_engine_step_k itself runs on those: the batch kernel or the serial form, a pending adjusted parameter's first
 * cycle, touchdown detection, the first-effort switch, the split halves and the normalisation of the IMU quaternion are that call's, unchanged.
 * DEFINITION, observations.  SHC_OBS_Q and SHC_OBS_QD only (the ring holds joints).  Column c of row (k, i) holds the double
 * shc_engine_get_step_k_joint_state(e, first_cycle + k, ..) writes for that robot, leg and joint - unchanged for SHC_OBS_F64, static_cast<float>
 * for SHC_OBS_F32; `pad` where the robot has no such leg or joint (the joints a shorter leg of a mixed-DOF robot lacks hold what that getter holds
 * there); columns [width, row_stride) and rows of other cycles are not touched.  The call writes nothing into an engine.
 * LIFETIMES.  `actions` is read by the staging kernel alone, on the engine's stream: it must be ready there, as for shc_engine_set_actions, and
 * may be rewritten as soon as that stream has passed the call - an event recorded on the engine's stream right after the call is enough.  That
 * is LESS than shc_engine_step_k asks of its own arrays (valid until the engine is joined): that rule applies to the staged arrays, which the
 * engine owns.  They are allocated by the first call that needs them, grown (never shrunk) by a call that needs more - that call joins the engine
 * and drains its stream first - and freed with the engine; an engine with split launches in flight is joined (events, no host wait) before a
 * call overwrites them.  The observation call joins split launches, as shc_engine_get_step_k_joint_state, and runs on the engine's stream.
 * FLEET.  Defined the same way against shc_fleet_step_k and shc_fleet_get_step_k_joints_device, in the row geometry of shc_fleet_shape or
 * larger: robot r of a part uses row ids[r] - its CALLER's instance id - of each cycle of the [K][n][row_stride] array.  Per part one staging
 * launch and one read launch, on the part's stream; the staging is the part's K-deep staging of shc_fleet_step_k, counted by
 * shc_fleet_io_bytes: no allocation after the first call of a given K and set of groups.  The STREAMS rules of shc_fleet_step_k apply.
 * REFUSALS (decided before anything changes; a fleet asks every part first).  SHC_ERR_INVALID_ARG: a NULL handle, spec or array; whatever the
 * action / observation pass refuses of a spec; legs / dof below the engine's or the fleet's shape; an array not aligned to its element size;
 * n_cycles outside 1 .. 4096, or a cycle range outside the latest launch (or no launch yet); cycle_stride non-zero and below n x the row stride;
 * an output ring or K-deep staging of 2 GiB or more; SHC_ACT_LINEAR_XY without SHC_ACT_ANGULAR or one IMU field without the other (the K-cycle
 * launches take those in pairs).  SHC_ERR_UNSUPPORTED: the two pose-input fields (set them beforehand: held for the K cycles); an observation
 * field other than q / qd; an engine still starting up; a fleet that spans devices.  SHC_ERR_BUSY: resident mode.
 */
int shc_engine_step_k_actions(shc_engine *e, int n_cycles, const shc_act_spec *spec, const void *actions /* device, [K][n][row_stride] */, int64_t cycle_stride);
int shc_engine_get_step_k_observations(shc_engine *e, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out /* device, [n_cycles][n][row_stride] */,
                                       int64_t cycle_stride);
int shc_fleet_step_k_actions_device(shc_fleet *f, int n_cycles, const shc_act_spec *spec, const void *actions /* [K][n][row_stride], caller's order */,
                                    int64_t cycle_stride);
int shc_fleet_get_step_k_observations_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out /* [n_cycles][n][row_stride], caller's order */,
                                             int64_t cycle_stride);
/*
 * Rollout kinematics: what is a pure function of the joints a K-cycle launch left in its output ring, per cycle - where the feet were, and
 * whether (and in which cycle) a robot ran into its joint limits.  DEVICE arrays only, as the rollout tensors; no cycle kernel takes part, and
 * neither call writes into an engine: state records, auxiliary blobs and the ring are byte for byte what they were.
 * KINEMATICS.  The spec, row and column rules of shc_engine_get_step_k_observations, for any subset of SHC_OBS_Q, SHC_OBS_QD and
 * SHC_OBS_MODEL_TIP.  The q / qd columns are what that call writes.  Column c of SHC_OBS_MODEL_TIP in row (k, i) holds the double
 * shc_engine_get_observations writes for SHC_OBS_MODEL_TIP on an engine whose stored joints are those of ring slot first_cycle + k: Leg::applyFK
 * (model.cpp:975) on the ring's own q, in the robot frame - unchanged for SHC_OBS_F64, static_cast<float> for SHC_OBS_F32, `pad` where the robot
 * has no such leg.
 * HEALTH.  Record (k, i) of health [n_cycles][n] is what shc_debug_robot_health returns for robot i when it is given q and qd of ring slot
 * first_cycle + k (as shc_engine_get_step_k_joint_state returns them), model_tip = poser_tip, zero admittance, zero leg_status and a finite pose:
 * min_limit_proximity, max_speed_ratio, bytes 1 and 2 of leg_masks, SHC_HEALTH_POSITION_LIMIT / _SPEED_LIMIT / _NEAR_LIMIT are live, and
 * SHC_HEALTH_NONFINITE over the q / qd of a leg's own joints; max_tip_deviation and byte 0 of leg_masks are 0.  first_hit[i] is the smallest
 * cycle index c of the latest launch in [first_cycle, first_cycle + n_cycles) whose record has flags & criteria.select != 0, or -1: the `done`
 * mask of a rollout and the index of the first bad step.  Either output may be NULL (not both); health is 16-byte aligned, first_hit 4-byte
 * aligned; criteria is HOST memory, NULL = select 0.  One launch, no atomics: the same bytes on every run.
 * The tips and forces of the walker and the poser, the body pose and the IK deviation of a cycle are not functions of the ring: not delivered.
 * ORDER.  Both calls join split launches (events, no host wait), run on the engine's stream and allocate nothing.
 * FLEET.  Rows, records and first_hit in the CALLER's instance order (shc_fleet_get_step_k_observations_device): one launch per part on the
 * part's stream, no staging.
 * REFUSALS (decided before anything is launched; a fleet asks every part first).  SHC_ERR_INVALID_ARG: a NULL handle, spec or out, or both
 * health outputs NULL; whatever the observation pass refuses of a spec; a misaligned buffer; a cycle range outside the latest K-cycle launch, or
 * no launch yet; cycle_stride non-zero and below n x the row stride; criteria.reserved != 0 or select bits outside the six.
 * SHC_ERR_UNSUPPORTED: an observation field outside the three; criteria.select with SHC_HEALTH_IK_DEVIATION or SHC_HEALTH_TIP_DEVIATION (the
 * ring holds joints: a caller must not believe those are watched); a fleet that spans devices.  SHC_ERR_BUSY: resident mode.
 */
int shc_engine_get_step_k_kinematics(shc_engine *e, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out /* device, [n_cycles][n][row_stride] */,
                                     int64_t cycle_stride);
int shc_engine_scan_step_k_health(shc_engine *e, int first_cycle, int n_cycles, const shc_health_criteria *criteria /* host, may be NULL */,
                                  shc_robot_health *health /* device, [n_cycles][n], may be NULL */, int32_t *first_hit /* device, [n], may be NULL; not both NULL */);
int shc_fleet_get_step_k_kinematics_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_obs_spec *spec, void *out /* [n_cycles][n][row_stride], caller's order */,
                                           int64_t cycle_stride);
int shc_fleet_scan_step_k_health_device(shc_fleet *f, int first_cycle, int n_cycles, const shc_health_criteria *criteria, shc_robot_health *health /* [n_cycles][n], caller's order */,
                                        int32_t *first_hit /* [n], caller's order */);
/*
 * Foothold pass: the externally requested tip targets / default stance poses of rough terrain mode (shc_external_target above) of every robot
 * taken from - or read back into - one dense [n][F] array of float64 or float32, in one kernel per engine (per part of a fleet).  What a
 * foothold planner on the GPU emits never crosses the host; the three host calls above stay as they are.
 * ROW.  The rule of the observation and action passes: the fields of a spec follow each other in the order of `fields`; every field is per
 * leg and takes legs x width columns, leg-major (widths 3, 4, 7, 1, 1, 1 in the order of the enum).  The width of a row and the column of one
 * component come from the two layout calls below; neither needs a device, and both take any selection of fields (what a mode asks of the
 * fields is the set calls' to judge; the get calls read any selection).
 * SET, mode SHC_FH_REQUEST (targetTipPoseCallback).  Every column is read as v = static_cast<double>(column).  For robot i and leg l < its
 * legs let d be its SHC_FH_DEFINED column (d = 1 when the field is not named).  !(d >= 0) - negative or NaN - leaves the leg alone.
 * Otherwise the engine ends byte for byte as shc_engine_set_external_target(e, which, i, 1, l, &row, ..) leaves it with row.defined = (d > 0),
 * row.frame_is_odom_ideal = (column != 0) and the other members taken from the columns; a field the spec does not name has the callback's
 * value: rotation all zero (UNDEFINED_ROTATION), transform the identity 0 0 0 1 0 0 0, clearance 0, frame 0.  SHC_FH_POSITION must be named.
 * "Byte for byte" covers the state record, the auxiliary blob (the records and the sequence state), the lazy allocation of the records and
 * of the sequence state, and the rules of the host call: a LegStepper takes a request only while its robot is not STOPPED, the TARGET of a
 * robot that stands goes to its planner-mode LegPoser, a DEFAULT for it and any stepper request without rough_terrain_mode is dropped.  (One
 * host-side fact is decided per call, not per leg: a REQUEST call marks the engine as carrying external requests even when every leg of its
 * rows is left alone; no record changes by that.)
 * SET, mode SHC_FH_REFRESH_TRANSFORM (generateExternalTargetTransforms).  SHC_FH_TRANSFORM must be named, SHC_FH_DEFINED may be (the same skip
 * rule), nothing else: every selected leg ends as shc_engine_set_external_transform leaves it - only records that are currently defined take
 * the new transform.
 * Columns of legs the robot lacks and columns [width, row_stride) are ignored; the array is never written.
 * IGNORED.  The number of dropped rows, as the host call counts them, is ADDED to *ignored (may be NULL): a host word, valid on return, with
 * on_device = 0; with on_device = 1 and in the fleet form a device int64, 8-byte aligned, that the caller zeroes, ordered on the stream - all
 * parts of a fleet add to the same word.
 * GET.  For every leg a robot has the named columns hold what shc_engine_get_external_target(which) returns for it: SHC_FH_DEFINED and
 * SHC_FH_FRAME_IS_ODOM_IDEAL 0 or 1, the clearance 0 for SHC_EXTERNAL_DEFAULT; unchanged for SHC_OBS_F64, static_cast<float> for SHC_OBS_F32.
 * `pad`, converted once on the host, goes into every column of a leg the robot lacks; columns [width, row_stride) are not touched.  Nothing
 * is written into the engine beyond the lazy allocations the host getter makes too.
 * FLEET.  Robot r of a part reads or writes row ids[r] - its CALLER's instance id - of the [n][row_stride] device array; one kernel per part
 * on the part's stream; part k ends as shc_engine_set_footholds leaves it on the gathered rows.  A part's first foothold call allocates its
 * records (and the sequence state for targets); after that nothing is allocated or staged and shc_fleet_io_bytes does not change.  The
 * readiness checks and the ordering calls of fleet device I/O apply as written there.
 * STREAMS.  The engine calls join split steps first, as the host calls do, and run on the engine's stream.  With on_device = 1 there is no
 * host wait, no allocation and no free but the first call's lazy ones; on_device = 0 stages the columns [0, width) of the host rows with one
 * 2-D copy and synchronises.
 * REFUSALS (decided before anything changes; a fleet asks every part before the first launch).  SHC_ERR_INVALID_ARG: NULL handle, spec or
 * array; n_fields outside 1 .. SHC_FH_FIELD_COUNT; an unknown or repeated field; an unknown dtype, which or mode; reserved != 0; legs below the
 * engine's legs or the fleet's shape, or above SHC_MAX_LEGS; row_stride non-zero and below the width; a mandatory field missing or a forbidden
 * one named for the mode; an array not aligned to its element size or `ignored` not aligned to 8 bytes.  SHC_ERR_UNSUPPORTED:
 * SHC_EXTERNAL_DEFAULT on an engine or part without rough_terrain_mode, as the host calls; a fleet that spans devices.  SHC_ERR_BUSY: resident mode.
 */
enum {
  SHC_FH_POSITION,            /* 3: ExternalTarget::pose_ position                                  */
  SHC_FH_ROTATION,            /* 4: pose_ rotation wxyz; all zero = UNDEFINED_ROTATION              */
  SHC_FH_TRANSFORM,           /* 7: transform_ (x y z qw qx qy qz)                                  */
  SHC_FH_SWING_CLEARANCE,     /* 1                                                                  */
  SHC_FH_FRAME_IS_ODOM_IDEAL, /* 1: != 0 -> frame_id_ == "odom_ideal"                               */
  SHC_FH_DEFINED,             /* 1: > 0 request, 0 withdraw, negative or NaN: leave the leg alone   */
  SHC_FH_FIELD_COUNT
};
enum { SHC_FH_REQUEST = 0, SHC_FH_REFRESH_TRANSFORM = 1 };
typedef struct shc_foothold_spec {   /* 64 bytes */
  int32_t n_fields, fields[SHC_FH_FIELD_COUNT]; /* column order = this order; a field may appear once                */
  int32_t dtype;                                /* SHC_OBS_F64 / SHC_OBS_F32                                          */
  int32_t legs;                                 /* row geometry: >= the engine's legs / the fleet's shc_fleet_shape max_legs */
  int32_t which;                                /* SHC_EXTERNAL_TARGET / _DEFAULT / _PLANNER_TARGET                   */
  int32_t mode;                                 /* SHC_FH_REQUEST / SHC_FH_REFRESH_TRANSFORM (set only; 0 for get)    */
  int32_t reserved;                             /* 0 */
  int64_t row_stride;                           /* elements between rows; 0 = dense; >= the width otherwise           */
  double pad;                                   /* get only: written where a robot has no such leg                    */
} shc_foothold_spec;
int64_t shc_foothold_width(const shc_foothold_spec *spec);                /* columns of a row; < 0 for an invalid spec; no device needed */
int shc_foothold_column(const shc_foothold_spec *spec, int field, int leg, int k); /* column of component k of `field` of `leg`; -1 if absent */
int shc_engine_set_footholds(shc_engine *e, const shc_foothold_spec *spec, const void *rows, int on_device, int64_t *ignored);
int shc_engine_get_footholds(shc_engine *e, const shc_foothold_spec *spec, void *rows, int on_device);
int shc_fleet_set_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, const void *rows /* [n][row_stride], caller's order */, int64_t *ignored_device);
int shc_fleet_get_footholds_device(shc_fleet *f, const shc_foothold_spec *spec, void *rows /* [n][row_stride], caller's order */);
/*
 * Reach probe: which tip targets a leg can reach from its present joints, for C candidate targets per robot, in one kernel per engine (per
 * part of a fleet) that never writes into an engine.  It is the line search of Leg::generateWorkspace (model.cpp:397-470) run with the per-leg
 * calls above: a planner - or a learner bounding a task-space action - gets for every (robot, candidate, leg) the answer that a checkpoint
 * restore and S rounds of shc_leg_set_desired_tip_pose + shc_leg_apply_ik give, without the (2 S + 1) C launches and without the joints, the
 * desired tip and the tip-force estimate of the engine being overwritten.
 * DEFINITION.  For robot i, candidate c and leg l < its legs, each on its own: q0, qd0 are the leg's stored joints, o the tip position that
 * applyIK measures from them (FK of q0 in the robot frame: the frame of shc_leg_set_desired_tip_pose, shc_leg_apply_fk and
 * SHC_OBS_MODEL_TIP) and t = static_cast<double> of the candidate's three columns, in the same frame.  Then for s = 1 .. S:
 *   w = double(s) / S;  desired = o * (1.0 - w) + t * w   (per component; each product and the sum rounded once, no contraction - the
 *   float64 expression of numpy gives the same bits);  setDesiredTipPose(desired, rotation undefined, apply_delta = 0);
 *   r = applyIK(simulation = true);  stop when r == 0.0.
 * applyIK is what shc_leg_apply_ik with simulation = 1 runs for the leg - the DLS step, updateJointPositions with the engine's
 * clamp_joint_positions and no velocity clamp, the 5 mm deviation check - but for the closing tip-force estimate, which feeds nothing back
 * into the joints; nothing is stored.  With steps_done the number of steps that returned non-zero (0 .. S):
 *   SHC_REACH_FRACTION         double(steps_done) / S
 *   SHC_REACH_LIMIT_PROXIMITY  r of the last executed step (0 after a failure)
 *   SHC_REACH_TIP              the FK tip after the last executed step, the failing one included, as the workspace search measures it
 *   SHC_REACH_Q                the joints after that step
 * unchanged for SHC_OBS_F64, static_cast<float> for SHC_OBS_F32.  A candidate with a NaN in any of a leg's three columns is not asked for
 * that leg: the leg's columns hold `pad` (converted once on the host), as do the columns of legs and joints the robot lacks.
 * ROWS.  Robot i's target row holds C blocks of legs x 3 columns, its output row C blocks of D columns, D from the width call below.  Within
 * a block the rule of the observation pass: the fields follow each other in the order of `fields`, every field is per leg and takes
 * legs x width columns, leg-major (widths 1, 1, 3, dof in the order of the enum).  Columns beyond the C blocks of a row are never touched, and
 * the target array is never written.  Both arrays are device arrays of the spec's element type, ready on the engine's stream.
 * NOTHING IS WRITTEN into an engine: state records, auxiliary blobs, held inputs and the output ring of a K-cycle launch are byte for byte
 * what they were.
 * FLEET.  Robot r of a part reads row ids[r] - its CALLER's instance id - of the [n][C][legs][3] targets and writes row ids[r] of the
 * [n][C][D] output; every part is asked first, then one kernel per part on the part's stream with no staging: shc_fleet_io_bytes does not
 * change after the first device I/O call.  The readiness checks and the ordering calls of fleet device I/O apply as written there.
 * STREAMS.  The engine call joins split steps by events, as the observation pass does, and runs on the engine's stream: no host wait, no
 * allocation, no free.  count = 0 is a no-op.
 * REFUSALS (decided before anything is launched).  SHC_ERR_INVALID_ARG: a NULL handle, spec or array; n_fields outside
 * 1 .. SHC_REACH_FIELD_COUNT; an unknown or repeated field; an unknown dtype; reserved != 0; legs / dof below the engine's or the fleet's
 * shape, or above SHC_MAX_LEGS / SHC_MAX_JOINTS; candidates outside 1 .. 64; steps outside 1 .. 4096; row_stride non-zero and below C x D;
 * target_row_stride non-zero and below C x legs x 3; an instance range outside [0, n); an array not aligned to its element size.
 * SHC_ERR_BUSY: resident mode.  SHC_ERR_UNSUPPORTED: a fleet that spans devices.
 */
enum {
  SHC_REACH_FRACTION,        /* 1: steps that returned non-zero / S                              */
  SHC_REACH_LIMIT_PROXIMITY, /* 1: what the last executed applyIK returned                       */
  SHC_REACH_TIP,             /* 3: FK tip after the last executed step, robot frame              */
  SHC_REACH_Q,               /* dof: the joints after that step                                  */
  SHC_REACH_FIELD_COUNT
};
typedef struct shc_reach_spec {      /* 72 bytes */
  int32_t n_fields, fields[SHC_REACH_FIELD_COUNT]; /* column order = this order; a field may appear once                */
  int32_t dtype;                                /* SHC_OBS_F64 / SHC_OBS_F32: element type of BOTH arrays             */
  int32_t legs, dof;                            /* row geometry, as shc_obs_spec                                      */
  int32_t candidates;                           /* C: 1 .. 64                                                         */
  int32_t steps;                                /* S: 1 .. 4096                                                       */
  int32_t reserved;                             /* 0 */
  int64_t row_stride;                           /* out: elements between robots; 0 = C x D                            */
  int64_t target_row_stride;                    /* targets: elements between robots; 0 = C x legs x 3                 */
  double pad;                                   /* written where a leg is not asked or a robot has no such leg / joint */
} shc_reach_spec;
int64_t shc_reach_width(const shc_reach_spec *spec);                      /* D: columns of ONE candidate's block; < 0 for an invalid spec; no device needed */
int shc_reach_column(const shc_reach_spec *spec, int field, int leg, int k); /* column of component k of `field` of `leg` within a block; -1 if absent */
int shc_engine_probe_reach(shc_engine *e, int64_t first, int64_t count, const shc_reach_spec *spec, const void *targets /* device, [count][C][legs][3] */,
                           void *out /* device, [count][C][D] */);
int shc_fleet_probe_reach_device(shc_fleet *f, const shc_reach_spec *spec, const void *targets /* [n][C][legs][3], caller's order */,
                                 void *out /* [n][C][D], caller's order */);
/* The exchange step of a sharded batch: every device ends up with the desired joint positions of ALL instances
 * ([n][max_legs][max_dof], caller's order, NaN padded) in its own HBM, copied device to device (hipMemcpyPeerAsync: xGMI on an
 * MI355X node).  device_buffers[d] (may be NULL) receives device_ids[d]'s buffer; the buffers belong to the fleet. */
int shc_fleet_all_gather_joints(shc_fleet *f, double **device_buffers);

/* Step plan pass (shc_plan_spec, shc_engine_get_step_plan, shc_fleet_get_step_plan_device): declared in a header of its own, part of this ABI. */
#include "shc_step_plan.h"

#ifdef __cplusplus
}
#endif
#endif /* SHC_BATCH_H */
