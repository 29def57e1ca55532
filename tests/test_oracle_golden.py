"""CPU: the oracle against the committed golden vectors (tests/golden/math_golden.json, made by make_golden.py with
scipy / numpy — implementations independent of the oracle) and the hand-derived step-cycle known answers."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle_lib import OracleRobot, _ptr, lib
from syropod_highlevel_controller_amd import default_hexapod_params
from syropod_highlevel_controller_amd.params import StepCycle

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "math_golden.json")))


def _arr(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def same_rotation(qa, qb, tol=1e-12):
    qa, qb = np.asarray(qa), np.asarray(qb)
    return min(np.abs(qa - qb).max(), np.abs(qa + qb).max()) < tol


def test_euler_to_quat_matches_scipy():
    L = lib()
    for c in GOLD["euler"]:
        out = np.zeros(4)
        L.orc_test_euler_to_quat(_ptr(_arr(c["euler"])), 0, _ptr(out))
        assert same_rotation(out, c["quat_extrinsic"])
        L.orc_test_euler_to_quat(_ptr(_arr(c["euler"])), 1, _ptr(out))
        assert same_rotation(out, c["quat_intrinsic"])


def test_quat_to_euler_round_trip():
    # the reference's quaternionToEulerAngles (with its flip fix-up) must invert eulerAnglesToQuaternion for |pitch| < pi/2
    L = lib()
    for c in GOLD["euler"]:
        for intrinsic, key in ((0, "quat_extrinsic"), (1, "quat_intrinsic")):
            e = np.zeros(3)
            L.orc_test_quat_to_euler(_ptr(_arr(c[key])), intrinsic, _ptr(e))
            q = np.zeros(4)
            L.orc_test_euler_to_quat(_ptr(e), intrinsic, _ptr(q))
            assert same_rotation(q, c[key], 1e-11)
            # same angles modulo 2 pi: the reference's flip fix-up (standard_includes.h:270-289) can return roll/yaw in
            # (pi, 3 pi / 2) — a quirk the oracle keeps
            # it also re-labels any rotation whose 2nd/3rd Eigen angle exceeds pi/2 with the alternate Euler triple, so
            # the triple itself is only comparable when every input angle is below pi/2
            if np.all(np.abs(c["euler"]) < np.pi / 2 - 1e-6):
                np.testing.assert_allclose(e, c["euler"], atol=1e-10)


def test_from_two_vectors():
    L = lib()
    for c in GOLD["from_two_vectors"]:
        out = np.zeros(4)
        L.orc_test_from_two_vectors(_ptr(_arr(c["a"])), _ptr(_arr(c["b"])), _ptr(out))
        np.testing.assert_allclose(out, c["quat"], atol=1e-13)


def test_slerp_and_matrix_to_quat():
    from scipy.spatial.transform import Rotation as R
    L = lib()
    for c in GOLD["slerp"]:
        out = np.zeros(4)
        L.orc_test_slerp(_ptr(_arr(c["a"])), c["t"], _ptr(_arr(c["b"])), _ptr(out))
        assert abs(np.linalg.norm(out) - 1.0) < 1e-12
        m = R.from_quat([out[1], out[2], out[3], out[0]]).as_matrix()
        np.testing.assert_allclose(m, c["rotmat"], atol=1e-12)
    for c in GOLD["quat_from_matrix"]:
        out = np.zeros(4)
        L.orc_test_quat_from_matrix(_ptr(_arr(c["m"])), _ptr(out))
        assert same_rotation(out, c["quat"])


def test_lu_inverse():
    L = lib()
    for c in GOLD["inverse"]:
        n = c["n"]
        inv = np.zeros(n * n)
        assert L.orc_test_lu_inverse(_ptr(_arr(c["a"])), n, _ptr(inv)) == 1
        np.testing.assert_allclose(inv, c["inv"], rtol=1e-9, atol=1e-9)


def test_hexapod_fk_matches_numpy_chain():
    L = lib()
    p = default_hexapod_params("tripod")
    for c in GOLD["hexapod_fk"]:
        tip, quat = np.zeros(3), np.zeros(4)
        L.orc_test_leg_fk(C.byref(p), c["leg"], _ptr(_arr(c["q"])), _ptr(tip), _ptr(quat))
        np.testing.assert_allclose(tip, c["tip"], atol=1e-15)
        assert same_rotation(quat, c["quat"])


def test_hexapod_ik_step_matches_numpy():
    L = lib()
    p = default_hexapod_params("tripod")
    for c in GOLD["hexapod_ik_step"]:
        qo, qdo, tip = np.zeros(3), np.zeros(3), np.zeros(3)
        L.orc_test_leg_ik_step(C.byref(p), c["leg"], _ptr(_arr(c["q"])), _ptr(_arr(c["qd"])), _ptr(_arr(c["desired"])), 1,
                               _ptr(qo), _ptr(qdo), _ptr(tip))
        np.testing.assert_allclose(qo, c["q_out"], atol=1e-13)
        np.testing.assert_allclose(qdo, c["qd_out"], atol=1e-11)


def test_admittance_rk4():
    L = lib()
    p = default_hexapod_params("wave")
    for c in GOLD["admittance"]:
        st = _arr(c["x0"]).copy()
        d = np.zeros(3)
        L.orc_test_admittance(C.byref(p), _ptr(st), _ptr(_arr(c["force"])), _ptr(d))
        np.testing.assert_allclose(st, c["state"], atol=1e-15)          # literal RK4 in numpy
        np.testing.assert_allclose(d, c["delta"], atol=1e-15)
        np.testing.assert_allclose(st, c["state_exact"], atol=5e-8)      # exact solution: RK4 truncation only
        np.testing.assert_allclose(d, c["delta_exact"], atol=5e-8)


def test_bezier():
    L = lib()
    for c in GOLD["bezier"]:
        b, db = np.zeros(3), np.zeros(3)
        L.orc_test_quartic_bezier(_ptr(_arr(c["nodes"])), c["t"], _ptr(b), _ptr(db))
        np.testing.assert_allclose(b, c["b"], atol=1e-14)
        np.testing.assert_allclose(db, c["db"], atol=1e-13)


@pytest.mark.parametrize("gait", ["tripod", "wave", "ripple", "amble"])
def test_step_cycle_known_answers(gait):
    """Hand-derived from walk_controller.cpp:365-410 and :277 at default.yaml / gait.yaml."""
    L = lib()
    p = default_hexapod_params(gait)
    sc = StepCycle()
    L.orc_test_generate_step_cycle(C.byref(p), C.byref(sc))
    k = GOLD["step_cycle"][gait]
    for f in ("period", "stance_end", "swing_start", "swing_end", "stance_start", "stance_period", "swing_period"):
        assert getattr(sc, f) == k[f], f
    assert sc.frequency == pytest.approx(k["frequency"], rel=1e-15)
    assert sc.stance_period % 2 == 0 and sc.swing_period % 2 == 0      # ROS_ASSERTs at walk_controller.cpp:392-393
    r = OracleRobot(p)
    assert list(r.tables().phase_offset)[:6] == k["phase_offset"]


# ------------------------------------------------------------------------------------------------ multi-cycle trajectories
def _walk_scenarios():
    import json
    import os
    meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "walk_golden_meta.json")))
    return sorted(meta.items())


@pytest.mark.parametrize("name,meta", _walk_scenarios(), ids=[n for n, _ in _walk_scenarios()])
def test_walk_trajectories(name, meta):
    """Hundreds of cycles of walking from an INDEPENDENT numpy restatement of WalkController::updateWalk / getLimit / LegStepper
    / updateWalkPlane and PoseController's walk-plane, auto and IMU poses (tests/golden/make_walk_golden.py, written from the
    reference sources alone): velocity limiting, every walk-state transition, first-step handling of legs that start mid swing,
    swing / stance Bezier tips, default-tip updates on stopping, auto-poser latches, the IMU PID, and rough terrain mode's
    model-free branches (default-tip update every step, requested targets with clearance / tf transform / odometry lead,
    requested default poses, the reactive step-depth target, the walk plane fitted through the moving defaults).  Scenarios
    with "model" also carry the JOINTS of an independent numpy chain for the whole cycle (updateStance, setDesiredTipPose, the
    6x6 DLS solveIK with its cost gradient, updateJointPositions), free-running from the recorded start-up state: 1e-6 rad bar.  The oracle must reproduce the
    walker tips to 1e-9 m, the body pose to 1e-9 and every integer exactly."""
    import os
    from oracle_lib import OracleRobot
    from syropod_highlevel_controller_amd import default_hexapod_params
    from syropod_highlevel_controller_amd.params import VEL_REAL
    data = np.load(os.path.join(os.path.dirname(__file__), "golden", "walk_golden.npz"))
    g = {k.split("/", 1)[1]: data[k] for k in data.files if k.startswith(name + "/")}
    p = default_hexapod_params(meta["gait"])
    if meta["overrides"].get("morphology") == "8x5":   # BASELINE.json config 4's synthetic octopod
        from syropod_highlevel_controller_amd import synthetic_octopod_params
        p = synthetic_octopod_params(meta["gait"], 5, 8)
    if meta["overrides"].get("morphology") == "mixed":   # legs of 3 / 5 / 4 / 3 / 5 / 4 joints in one robot
        from syropod_highlevel_controller_amd import synthetic_mixed_dof_params
        p = synthetic_mixed_dof_params(meta["gait"])
    dofs = [p.leg_dof[l] for l in range(p.leg_count)]
    LD = (p.leg_count, max(dofs))

    def padded(flat):   # the oracle packs each leg's own joints; the fixture is [legs][longest leg], zero tails
        out, at = np.zeros(LD), 0
        for l, d in enumerate(dofs):
            out[l, :d] = flat[at:at + d]
            at += d
        return out
    for k, v in meta["overrides"].items():
        if k == "velocity_input_mode":
            p.velocity_input_mode = VEL_REAL if v == "real" else 0
        elif k in ("n_auto_posers", "model", "morphology", "contacts", "efforts", "pose_inputs", "gait_change", "adjust"):
            pass  # (default_hexapod_params already carries auto_pose.yaml; "model": the scenario also carries joints)
        else:
            setattr(p, k, v)
    if p.imu_posing:
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    p.time_to_start = meta["time_to_start"]   # 100 start-up steps: the start-up iteration is well-posed there (make_init_golden.py)
    r = OracleRobot(p)
    t = r.tables()
    for k, table in meta["limits"].items():  # the fixture's limit tables (the numpy init chain's) are the ones this oracle derives too
        np.testing.assert_allclose(list(getattr(t, k)), table, rtol=1e-9)
    worst_tip = worst_pose = worst_q = 0.0
    start_diff = None
    if "joint_start" in g:   # the oracle's own direct start-up + first loop against the independent init chain's: no state is handed over
        start_diff = float(np.abs(np.stack([padded(x) for x in r.joints()]) - g["joint_start"]).max())
        assert start_diff < (1e-9 if LD[1] > 3 else 1e-12), (name, start_diff)
    from syropod_highlevel_controller_amd.params import ExternalTarget
    L = lib()
    for c in range(meta["cycles"]):
        for ec, kind, leg, v in meta.get("events", []):   # rough-terrain scenarios: TargetTipPose / tf refresh / tip-state messages
            if ec != c:
                continue
            which = 0 if kind.endswith("target") else 1
            if kind in ("target", "default", "withdraw_default"):
                row = ExternalTarget()
                if kind != "withdraw_default":
                    row.defined, row.swing_clearance, row.frame_is_odom_ideal = 1, v[7], int(v[8])
                    row.pose[:] = v[:7]
                    row.transform[:] = [0, 0, 0, 1, 0, 0, 0]
                L.orc_set_external_target(r.h, which, leg, C.byref(row))
            elif kind.startswith("transform_"):
                L.orc_set_external_transform(r.h, which, leg, _ptr(_arr(v)))
            elif kind == "zero_tip_force":
                L.orc_set_tip_force(r.h, _ptr(np.zeros(3 * p.leg_count)))
            elif kind == "pose_input":
                r.set_pose_input(v[:3], v[3:])
            elif kind == "pose_reset_mode":
                L.orc_set_pose_reset_mode(r.h, int(v[0]))
        if "gait_request" in g and g["gait_request"][c]:   # gait_change_flag_ set: changeGait runs every loop until the robot has stopped
            L.orc_change_gait(r.h, C.byref(default_hexapod_params(meta["overrides"]["gait_change"])))
        r.set_velocity(float(g["lin"][c][0]), float(g["lin"][c][1]), float(g["ang"][c]))
        if "adjust_request" in g:   # parameterAdjustCallback sets parameter_adjust_flag_; runningState serves it inside the loops (state_running_state) until it is set
            fresh = g["adjust_request"][c] and (c == 0 or g["adjust_request"][c - 1] != g["adjust_request"][c] or g["adjust_value"][c - 1] != g["adjust_value"][c])
            if fresh:
                L.orc_request_parameter_adjust(r.h, int(g["adjust_request"][c]), float(g["adjust_value"][c]))
            assert bool(L.orc_parameter_adjust_pending(r.h)) == bool(g["adjust_request"][c]), (name, c)   # ... for exactly as many loops as the fixture's robot waited
        if p.imu_posing or p.inclination_posing:
            r.set_imu(g["imu_q"][c], g["gyro"][c])
        if p.admittance_control and not p.use_joint_effort:
            r.set_tip_force(g["force"][c])
        if "effort" in g:              # measured joint torques -> Leg::calculateTipForce
            r.set_joint_effort(g["effort"][c])
        if "contact_force" in g:       # tip-state messages of the synthetic terrain: touchdown detection runs on arrival
            r.set_tip_force(g["contact_force"][c])
        r.cycle(1)
        ls = r.leg_state()
        pose, vel, ws = r.body_state()
        assert ws == g["walk_state"][c], (name, c)
        assert np.array_equal(ls["leg_status"] & 3, g["state"][c]), (name, c)
        assert np.array_equal(ls["leg_status"] >> 8, g["phase"][c]), (name, c)
        np.testing.assert_allclose(vel, g["velocity"][c], atol=1e-12, err_msg=f"{name} cycle {c}")
        worst_tip = max(worst_tip, np.abs(ls["walker_tip"] - g["tips"][c]).max())
        q = np.array(pose)
        if q[3] < 0:
            q[3:] = -q[3:]
        worst_pose = max(worst_pose, np.abs(q - g["pose"][c]).max())
        assert worst_tip < 1e-9 and worst_pose < 1e-9, (name, c, worst_tip, worst_pose)
        odo = np.zeros(7)                     # WalkController::odometry_ideal_: the desired body velocity integrated (:643, :783-791)
        L.orc_get_odometry(r.h, _ptr(odo))
        if odo[3] < 0:
            odo[3:] = -odo[3:]
        assert np.abs(odo - g["odometry"][c]).max() < 1e-12, (name, c, odo, g["odometry"][c])
        if "q" in g:   # joints of the whole cycle (updateStance + setDesiredTipPose + applyIK) from the independent numpy chain, free-running
            worst_q = max(worst_q, np.abs(padded(r.joints()[0]) - g["q"][c]).max())
            for f in ("poser_tip", "model_tip"):   # what publishLegState sends of the LegPoser's and the leg's tip poses
                assert np.abs(ls[f] - g[f][c]).max() < 1e-9, (name, c, f)
            assert worst_q < 1e-6, (name, c, worst_q)
            if meta["overrides"].get("dynamic_stiffness"):   # Leg::virtual_stiffness_ as publishLegState reports it (state_controller.cpp:889)
                from syropod_highlevel_controller_amd.params import LegStateMsg
                msg = (LegStateMsg * p.leg_count)()
                L.orc_get_leg_state_msg(r.h, msg)
                assert np.abs(np.array([m.virtual_stiffness for m in msg]) - g["stiffness"][c]).max() < 1e-12, (name, c)
            if "effort" in g:          # the tip-force estimate itself (LegState.tip_force carries it times the force gain, :883-885)
                assert np.abs(ls["tip_force"] - g["tip_force_calc"][c]).max() < 1e-9, (name, c)
    print(f"{name}: {meta['cycles']} cycles, walk states {meta['visited_walk_states']}, max |tip diff| {worst_tip:.2e} m, max |pose diff| {worst_pose:.2e}"
          + (f", max |joint diff| {worst_q:.2e} rad (free-running independent IK chain, each side from its own start-up: {start_diff:.1e} rad apart)" if "q" in g else ""))


# ------------------------------------------------------------------------------------------------ LegPoser primitives
def _golden_hexapod_params(gait="tripod"):
    """default.yaml with the start-up length the generators use (tests/golden/make_walk_golden.py START_UP_TIME: 100 start-up steps,
    where two correct implementations of that iteration agree to 1e-15 rad) - the oracle and the numpy chain each run their own."""
    p = default_hexapod_params(gait)
    p.time_to_start = 2.0
    return p


SEQ = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_golden.npz"))


@pytest.mark.parametrize("name", sorted({k.split("/")[1] for k in SEQ.files if k.startswith("step/")}))
def test_sequence_trajectories(name):
    """LegPoser::stepToPosition (pose_controller.cpp:1571-1712) call by call against the independent numpy restatement of
    tests/golden/make_sequence_golden.py: progress values exact, tip positions and directions to 1e-12."""
    from golden_replay import oracle_backend, replay_step_to_position
    replay_step_to_position(oracle_backend, name)


@pytest.mark.parametrize("name", sorted({k.split("/")[1] for k in SEQ.files if k.startswith("cfg/")}))
def test_configuration_transition_trajectories(name):
    """LegPoser::transitionConfiguration (pose_controller.cpp:1476-1567) against the independent restatement."""
    from golden_replay import oracle_backend, replay_configuration_transition
    replay_configuration_transition(oracle_backend, name)


def test_pack_and_unpack_trajectories():
    """PoseController::packLegs / unpackLegs (pose_controller.cpp:615-706) against the independent restatement (Packer in
    tests/golden/make_sequence_golden.py): two pack steps in, back out to the unpacked positions."""
    from golden_replay import oracle_backend, replay_pack_unpack
    print(replay_pack_unpack(oracle_backend))


@pytest.mark.parametrize("start", ["ready", "offset", "8x5"])
def test_startup_sequence_trajectories(start):
    """PoseController::executeSequence (pose_controller.cpp:145-459) against the independent numpy restatement of
    tests/golden/make_startup_golden.py: a first START_UP (learning its transition poses inside the joint-limit safety factor; from
    the READY estimate, and from a configuration up to 0.25 rad away from it), SHUT_DOWN, START_UP again (replay) - every return
    value exactly, joints to 1e-6 rad call by call."""
    from golden_replay import oracle_backend, replay_startup_sequence
    print(replay_startup_sequence(oracle_backend, start))


@pytest.mark.parametrize("mode", ["tip_control", "joint_control", "imu_and_inclination_posing", "8x5_gravity_aligned_tips", "auto_posing"])
def test_manual_leg_trajectories(mode):
    """Manual leg manipulation (legStateToggle, poseForLegManipulation, updateManual x 2, the manual-leg cases of updateStance /
    setDesiredTipPose / stepToPosition) against the independent numpy restatement of tests/golden/make_manual_golden.py, loop by
    loop: request results exactly; joints to 1e-6 rad while the robot walks, 5e-3 once it stands (free-running: the reference's
    IK step amplifies rounding differences on a standing robot).  joint_control: the velocity inputs step the
    coxa / tibia joints and every applyIK of the MANUAL leg is rotation-constrained from the tip pose of before the step.  (The same
    replay runs on the HIP engine in tests/test_gpu_golden.py.)"""
    from golden_replay import oracle_backend, replay_manual
    print(replay_manual(oracle_backend, mode))


@pytest.mark.parametrize("posing", ["walk_plane_posing", "imu_and_inclination_posing", "8x5_gravity_aligned_tips", "auto_posing"])
def test_planner_trajectories(posing):
    """Planner mode (executePlan, PoseController::transitionConfiguration / transitionStance, the LegPoser's external target)
    against the independent numpy restatement of tests/golden/make_planner_golden.py, loop by loop: executePlan's result and
    plan_step_ exactly; joints free-running (tolerances in golden_replay.py).  The second run executes the plan under IMU + inclination
    posing: the body pose moves under the robot while it stands, waits (updateModel on the LegPoser tips of the last updateStance) and
    transitions.  (The same replay runs on the HIP engine in tests/test_gpu_golden.py.)"""
    from golden_replay import oracle_backend, replay_planner
    print(replay_planner(oracle_backend, posing))


def test_step_to_new_stance_trajectory():
    """PoseController::stepToNewStance (pose_controller.cpp:521-557) against the independent restatement in
    tests/golden/make_startup_golden.py: both leg groups step onto their default tip poses; return values exactly, joints free-running."""
    from golden_replay import oracle_backend, replay_step_to_new_stance
    print(replay_step_to_new_stance(oracle_backend))


# ------------------------------------------------------------------------------------------------ the init chain
INIT_META = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_golden_meta.json")))


@pytest.mark.parametrize("who", ["oracle", "product_host_chain"])
@pytest.mark.parametrize("name", sorted(INIT_META))
def test_init_chain_golden(name, who):
    """The init chain - direct start-up solve, Leg::generateWorkspace (single plane and layered), generateWalkspace, generateLimits,
    phase offsets - against the independent numpy restatement of tests/golden/make_init_golden.py (written from the reference alone:
    src/pose_controller.cpp:463-517, src/model.cpp:120-138, 286-551, src/walk_controller.cpp:57-411), at start-up step counts where
    the iteration is well-posed (200 for 3-joint legs, 100 for the redundant 5-joint chains; tests/test_oracle_conditioning.py).
    Both the oracle and the product's host chain (shc_generate_tables: host code, no GPU needed) are held to it."""
    from oracle_lib import OracleRobot
    from syropod_highlevel_controller_amd import default_hexapod_params, engine, synthetic_octopod_params
    m = INIT_META[name]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_golden.npz"))
    if m["morphology"] == "mixed":      # legs of 3 / 5 / 4 / 3 / 5 / 4 joints: the numpy chain and the oracle run every leg with its own joint
        from syropod_highlevel_controller_amd import synthetic_mixed_dof_params   # count, the product pads the shorter legs behind their tips
        p = synthetic_mixed_dof_params(m["gait"])
    else:
        p = synthetic_octopod_params(m["gait"], 5, 8) if m["morphology"] == "8x5" else default_hexapod_params(m["gait"])
    p.time_to_start, p.rough_terrain_mode, p.gravity_aligned_tips = m["time_to_start"], m["rough_terrain_mode"], m["gravity_aligned_tips"]
    L, NJ = p.leg_count, max(p.leg_dof[l] for l in range(p.leg_count))
    t = OracleRobot(p).tables() if who == "oracle" else engine.generate_tables(p)
    assert list(t.phase_offset)[:L] == m["phase_offset"]
    for k in ("period", "swing_start", "swing_end", "stance_period", "swing_period"):
        assert getattr(t.step, k) == m["step"][k]
    assert t.step.frequency == m["step"]["frequency"]
    q = np.array([[t.default_joint_position[l][j] for j in range(NJ)] for l in range(L)])
    gq = g[name + ".q0"]
    dq = float(np.nanmax(np.abs(q - gq)))                    # (NaN in the fixture: a leg with fewer joints than the longest)
    assert (q[np.isnan(gq)] == 0.0).all()                    # ... whose padded entries the tables leave at 0
    wp = np.array([[t.workspace_radius[l][b] for b in range(9)] for l in range(L)])
    dwp = float(np.abs(wp - g[name + ".workplane"]).max())
    print(f"init chain {name} ({who}): start-up configuration after {m['startup_calls']} steps |dq| = {dq:.2e} rad, workplane {dwp:.2e} m")
    assert dq <= (1e-8 if NJ > 3 and not m["gravity_aligned_tips"] else 1e-11)   # (position-only IK on 5 joints drifts along its null space)
    assert dwp <= 1e-9
    for k in ("walkspace", "max_linear_speed", "max_angular_speed", "max_linear_acceleration", "max_angular_acceleration"):
        np.testing.assert_allclose(list(getattr(t, k)), g[name + "." + k], rtol=1e-9, atol=1e-12)
