"""GPU: the loop-level calls - every StateController::loop() that is not the plain control cycle (toggle_leg_state, execute_plan, execute_sequence,
step_to_new_stance, finish_sequence_startup, pack_legs / unpack_legs) - after their host side moved onto one driver (csrc/shc_loop_calls.hpp: loop_call,
RtFlagsGuard) and their device side onto RobIO / pose_step_dev / posing_part_dev (csrc/shc_leg_api.hpp, csrc/shc_sequence.hpp), DESIGN.md section 4.3.

Free-running, no oracle in the loop: every array a loop-level call returns, and at a handful of points the bytes of get_state(), get_aux_state(), joints()
and leg_manipulation_state(), are compared byte for byte with tests/golden/loop_calls_golden.npz - what the commit before the move returned for the same
calls on an MI355X (`python tests/test_gpu_loop_calls.py OUT.npz` records it, with that commit's package on PYTHONPATH).

The loop-level kernels run one thread per robot in blocks of 64, and the marked cycle that follows mixes marked and unmarked robots inside a wavefront's
robot groups: n = 65 (two blocks, the second holds one robot), else one robot more than a wavefront of the cycle kernel holds (11 hexapods, 9 octopods).
The schedules are those tests/test_gpu_manual_legs.py and tests/test_gpu_planner.py hold to the oracle call by call (parameters from the package's own
builders), here run in one piece: walk (two robots without a velocity command) / toggle a leg per robot (two robots without a request) / manipulate / a
second leg, a third is refused / toggle back / planner mode on / a configuration step, a tip-target + body-pose step, a body-pose-only step / planner
mode off / walk.  The sequence cases: three robots started from their own joint positions run START_UP (which generates the sequence), SHUT_DOWN,
START_UP, finish_sequence_startup, step_to_new_stance, then pack and unpack; once more on the hexapod with auto posing on its own clock, where every
sequence call runs a pose-only pass of the cycle kernel (those robots start from one configuration: finish_sequence_startup wants them in one pose phase).

A recording that does not show every branch of the driver is refused (`check_coverage`), and the test asserts the same of its own run."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "loop_calls_golden.npz")
pytestmark = pytest.mark.gpu

CASES = ("hexapod_65_manual_posing", "hexapod_imu_posing", "hexapod_auto_inclination_admittance", "octopod_8x5_gravity", "mixed_dof_354354")
SEQUENCE_CASES = ("hexapod_sequences", "octopod_8x5_sequences", "hexapod_sequences_own_clock")
SEED = {name: 700 + i for i, name in enumerate(CASES + SEQUENCE_CASES)}
WAITING, WALKING = -2, -1


def case_params(name):
    """(parameters, robots)"""
    from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_mixed_dof_params, synthetic_octopod_params
    if name.startswith("octopod_8x5"):
        p = synthetic_octopod_params("ripple", 5, 8)
        if name == "octopod_8x5_gravity":   # the rotation-constrained IK (F_ROT) under the loop-level kernels
            p.gravity_aligned_tips = 1
    elif name.startswith("mixed"):
        p = synthetic_mixed_dof_params("ripple", (3, 5, 4, 3, 5, 4))
    else:
        p = default_hexapod_params("tripod")
    if name == "hexapod_65_manual_posing":    # LOOP_WHOLE; the toggle's updateStiffness runs as well
        p.admittance_control, p.dynamic_stiffness = 1, 1
        return p, 65
    if name == "hexapod_imu_posing":          # LOOP_MARK / LOOP_AFTER_POSE
        p.imu_posing = 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    if name == "hexapod_auto_inclination_admittance":
        p.auto_posing, p.inclination_posing, p.manual_posing, p.admittance_control = 1, 1, 1, 1
    if name == "hexapod_sequences_own_clock":
        p.auto_posing, p.pose_frequency = 1, 0.8
    if name in SEQUENCE_CASES:
        return p, 3
    return p, (9 if p.leg_count == 8 else 11)


def posed_protocol(p):
    """The body pose moves while a robot stands: the mark / pose pass / body form of the protocol (else the kernel runs the whole loop)."""
    return bool(p.imu_posing or p.auto_posing or p.inclination_posing)


def snapshot(out, key, e):
    """The bytes of everything the engine keeps, under `key` (an oracle run, which only confirms the schedule, has no auxiliary blob: nothing recorded)."""
    if not hasattr(e, "get_aux_state"):
        return
    out[f"{key}.state"] = np.frombuffer(bytes(e.get_state()), dtype=np.uint8)
    out[f"{key}.aux"] = np.frombuffer(bytes(e.get_aux_state()), dtype=np.uint8)
    q, qd = e.joints()
    out[f"{key}.q"], out[f"{key}.qd"] = np.array(q), np.array(qd)
    out[f"{key}.manipulation"] = np.array(e.leg_manipulation_state())


def rows(log):
    return np.array(log, dtype=np.int32)


def record_case(name, make):
    """The toggle / manipulate / plan schedule on one engine."""
    from syropod_highlevel_controller_amd.params import ExternalTarget
    p, n = case_params(name)
    L, D = p.leg_count, max(p.leg_dof[l] for l in range(p.leg_count))
    rng = np.random.default_rng(SEED[name])
    out = {f"{name}.posed": np.array([posed_protocol(p)])}
    e = make(p, n)
    widths = [D] * L if e.joints()[0].shape[1] == L * D else [p.leg_dof[l] for l in range(L)]   # (an oracle packs each leg's own joint count)
    at = np.concatenate([[0], np.cumsum(widths)])
    calls = [0]

    def imu():   # a new IMU reading every 20 loops: the robots stand on a slope that changes under them
        calls[0] += 1
        if (p.imu_posing or p.inclination_posing) and calls[0] % 20 == 1:
            axis, half = rng.normal(0, 1, (n, 3)) * [1, 1, 0.2], 0.5 * rng.uniform(0.02, 0.12, (n, 1))
            axis /= np.linalg.norm(axis, axis=1, keepdims=True)
            e.set_imu(np.concatenate([np.cos(half), np.sin(half) * axis], axis=1), rng.normal(0, 0.03, (n, 3)))

    def cycles(k):
        for _ in range(k):
            imu()
            e.step(1)

    def toggle(selection, log, limit=1500):
        sel = np.array(selection, dtype=np.int32)
        pending = sel >= 0
        for _ in range(limit):
            if not pending.any():
                return
            imu()
            res = np.array(e.toggle_leg_state(np.where(pending, sel, -1).astype(np.int32)))
            log.append(res)
            still = res == -1      # still walking: the node zeroes that robot's velocity inputs and its loop runs the normal cycle
            if still.any():
                lin[still], ang[still] = 0.0, 0.0
                e.set_velocity(lin, ang)
            pending &= ~((res == 1) | (res == 2))
        raise AssertionError((name, "toggle did not finish", res.tolist()))

    def plan_until(log, steps, value, limit=700):
        done = np.zeros(n, dtype=bool)
        for _ in range(limit):
            imu()
            pr, st = e.execute_plan()
            log.append(np.array(pr))
            steps.append(np.array(st))
            done |= np.array(pr) == value
            if done.all():
                return
        raise AssertionError((name, "plan step did not finish", np.array(pr).tolist()))

    try:
        # ---- walk; robots 0 and 5 have no velocity command and stand
        lin, ang = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
        lin[[0, 5]], ang[[0, 5]] = 0.0, 0.0
        e.set_velocity(lin, ang)
        if p.admittance_control:
            e.set_tip_force(np.full((n, L, 3), 1.5))
        cycles(60)
        # ---- a leg per robot (robot i: leg i % L); robots 3 and n - 1 have no request and keep walking
        none = (3, n - 1)
        first = [-1 if i in none else i % L for i in range(n)]
        log = []
        toggle(first, log)
        out[f"{name}.toggle.first"] = rows(log)
        # ---- manipulate: tip velocity inputs, then a tip position; body velocity commands are ignored by the frozen robots
        prim = np.array(first, dtype=np.int32)
        lin[:], ang[:] = rng.uniform(-0.5, 0.5, (n, 2)), 0.3
        e.set_velocity(lin, ang)
        e.set_manual_inputs(prim, rng.uniform(-1, 1, (n, 3)), None, None, None, None)
        cycles(25)
        pos = np.array([[p.stance_position[max(first[i], 0)][0] * 0.9, p.stance_position[max(first[i], 0)][1] * 0.9, -0.06] for i in range(n)])
        e.set_manual_inputs(prim, np.zeros((n, 3)), pos, None, None, None)
        cycles(25)
        snapshot(out, f"{name}.manipulated", e)
        # ---- a second leg on robots 0-2, then a third on robot 0 is refused
        second = [(first[i] + 2) % L if i < 3 else -1 for i in range(n)]
        log = []
        toggle(second, log)
        e.set_manual_inputs(prim, rng.uniform(-1, 1, (n, 3)), None, np.array(second, dtype=np.int32), rng.uniform(-1, 1, (n, 3)), None)
        cycles(20)
        toggle([(first[0] + 4) % L] + [-1] * (n - 1), log)
        out[f"{name}.toggle.second_and_third"] = rows(log)
        # ---- back to walking
        e.set_manual_inputs(None, None, None, None, None, None)
        log = []
        toggle(second, log)
        toggle(first, log)
        out[f"{name}.toggle.back"] = rows(log)
        assert (np.array(e.leg_manipulation_state()) == 0).all(), name
        lin[:], ang[:] = rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-0.5, 0.5, n)
        lin[[0, 5]], ang[[0, 5]] = 0.0, 0.0
        e.set_velocity(lin, ang)
        cycles(40)
        snapshot(out, f"{name}.walking_again", e)
        # ---- planner mode: walking robots are stopped by the call (their loop is the marked cycle), standing ones wait for plan step 0
        e.set_planner_mode(True)
        log, steps = [], []
        plan_until(log, steps, WAITING)
        for _ in range(600):
            if (log[-1] == WAITING).all():
                break
            plan_until(log, steps, WAITING, limit=1)
        assert (log[-1] == WAITING).all(), (name, log[-1].tolist())
        # ---- plan step 0: a joint configuration; robot i leaves leg i % L out of the message, robot 7 names no leg at all
        q0 = np.array(e.joints()[0])
        cfg = q0 + rng.uniform(-0.12, 0.12, (n, L, D)).reshape(n, L * D)[:, :q0.shape[1]]
        for i in range(n):
            cfg[i, at[i % L]:at[i % L + 1]] = np.nan
        cfg[7] = np.nan
        e.set_target_configuration(cfg)
        plan_until(log, steps, 100)
        for _ in range(3):
            plan_until(log, steps, WAITING, limit=1)
        # ---- plan step 1: tip targets for half the legs (with a swing clearance, some with a tip rotation) + a body pose for the even robots
        tips = np.array(e.leg_state()["model_tip"]).reshape(n, L, 3)
        targets = (ExternalTarget * (n * L))()
        quat = rng.normal(size=(n, L, 4)) * [0.25, 1.0, 0.25, 0.25] + [0, 0, 0.7, 0]
        quat /= np.linalg.norm(quat, axis=2, keepdims=True)
        offs = rng.normal(size=(n, L, 3))
        offs *= rng.uniform(0.035, 0.045, (n, L, 1)) / np.linalg.norm(offs, axis=2, keepdims=True)
        for i in range(n):
            for l in range(L):
                if (i + l) % 2:
                    continue
                r = targets[i * L + l]
                r.defined = 1
                r.pose[0:3] = list(tips[i, l] + offs[i, l])
                r.pose[3:7] = list(quat[i, l]) if (i + l) % 4 == 0 else [0, 0, 0, 0]
                r.transform[:] = [0, 0, 0, 1, 0, 0, 0]
                r.swing_clearance = 0.02 if l % 3 else 0.0
        e.set_external_target(targets, which=2 if D > 3 else 0)
        tr = np.tile(np.array([0.004, -0.003, 0.0, np.cos(0.01), 0, 0, np.sin(0.01)]), (n, L, 1))
        e.set_external_transform(tr, which=2)
        for i in range(0, n, 2):
            e.set_target_body_pose(np.array([[0.01, -0.008, 0.012, np.cos(0.02), np.sin(0.02), 0, 0]]), first=i)
        plan_until(log, steps, 100)
        snapshot(out, f"{name}.tip_targets_reached", e)
        # ---- plan step 2: a body pose alone
        e.set_target_body_pose(np.tile(np.array([0.0, 0.01, -0.01, 1.0, 0, 0, 0]), (n, 1)))
        plan_until(log, steps, 100)
        plan_until(log, steps, WAITING, limit=1)
        out[f"{name}.plan.progress"], out[f"{name}.plan.step"] = rows(log), rows(steps)
        # ---- planner off: walk again
        e.set_planner_mode(False)
        e.set_velocity(rng.uniform(-0.4, 0.4, (n, 2)), np.full(n, 0.2))
        cycles(60)
        snapshot(out, f"{name}.end", e)
    finally:
        if hasattr(e, "close"):
            e.close()
    return out


def record_sequence_case(name, make):
    """START_UP (generates the sequence), SHUT_DOWN, START_UP, finish_sequence_startup, step_to_new_stance, pack, unpack."""
    p, n = case_params(name)
    L, D = p.leg_count, p.leg_dof[0]
    rng = np.random.default_rng(SEED[name])
    ready = np.array([[p.joint[l][j].unpacked for j in range(D)] for l in range(L)])
    q0 = np.tile(ready, (n, 1, 1))
    if "own_clock" not in name:   # every robot learns its own sequence (a redundant 5-joint chain keeps its start offset along its null space to the end, and
        amplitude = 0.08 if D == 3 else 0.01   # finish_sequence_startup refuses a batch that ends more than 0.02 rad apart: a smaller offset there)
        q0[1:] += rng.uniform(-amplitude, amplitude, (n - 1, L, D))
    out = {f"{name}.posed": np.array([posed_protocol(p) and p.pose_frequency != -1.0])}
    e = make(p, n)

    def run(sequence, key, limit=6000):
        log = []
        for _ in range(limit):
            log.append(np.array(e.execute_sequence(sequence)))
            if (log[-1] == 100).all():
                out[f"{name}.sequence.{key}"] = rows(log)
                return
        raise AssertionError((name, key, "sequence did not finish", log[-1].tolist()))

    try:
        e.begin_sequence_startup(q0, True)
        run(0, "start_up_generating")
        snapshot(out, f"{name}.started", e)
        run(1, "shut_down")
        if hasattr(e, "finish_sequence_shutdown"):
            e.finish_sequence_shutdown()
        run(0, "start_up_replayed")
        e.finish_sequence_startup()
        snapshot(out, f"{name}.running", e)
        out[f"{name}.new_stance"] = rows([np.array(e.step_to_new_stance()) for _ in range(110)])
        lo = np.array([[p.joint[l][j].min for j in range(D)] for l in range(L)])
        hi = np.array([[p.joint[l][j].max for j in range(D)] for l in range(L)])
        packed = np.stack([ready + 0.5 * (rng.uniform(lo, hi) - ready), rng.uniform(lo, hi)])   # [2][legs][dof]
        for unpack in (False, True):
            log = []
            for _ in range(1000):
                log.append(e.pack_legs(packed, 2.0 / p.step_frequency, unpack))
                if log[-1] == 100:
                    break
            assert log[-1] == 100 and log.count(0) == 1, (name, unpack, log[-5:])
            out[f"{name}.{'unpack' if unpack else 'pack'}"] = rows(log)
        snapshot(out, f"{name}.end", e)
    finally:
        if hasattr(e, "close"):
            e.close()
    return out


def check_coverage(out):
    """Every branch of the loop-call driver shows in the returned arrays of `out` (all cases together)."""
    def values(part):
        return set(np.concatenate([v.ravel() for k, v in out.items() if part in k]).tolist())
    toggles = values(".toggle.")
    assert {-3, -1, 0, 1, 2} <= toggles, ("toggle results", sorted(toggles))
    plan = values(".plan.progress")
    assert {-1, -2, 100} <= plan and any(0 < v < 100 for v in plan), ("plan progress", sorted(plan))
    seq = values(".sequence.")
    assert {-1, 100} <= seq and any(0 <= v < 100 for v in seq), ("sequence progress", sorted(seq))
    posed = values(".posed")
    assert posed == {True, False}, ("the posed and the unposed protocol", posed)
    # the marked cycle follows a call in which some robot's loop was the ordinary cycle (toggle: no request or still walking; plan: still walking)
    marked = [bool(np.isin(row, (-1, -3)).any()) for k, v in out.items() if ".toggle." in k for row in v]
    marked += [bool((row == -1).any()) for k, v in out.items() if k.endswith(".plan.progress") for row in v]
    assert any(marked) and not all(marked), ("the marked cycle ran / was skipped", sum(marked), len(marked))


def engine(p, n):
    from syropod_highlevel_controller_amd.engine import BatchEngine
    return BatchEngine(p, n)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """One run of a case per session, shared by the tests below."""
    return (record_sequence_case if name in SEQUENCE_CASES else record_case)(name, engine)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", CASES + SEQUENCE_CASES)
def test_loop_level_calls_against_the_recorded_parent(golden, name):
    got = recorded(name)
    want = {k: v for k, v in golden.items() if k.startswith(name + ".")}
    assert sorted(want) == sorted(got)
    for k in sorted(want):
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and want[k].tobytes() == got[k].tobytes(), k


def test_the_run_shows_every_branch_of_the_driver(golden):
    check_coverage(golden)
    own = {}
    for name in CASES + SEQUENCE_CASES:
        own.update(recorded(name))
    check_coverage(own)


if __name__ == "__main__":   # record the golden: with the package of the commit whose behaviour is the reference on PYTHONPATH
    everything = {}
    for case in CASES + SEQUENCE_CASES:
        everything.update(recorded(case))
        print(case, "recorded", flush=True)
    check_coverage(everything)
    np.savez_compressed(sys.argv[1], **everything)
