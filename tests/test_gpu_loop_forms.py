"""GPU (-m gpu): the loop forms - shc_resident_kernel, shc_resident2_kernel, shc_batch_kernel - of EVERY morphology of SHC_FOR_EACH_MORPHOLOGY
(3 - 8 legs x 3 - 5 joints) and every feature word its KernelTable lists with a loop form in the default build: each one launched and held to
the launch form (shc_cycle_kernel through set_* + shc_engine_step(1) on a twin engine) byte for byte, the launch form held to the CPU oracle.

The loop forms carry their own copies of the tile load and store, of the per-cycle input take-over (lane < 3 * RPW, lane < RPW), of the int
write-back and of the walker / model hand-off; RPW = 64 / L is 21, 12 and 9 for 3, 5 and 7 legs (4 and 1 tail lanes of a wavefront that own no
robot; a robot-level int tile wider than a wavefront for 3 legs; an odd I_COUNT * RPW in the LDS size).  Batch sizes are 6 * RPW + RPW // 2 + 1:
seven robot groups - the last two-wavefront workgroup holds one group, the last group is partly filled.

  CASES                  (morphology, feature word, form): the table, pure data (tests/test_loop_forms_table.py holds it to the host probe of
                         csrc/shc_cycle_select.hpp without a card)
  byte identity          q / qd of all 260 cycles, the state record at the end and after 25 further plain steps
  edge shapes            1 robot and 2 * RPW robots (two full groups, one even workgroup), 20 cycles, F_C2, every form
  the oracle             engine A's q of every cycle of every case against OracleBatch free-running (1e-6 rad on the robots whose reference
                         trajectory is well-posed: a twin oracle at inputs * (1 + 1e-13) stays within 1e-9 rad; at least 0.9 of them must be),
                         and the launch forms no other test runs teacher-forced at 1e-12 rad
  which kernel ran       a fresh process per morphology logs (SHC_KERNEL_LOG) what it launches: exactly what the table promises, and every
                         loop kernel the KernelTable has
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import parity_report
from oracle_lib import OracleBatch
from syropod_highlevel_controller_amd import default_hexapod_params, synthetic_octopod_params
from syropod_highlevel_controller_amd.params import FEAT_DEFAULT, FEAT_ODOMETRY, FEAT_RESIDENT_ONE_WAVE, InstanceState
from test_cycle_select import probe, table  # noqa: F401  (probe: the module-scoped fixture that compiles the host probe)
from test_gpu_parity import make_inputs
from test_gpu_resident import imu_sample, state_bytes, velocity_schedule
from test_gpu_teacher_forced import Schedule, teacher_forced

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the case table (pure data, no GPU)
F_MANUAL, F_AUTO, F_INCL, F_IMU, F_ADM, F_TIPF, F_ODOM = 1, 2, 4, 8, 16, 32, 64
F_DYN, F_ROT, F_ROUGH, F_TALIGN, F_MLEGS = 1 << 31, 1 << 30, 1 << 29, 1 << 28, 1 << 27
F_TERRAIN = F_ROUGH | F_TALIGN | F_MLEGS
F_C2, F_C3 = F_MANUAL | F_ODOM, F_MANUAL | F_IMU | F_ADM | F_ODOM
FORM_RESIDENT, FORM_BATCH, FORM_TWO_WAVE = 1, 2, 4   # the bits of shc_select_probe_forms

# (legs, joints): gait - triples the launch-form oracle tests run (test_gpu_parity.py, test_gpu_teacher_forced.py): every gait is valid for its leg count
GAIT = {(3, 3): "wave", (4, 3): "tripod", (4, 4): "amble", (4, 5): "amble", (5, 3): "ripple", (6, 3): "tripod", (6, 4): "ripple", (6, 5): "tripod",
        (7, 3): "wave", (8, 3): "wave", (8, 4): "ripple", (8, 5): "ripple"}
MORPHOLOGIES = sorted(GAIT)
BASELINE_FAMILIES = [F_C2 | F_TIPF, F_C3, F_C3 | F_TIPF, F_C2 | F_ROUGH, F_C2 | F_TIPF | F_ROUGH]


def loop_words(legs, joints):
    """The feature words of KernelTable<legs, joints> that have a loop form in the default build, as this module promises to launch them."""
    words = [F_C2, F_DYN] + ([F_C2 | F_ROT] if joints > 3 else [])
    if (legs, joints) == (6, 3):
        words += BASELINE_FAMILIES + [F_C2 | F_TALIGN, F_C2 | F_TIPF | F_TALIGN]
    if (legs, joints) == (8, 5):
        words += BASELINE_FAMILIES + [F_C3 | F_ROT, F_C2 | F_TIPF | F_ROT]
    return words


# Loop kernels the library has and this module does not launch: {(form, legs, joints, word): why}.  Expected to stay empty: an entry is for a kernel
# that faulted or hung on the GPU with its cause not found, and is repeated in the summary of the change that adds it.
KNOWN_UNLAUNCHED = {}

# Feature words no shc_params reaches, so that no engine can launch their kernels: {(legs, joints, word): why}.  tests/test_loop_forms_table.py proves each
# entry on the host (every configuration of the probe's enumeration that selects the word is one shc_engine.hip never builds), the kernel-log test
# below shows what the recipe runs on instead.
_ROUGH_8x5 = ("rough_terrain_mode on legs of more than 3 joints tracks tip rotations (hostinit::tips_rotation_tracked: an externally requested target may "
              "define one), so cycle_params sets gravity_aligned and select_features answers F_DYN | F_ROT | F_TERRAIN; only rough_terrain without "
              "gravity_aligned selects this word, which shc_engine.hip never builds for NJ > 3")
UNREACHABLE = {(8, 5, F_C2 | F_ROUGH): _ROUGH_8x5, (8, 5, F_C2 | F_TIPF | F_ROUGH): _ROUGH_8x5}


def has_resident(word):   # (mirrors of csrc/shc_cycle_select.hpp's has_*() in a default build; held to the probe by tests/test_loop_forms_table.py)
    return not word & F_MLEGS and (not word & F_DYN or not word & (F_TERRAIN | F_ROT))


def has_batch(word):
    return not word & F_MLEGS and not word & F_DYN


def has_two_wave(word):
    return has_resident(word) and not word & (F_TERRAIN | F_ROT)


def has_helper_wave(legs, joints, word):
    return (legs, joints) == (6, 3) and word in (F_C2, F_C2 | F_TIPF)


def word_forms(word):
    """The forms of this module a feature word is run in."""
    return (["two_waves"] if has_two_wave(word) else []) + (["one_wave"] if has_resident(word) else []) + (["batch"] if has_batch(word) else [])


def logged_form(legs, joints, word, form):
    """The name shc_cycle_inst.hip logs the kernel of a form under."""
    if form == "batch":
        return "batch"
    if form == "one_wave":
        return "resident"
    return "resident3" if has_helper_wave(legs, joints, word) else "resident2"


def feature_names(word):
    bits = [(F_DYN, "DYN"), (F_ROT, "ROT"), (F_ROUGH, "ROUGH"), (F_TALIGN, "TALIGN"), (F_MLEGS, "MLEGS")]
    if word & F_DYN:
        return "+".join(n for b, n in bits if word & b)
    base = {F_C2: "C2", F_C2 | F_TIPF: "C2+TIPF", F_C3: "C3", F_C3 | F_TIPF: "C3+TIPF"}[word & 0x7F]
    return "+".join([base] + [n for b, n in bits if word & b])


def reachable_words(legs, joints):
    return [w for w in loop_words(legs, joints) if (legs, joints, w) not in UNREACHABLE]


WORD_CASES = [(legs, joints, word) for legs, joints in MORPHOLOGIES for word in reachable_words(legs, joints)]
CASES = [(legs, joints, word, form) for legs, joints, word in WORD_CASES for form in word_forms(word)
         if (logged_form(legs, joints, word, form), legs, joints, word) not in KNOWN_UNLAUNCHED]


def word_id(case):
    return f"{case[0]}x{case[1]}-{feature_names(case[2])}" + (f"-{case[3]}" if len(case) > 3 else "")


def robots_per_wave(legs):
    return 64 // legs


def batch_size(legs):
    """Seven robot groups: six full ones, the seventh partly filled - the last two-wavefront workgroup holds one group."""
    rpw = robots_per_wave(legs)
    return 6 * rpw + rpw // 2 + 1


def case_params(legs, joints, word):
    """The Params recipe of a feature word: what a user sets to land on it."""
    p = default_hexapod_params(GAIT[legs, joints]) if (legs, joints) == (6, 3) else synthetic_octopod_params(GAIT[legs, joints], joints, legs)
    if word & F_DYN:      # a runtime-flag configuration: I_APOSER and I_POSE_PHASE are live, the int write-back has something to write
        p.auto_posing = 1
    if word & F_IMU:      # the north-star set (config3_params of test_gpu_resident.py): admittance + IMU posing
        p.admittance_control, p.imu_posing = 1, 1
        p.rotation_pid_gains[:] = [0.2, 0.02, 0.01]
    if word & (F_ROT | F_TALIGN):   # tip rotations on longer legs, the tip-align pose on 3-joint legs
        p.gravity_aligned_tips = 1
    if word & F_ROUGH:
        p.rough_terrain_mode, p.step_depth = 1, 0.012
    return p


def configuration_index(p, efforts_live, features=FEAT_DEFAULT):
    """Configuration i of the host probe's enumeration (tests/cycle_select_probe.hip) that cycle_params() of shc_engine.hip builds from these Params."""
    dof = max(p.leg_dof[l] for l in range(p.leg_count))
    tip_force = bool((features & 1 or p.use_joint_effort) and efforts_live)
    tracked = dof > 3 and (p.gravity_aligned_tips or p.rough_terrain_mode)   # hostinit::tips_rotation_tracked
    switches = [p.manual_posing, p.auto_posing, p.inclination_posing, p.imu_posing, p.admittance_control, tip_force, features & 2,
                p.rough_terrain_mode, p.gravity_aligned_tips and p.leg_dof[0] <= 3, tracked]
    return sum(1 << k for k, on in enumerate(switches) if on)


# ------------------------------------------------------------------------------------------------ inputs
WARM_UP, CYCLES, FURTHER, K_BATCH = 37, 260, 25, 13
FORCE_Z = 2.0   # N: tip forces of the admittance recipes, z ~ U(0, FORCE_Z) (test_config3_wave_admittance_imu[2.0]'s scale: an offset the legs can follow)


def contact_sample(rng, n, legs):
    """Contact forces around the touchdown / lift-off thresholds (test_gpu_resident.py's rough-terrain cases)."""
    f = rng.normal(0, 0.25, (n, legs, 3))
    f[..., 2] += rng.choice([0.0, 0.05, 0.6, 1.5], size=(n, legs), p=[0.3, 0.2, 0.2, 0.3])
    return f


def input_plan(p, word, n, cycles):
    """What every cycle delivers (the callbacks of one loop iteration): a new velocity command every cycle, a third of the robots stopping and
    restarting; the other groups of the recipe are delivered every cycle too, their values change every few cycles (a tip-state message is an event
    of its own in rough terrain mode, so 'held' and 'the same again' differ there: every form gets the same deliveries)."""
    rng = np.random.default_rng(11)
    legs, dof = p.leg_count, p.leg_dof[0]
    plan = {"velocity": velocity_schedule(rng, n, cycles), "imu": None, "force": None, "effort": None, "effort0": None}

    def every(k, sample):   # message m = c // k is delivered in cycles m * k ... m * k + k - 1
        out = []
        for c in range(cycles):
            out.append(sample(c // k) if c % k == 0 else out[-1])
        return out
    if word & F_TIPF:
        plan["effort0"] = rng.normal(0, 0.5, (n, legs * dof))
        plan["effort"] = every(5, lambda m: rng.normal(0, 0.5, (n, legs * dof)))
    if word & F_IMU:
        plan["imu"] = every(2, lambda m: imu_sample(rng, n))
        plan["force"] = every(3, lambda m: np.stack([rng.normal(0, 1, (n, legs)), rng.normal(0, 1, (n, legs)), rng.uniform(0, FORCE_Z, (n, legs))], axis=2))
    if word & F_ROUGH:   # contact forces that come and go: every fourth message reports no contact at all
        plan["force"] = every(4, lambda m: contact_sample(rng, n, legs) * (0.0 if m % 4 == 3 else 1.0))
    return plan


def warm_up(o, plan, twin=1.0):
    """Some history before the compared cycles: the robots are walking when they start."""
    if plan["effort0"] is not None:   # (the tip-force estimate is live from the first torque on: the kernels with calculateTipForce)
        o.set_joint_effort(plan["effort0"])
    o.set_velocity(plan["velocity"][0][0] * twin, plan["velocity"][0][1])


def deliver(o, plan, c, twin=1.0):
    """Cycle c's inputs through the setters (engine A, the oracle and - with twin = 1 + 1e-13 on the linear velocity and the forces - its twin)."""
    o.set_velocity(plan["velocity"][c][0] * twin, plan["velocity"][c][1])
    if plan["imu"] is not None:
        o.set_imu(*plan["imu"][c])
    if plan["force"] is not None:
        o.set_tip_force(plan["force"][c] * twin)
    if plan["effort"] is not None:
        o.set_joint_effort(plan["effort"][c])


def posted(plan, c):
    kw = {"velocity": plan["velocity"][c]}
    if plan["imu"] is not None:
        kw["imu"] = plan["imu"][c]
    if plan["force"] is not None:
        kw["tip_force"] = plan["force"][c]
    if plan["effort"] is not None:
        kw["joint_effort"] = plan["effort"][c]
    return kw


# ------------------------------------------------------------------------------------------------ engine A: the launch form, once per case
@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


_reference = {}


def reference(Engine, legs, joints, word, n, cycles):
    """Engine A: setters + shc_engine_step(1) per cycle - q / qd of every cycle, the state record at the end and after FURTHER plain steps.  Computed
    once per (morphology, word, n), shared by the tests of every form and by the oracle test, never changed."""
    key = (legs, joints, word, n, cycles)
    if key not in _reference:
        p = case_params(legs, joints, word)
        plan = input_plan(p, word, n, cycles)
        a = Engine(p, n)
        warm_up(a, plan)
        a.step(WARM_UP)
        q, qd = np.empty((cycles, n, legs * joints)), np.empty((cycles, n, legs * joints))
        for c in range(cycles):
            deliver(a, plan, c)
            a.step(1)
            q[c], qd[c] = a.joints()
        end = state_bytes(a)
        a.step(FURTHER)
        later = state_bytes(a)
        a.close()
        for arr in (q, qd):
            arr.setflags(write=False)
        _reference[key] = {"params": p, "plan": plan, "q": q, "qd": qd, "end": end, "later": later}
    return _reference[key]


def first_difference(ref, c, q, qd, legs):
    """Where a loop form left engine A: cycle, robot, robot group and lane of the first differing value (a group at the tail or the last workgroup
    points at the group geometry)."""
    bad = np.argwhere((q != ref["q"][c]) | (qd != ref["qd"][c]))
    i, j = (int(v) for v in bad[0])
    rpw = robots_per_wave(legs)
    return (f"cycle {c}: {len(bad)} values differ, the first at robot {i} (group {i // rpw}, robot {i % rpw} of it) joint {j}: q {q[i, j]!r} vs {ref['q'][c][i, j]!r}, "
            f"|dq| up to {np.abs(q - ref['q'][c]).max():.3e}; robots that differ: {sorted(set(int(b[0]) for b in bad))[:24]}")


def run_resident(b, ref, legs, cycles, depth=8):
    """The same cycles through one resident launch: inputs posted up to ring_depth - 1 cycles ahead, released, every cycle's output read."""
    plan = ref["plan"]
    b.resident_begin(ring_depth=depth, max_cycles=cycles + 10, idle_timeout_ms=2000)   # (a stuck loop leaves by itself)
    for c0 in range(0, cycles, depth - 1):
        c1 = min(cycles, c0 + depth - 1)
        for c in range(c0, c1):
            assert b.resident_post(**posted(plan, c)) == c
        b.resident_publish(c1 - c0)
        b.resident_wait(c1)
        for c in range(c0, c1):
            q, qd = b.resident_joints(c)
            assert q.tobytes() == ref["q"][c].tobytes() and qd.tobytes() == ref["qd"][c].tobytes(), first_difference(ref, c, q, qd, legs)
    assert b.resident_end() == cycles


def run_batch(b, ref, legs, cycles):
    """The same cycles as launches of K_BATCH cycles from K-deep device arrays, every cycle read from the K-deep output ring."""
    import torch
    plan = ref["plan"]
    for c0 in range(0, cycles, K_BATCH):
        c1 = min(cycles, c0 + K_BATCH)
        rows = {"lin": np.stack([plan["velocity"][c][0] for c in range(c0, c1)]), "ang": np.stack([plan["velocity"][c][1] for c in range(c0, c1)])}
        if plan["imu"] is not None:
            rows["imu_q"], rows["imu_w"] = np.stack([plan["imu"][c][0] for c in range(c0, c1)]), np.stack([plan["imu"][c][1] for c in range(c0, c1)])
        for key in ("force", "effort"):
            if plan[key] is not None:
                rows[key] = np.stack(plan[key][c0:c1])
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in rows.items()}
        torch.cuda.synchronize()
        ptr = lambda k: dev[k].data_ptr() if k in dev else None
        b.step_k(c1 - c0, velocity=(ptr("lin"), ptr("ang")), imu=(ptr("imu_q"), ptr("imu_w")) if "imu_q" in dev else None, tip_force=ptr("force"),
                 joint_effort=ptr("effort"))
        b.synchronize()
        for c in range(c0, c1):
            q, qd = b.step_k_joints(c - c0)
            assert q.tobytes() == ref["q"][c].tobytes() and qd.tobytes() == ref["qd"][c].tobytes(), first_difference(ref, c, q, qd, legs)
        del dev


def check_form(Engine, legs, joints, word, form, n, cycles):
    ref = reference(Engine, legs, joints, word, n, cycles)
    b = Engine(ref["params"], n)
    if form == "one_wave":
        b.set_features(FEAT_DEFAULT | FEAT_RESIDENT_ONE_WAVE)
    warm_up(b, ref["plan"])
    b.step(WARM_UP)
    if form == "batch":
        run_batch(b, ref, legs, cycles)
    else:
        run_resident(b, ref, legs, cycles)
    q, qd = b.joints()
    assert q.tobytes() == ref["q"][cycles - 1].tobytes() and qd.tobytes() == ref["qd"][cycles - 1].tobytes()
    assert state_bytes(b) == ref["end"], state_difference(b, ref["end"], legs)
    b.step(FURTHER)   # ... and the engine goes on identically through ordinary launches: the inputs of the last cycle were carried over
    assert state_bytes(b) == ref["later"], state_difference(b, ref["later"], legs)
    b.close()


def state_difference(b, want, legs):
    got, want = np.frombuffer(b.get_state(), dtype=np.dtype(InstanceState)), np.frombuffer(want, dtype=np.dtype(InstanceState))
    fields = [f for f in got.dtype.names if got[f].tobytes() != want[f].tobytes()]
    robots = sorted(set(int(i) for f in fields for i in np.flatnonzero([got[f][i].tobytes() != want[f][i].tobytes() for i in range(len(got))])))
    return f"state fields that differ: {fields}; robots {robots[:24]} ({robots_per_wave(legs)} robots per group)"


# ------------------------------------------------------------------------------------------------ byte identity
@pytest.mark.parametrize("case", CASES, ids=word_id)
def test_loop_form_is_byte_identical_to_single_cycle_launches(Engine, case):
    """Engine A: set_* + shc_engine_step(1) per cycle.  Engine B: the same 260 cycles in one loop form - two_waves: one resident launch (the three-role
    form on 6 x 3 F_C2 [| F_TIPF]); one_wave: the same under FEAT_RESIDENT_ONE_WAVE; batch: 20 launches of shc_engine_step_k over 13-deep device arrays.
    q / qd of EVERY cycle, the complete state record at the end and after 25 further plain steps are equal byte for byte."""
    legs, joints, word, form = case
    check_form(Engine, legs, joints, word, form, batch_size(legs), CYCLES)


@pytest.mark.parametrize("form", ["two_waves", "one_wave", "batch"])
@pytest.mark.parametrize("groups", [0, 2], ids=["one_robot", "two_full_groups"])
@pytest.mark.parametrize("legs,joints", MORPHOLOGIES)
def test_loop_form_edge_shapes(Engine, legs, joints, groups, form):
    """One robot (a single live group in a workgroup whose second wavefront pair idles) and 2 * RPW robots (two full groups, one even workgroup, no
    partly filled group): default.yaml's posing set, 20 cycles, every form, the same byte identity."""
    check_form(Engine, legs, joints, F_C2, form, groups * robots_per_wave(legs) or 1, 20)


# ------------------------------------------------------------------------------------------------ the oracle
_oracle = {}


def oracle_run(legs, joints, word, n, cycles):
    """OracleBatch free-running on the inputs of engine A, and its twin at linear velocity and forces * (1 + 1e-13): q of every cycle, which robots are
    still well-posed after every cycle (a robot is out once the twins differ by more than 1e-9 rad) and the state record at the end.  CPU only."""
    key = (legs, joints, word, n, cycles)
    if key not in _oracle:
        p = case_params(legs, joints, word)
        plan = input_plan(p, word, n, cycles)
        ob, tw = OracleBatch(p, n), OracleBatch(p, n)
        for o, k in ((ob, 1.0), (tw, 1 + 1e-13)):
            warm_up(o, plan, k)
            o.step(WARM_UP, 8)
        q, well = np.empty((cycles, n, legs * joints)), np.ones((cycles, n), dtype=bool)
        for c in range(cycles):
            for o, k in ((ob, 1.0), (tw, 1 + 1e-13)):
                deliver(o, plan, c, k)
                o.step(1, 8)
            q[c] = ob.joints()[0]
            well[c] = (well[c - 1] if c else True) & (np.abs(q[c] - tw.joints()[0]).max(axis=1) <= 1e-9)
        _oracle[key] = (q, well, np.frombuffer(ob.get_state(), dtype=np.dtype(InstanceState)).copy(), ob.leg_state())
    return _oracle[key]


def recipe_is_live(p, word, q, state, leg_state):
    """The recipe does what it is there for (the reference's own state: a dead feature would be byte-identical in every form too)."""
    assert np.abs(q[-1] - q[0]).max() > 1e-2                        # the robots walk
    if word & F_DYN:                                                 # I_APOSER / I_POSE_PHASE: the auto-pose cycle runs
        assert state["auto_posing_state"].any() or state["pose_phase"].any() or state["auto_poser_flags"].any()
    if word & F_TIPF:
        assert np.abs(leg_state["tip_force"]).max() > 1e-3           # Leg::calculateTipForce is being evaluated
    if word & F_ADM:
        assert np.abs(leg_state["admittance"]).max() > 1e-5          # the admittance offsets move the tips
    if word & F_ROUGH:
        d = state["leg"]["step_plane_defined"][:, :p.leg_count]
        assert d.any() and not d.all()                               # touchdowns detected, not everywhere
    if word & F_TALIGN:
        assert max(np.abs(state["tip_align_pose"][:, :3]).max(), np.abs(state["origin_tip_align_pose"][:, :3]).max()) > 1e-4


@pytest.mark.parametrize("case", WORD_CASES, ids=word_id)
def test_launch_form_matches_the_oracle_free_running(Engine, case):
    """Engine A's q of EVERY cycle (what the loop forms are held to, byte for byte) against the CPU oracle free-running on the same inputs: 1e-6 rad on
    the robots whose reference trajectory is well-posed (twin oracle), which at least 0.9 of them must be."""
    legs, joints, word = case
    n = batch_size(legs)
    ref = reference(Engine, legs, joints, word, n, CYCLES)
    q, well, state, leg_state = oracle_run(legs, joints, word, n, CYCLES)
    recipe_is_live(ref["params"], word, q, state, leg_state)
    worst = max(float(np.abs(ref["q"][c] - q[c])[well[c]].max()) if well[c].any() else 0.0 for c in range(CYCLES))
    share = float(well[-1].mean())
    parity_report(f"[loop forms {word_id(case)}] {n} robots x {CYCLES} cycles, new inputs every cycle, free-running: max |dq| vs oracle = {worst:.2e} rad over "
                  f"the well-posed share {share:.3f}")
    assert share >= 0.9, share
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("efforts_live", [False, True], ids=["C3", "C3+TIPF"])
def test_octopod_north_star_launch_forms_teacher_forced(Engine, efforts_live):
    """shc_cycle_kernel<8, 5, F_C3 [| F_TIPF]>, the launch forms the loop forms above are held to: the oracle's complete state loaded before every
    cycle, one cycle, every field of every robot compared (test_gpu_teacher_forced.py's 1e-12 rad bar).  F_C3 without the tip-force estimate is
    FEAT_ODOMETRY alone (no other test runs the octopods on it)."""
    p = case_params(8, 5, F_C3)
    n, cycles = 40, 150
    inp = make_inputs(p, n, 851, imu=True, force=FORCE_Z, zero_every=9)
    rng = np.random.default_rng(852)
    sched = Schedule()
    for c in range(10, cycles, 10):
        sched.at(c, force=np.stack([rng.normal(0, 1, (n, 8)), rng.normal(0, 1, (n, 8)), rng.uniform(0, FORCE_Z, (n, 8))], axis=2))
    for c in range(17, cycles, 17):
        fresh = make_inputs(p, n, 860 + c, imu=True)
        sched.at(c, imu_q=fresh["imu_q"], gyro=fresh["gyro"])
    sched.at(70, lin=np.zeros((n, 2)), ang=np.zeros(n))
    sched.at(110, lin=inp["lin"], ang=-inp["ang"])
    teacher_forced(Engine, p, n, inp, cycles, sched, features=FEAT_DEFAULT if efforts_live else FEAT_ODOMETRY,
                   label=f"loop forms 8x5 {'C3+TIPF' if efforts_live else 'C3'}")


# ------------------------------------------------------------------------------------------------ which kernel actually ran, and completeness
def expected_log(legs, joints):
    """(form, legs, joints, word) of every loop kernel the child process of a morphology launches: what CASES promises."""
    return {(logged_form(l, j, word, form), l, j, word) for l, j, word, form in CASES if (l, j) == (legs, joints)}


def shipped_loop_kernels(P, legs, joints):
    """(form, legs, joints, word) of every loop kernel libshc_batch.so has for a morphology in the default build: the KernelTable through the host
    probe; the three-role form takes the place of the two-wavefront form where there is one."""
    out = set()
    for word in table(P, legs, joints):
        forms = int(P.shc_select_probe_forms(word))
        out |= {(name, legs, joints, word) for bit, name in ((FORM_RESIDENT, "resident"), (FORM_BATCH, "batch"),
                                                             (FORM_TWO_WAVE, "resident3" if has_helper_wave(legs, joints, word) else "resident2")) if forms & bit}
    return out


def child_main(legs, joints):
    """Runs in a fresh process (SHC_KERNEL_LOG in its environment): 2 cycles of every case and form of one morphology."""
    from syropod_highlevel_controller_amd.engine import BatchEngine
    n = 3
    for l, j, word, form in CASES:
        if (l, j) != (legs, joints):
            continue
        p = case_params(l, j, word)
        e = BatchEngine(p, n)
        if word & F_TIPF:
            e.set_joint_effort(np.full((n, l * j), 0.1))
        e.set_velocity(np.full((n, 2), 0.3), np.full(n, 0.2))
        if form == "batch":
            e.step_k(2)
            e.synchronize()
        else:
            if form == "one_wave":
                e.set_features(FEAT_DEFAULT | FEAT_RESIDENT_ONE_WAVE)
            e.resident_begin(ring_depth=4, max_cycles=8, idle_timeout_ms=2000)
            e.resident_publish(2)
            e.resident_wait(2)
            assert e.resident_end() == 2
        e.close()
    for l, j, word in UNREACHABLE:   # what the recipe of an unreachable word runs on instead: a launch form, and no loop form at all
        if (l, j) == (legs, joints):
            e = BatchEngine(case_params(l, j, word), n)
            if word & F_TIPF:
                e.set_joint_effort(np.full((n, l * j), 0.1))
            e.step(2)
            e.synchronize()
            try:
                e.resident_begin(ring_depth=4, max_cycles=8, idle_timeout_ms=2000)
            except RuntimeError as err:
                print(f"no-loop-form {word}: {err}")
            else:
                e.resident_end()
            e.close()


@pytest.mark.parametrize("legs,joints", MORPHOLOGIES)
def test_which_loop_kernels_a_process_launches(probe, tmp_path, legs, joints):   # noqa: F811
    """The forms are byte-identical by design, so the tests above cannot tell them apart: a fresh process runs 2 cycles of every case and form of a
    morphology and logs the kernels it launches.  The logged loop kernels are exactly what the table promises, and they are every loop kernel the
    library has for the morphology - nothing the KernelTable lists with a loop form is left out but what KNOWN_UNLAUNCHED / UNREACHABLE write down."""
    log = tmp_path / "kernels.txt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SHC_KERNEL_LOG=str(log), PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")] + [v for v in [os.environ.get("PYTHONPATH")] if v]))
    env.pop("SHC_RESIDENT_TWO_ROLE", None)
    run = subprocess.run([sys.executable, "-c", f"import test_gpu_loop_forms as t; t.child_main({legs}, {joints})"], cwd=root, env=env, timeout=300,
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [line.split() for line in log.read_text().splitlines()]
    launched = {(form, int(l), int(j), int(word)) for form, l, j, word in lines}
    loops = {k for k in launched if k[0] != "cycle" and k[0] != "half"}
    assert loops == expected_log(legs, joints), (sorted(loops - expected_log(legs, joints)), sorted(expected_log(legs, joints) - loops))
    unreachable = {(form, legs, joints, word) for (l, j, word) in UNREACHABLE if (l, j) == (legs, joints) for form in ("resident", "batch")}
    shipped = shipped_loop_kernels(probe, legs, joints)
    assert set(KNOWN_UNLAUNCHED) & loops == set() and unreachable <= shipped
    missing = shipped - loops - set(KNOWN_UNLAUNCHED) - unreachable
    assert not missing, f"loop kernels of the default build that nothing here launches: {sorted(missing)}"
    assert loops <= shipped, sorted(loops - shipped)
    for (l, j, word) in UNREACHABLE:   # the recipe of an unreachable word runs on the runtime-flag kernel with rough terrain and tip rotations: no loop form
        if (l, j) == (legs, joints):
            assert ("cycle", legs, joints, F_DYN | F_ROT | F_TERRAIN) in launched and f"no-loop-form {word}" in run.stdout, run.stdout[-2000:]
            assert not any(k[3] == word for k in launched)
