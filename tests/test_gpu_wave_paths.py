"""GPU (-m gpu): both sides of every wave-uniform shortcut of the cycle kernels, held to the oracle.

The scenarios of tests/wave_paths.py - every robot of a wave on the common side of a guard, then ONE robot of the wave (in its first group, an inner one, its
last, the last robot of the partial wave) on the other side, then every robot - run through the teacher-forced comparison of tests/test_gpu_teacher_forced.py
(teacher_forced / compare_records, imported: every field of every instance, 1e-12 rad, no mask).  The schedule keeps the oracle's record of every cycle of
this very run; the classifier says from them which side of each guard each wave was on in each cycle, and the coverage the CPU test shows for the scenarios
(tests/test_wave_paths_table.py) is asserted again for what was compared here.
"""
import pytest

import wave_paths as W
from conftest import parity_report
from test_gpu_teacher_forced import teacher_forced

pytestmark = pytest.mark.gpu
CYCLES = 150


@pytest.fixture(scope="module")
def Engine():
    from syropod_highlevel_controller_amd import engine
    if engine.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run the native HIP path")
    return engine.BatchEngine


@pytest.mark.parametrize("name", list(W.MORPHS))
def test_both_sides_of_every_guard_teacher_forced(Engine, name):
    guards = W.guards_of(name)
    total = W.Tally()
    for kind, position in W.MORPHS[name][3]:
        p, n, inp, sched = W.build_scenario(name, kind, position, CYCLES)
        label = f"wave paths {name} {kind} {position}"
        eng, ob, worst = teacher_forced(Engine, p, n, inp, CYCLES, sched, label=label)
        eng.close()
        assert sorted(sched.records) == list(range(CYCLES))
        t = W.tally_run(p, sched, W.as_np(ob.get_state()), CYCLES, guards)
        parity_report(f"[{label}] max |dq| = {worst:.3e} rad; wave-cycles " + "; ".join(t.line(g.id) for g in guards))
        total.merge(t)
    missing = total.missing(guards)
    assert not missing, f"{name}: fewer than {W.K_MIN} compared wave-cycles of (guard, class, count): {missing}"


def test_resident_loop_memos_hit_and_miss_per_wave(Engine):
    """The memos that live across cycles - the bearing-bracket memo of the velocity front (fb.limit_bracket / limit_value) and the odometry's OdomCache - exist in
    the resident 6 x 3 loop only: every launch form, step_k's batch kernel included, starts each cycle with fresh ones (cycle(), shc_cycle.hpp).  The loop in its
    default form, driven as tests/test_gpu_resident_front.py drives it, against a twin engine stepped by single launches (the form the teacher-forced test above
    holds to the oracle), byte for byte: q / qd of every cycle, the state record and the odometry at the end.  From the twin's records the classifier counts,
    per wave, the hits, the misses one robot caused (first / last group, partial wave) and the hits right after a miss."""
    import numpy as np
    p, n = W.loop_params(), W.batch_size(6)
    plan = W.loop_plan(n)

    def prepare():
        e = Engine(p, n)
        e.set_pose_input(np.zeros((n, 3)), np.zeros((n, 3)))
        e.set_velocity(*plan[0])
        e.step(W.LOOP_HISTORY)
        return e
    state_bytes = lambda e: bytes(memoryview(e.get_state()).cast("B"))
    a, records, joints = prepare(), [], []
    for lin, ang in plan:
        a.set_velocity(lin, ang)
        records.append(W.as_np(a.get_state()))
        a.step(1)
        joints.append(a.joints())
    records.append(W.as_np(a.get_state()))
    t = W.tally_loop(p, records, plan, W.memo_guards())
    missing = W.loop_missing(t, W.memo_guards())
    assert not missing, f"fewer than {W.K_MIN} wave-cycles of (guard, class, count): {missing}"
    b = prepare()
    b.resident_begin(ring_depth=8, max_cycles=W.LOOP_CYCLES + 10)
    for c, (lin, ang) in enumerate(plan):
        b.resident_post(velocity=(lin, ang))
        b.resident_publish(1)
        b.resident_wait(c + 1)
        q, qd = b.resident_joints(c)
        assert np.array_equal(q, joints[c][0]) and np.array_equal(qd, joints[c][1]), f"cycle {c}"
    assert b.resident_end() == W.LOOP_CYCLES
    assert state_bytes(b) == state_bytes(a)
    assert np.array_equal(b.odometry(), a.odometry()) and np.abs(a.odometry()[:, :2]).max() > 1e-3
    parity_report("[wave paths resident 6x3 memos] byte-identical to single launches; wave-cycles " +
                  "; ".join(f"{t.line(g.id)}, {W.HIT_AFTER_MISS} {t.counts[g.id][W.HIT_AFTER_MISS]}" for g in W.memo_guards()))
    a.close()
    b.close()


def _post_kwargs(ev):
    kw = {}
    if "lin" in ev:
        kw["velocity"] = (ev["lin"], ev["ang"])
    if "tv" in ev:
        kw["pose_input"] = (ev["tv"], ev["rv"])
    if "reset" in ev:
        kw["pose_reset_mode"] = ev["reset"]
    return kw


def test_scenarios_through_the_resident_loop_and_step_k(Engine):
    """The 6 x 3 scenarios - clamp, pose and reset, a lone stop; a stop of every robot and a lone restart; a start from rest of every robot but one - on the
    configuration whose resident loop keeps memos and runs the resident-only vote sites, three ways: (a) a twin engine, setters + shc_engine_step(1) per cycle (the
    form test_both_sides_of_every_guard_teacher_forced[6x3-loop] holds to the oracle); (b) the resident loop in its default form, ended and begun again at the
    scenario's cuts, driven as tests/test_gpu_resident_front.py drives it (ring posts where an input changes, bare publishes in between); (c) step_k launches as
    tests/test_gpu_step_k.py drives them, one per stretch between pose inputs (which step_k does not carry).  (b) and (c) equal (a) byte for byte: q / qd of every
    cycle, the state record at the end of every launch, the odometry.  The classifier counts from the twin's records which side of every loop-only guard each
    wave was on: memo hits and misses per wave, misses one robot caused, hits right after a miss (step_k keeps no memo - cycle() starts each cycle with fresh
    ones - so for it the comparison is what is asked)."""
    import numpy as np
    import torch
    from test_gpu_parity import apply
    state_bytes = lambda e: bytes(memoryview(e.get_state()).cast("B"))
    total = W.Tally()
    for kind, position in W.MORPHS["6x3-loop"][3]:
        p, n, inp, sched = W.build_scenario("6x3-loop", kind, position, CYCLES)
        label = f"{kind} {position}"
        a, b, k = Engine(p, n), Engine(p, n), Engine(p, n)
        for e in (a, b, k):
            apply(e, inp)
        sched.recorder = a
        joints, after, odom = [], [], []
        for c in range(CYCLES):
            sched.fire(c, (a,))
            a.step(1)
            joints.append(a.joints())
            after.append(state_bytes(a))
            odom.append(a.odometry().copy())
        t = W.tally_loop_run(p, sched, W.as_np(a.get_state()), CYCLES)
        total.merge(t)
        # (b) the resident loop
        bounds = [0] + list(sched.cuts) + [CYCLES]
        for c0, c1 in zip(bounds[:-1], bounds[1:]):
            b.resident_begin(ring_depth=8, max_cycles=c1 - c0 + 10)
            for c in range(c0, c1):
                kw = _post_kwargs(sched.events.get(c, {}))
                if kw:
                    b.resident_post(**kw)
                b.resident_publish(1)
                b.resident_wait(c - c0 + 1)
                q, qd = b.resident_joints(c - c0)
                assert np.array_equal(q, joints[c][0]) and np.array_equal(qd, joints[c][1]), f"resident loop, {label}, cycle {c}"
            assert b.resident_end() == c1 - c0
            assert state_bytes(b) == after[c1 - 1], f"resident loop, {label}, state after cycle {c1 - 1}"
            assert np.array_equal(b.odometry(), odom[c1 - 1]), f"resident loop, {label}, odometry after cycle {c1 - 1}"
        # (c) step_k: one launch per stretch between pose inputs
        starts = sorted({0} | {c for c, ev in sched.events.items() if "tv" in ev or "reset" in ev})
        held = {"lin": np.array(inp["lin"]), "ang": np.array(inp["ang"])}
        for c0, c1 in zip(starts, starts[1:] + [CYCLES]):
            ev = sched.events.get(c0, {})
            if "tv" in ev:
                k.set_pose_input(ev["tv"], ev["rv"])
            if "reset" in ev:
                k.set_pose_reset_mode(ev["reset"])
            lin, ang = [], []
            for c in range(c0, c1):
                if "lin" in sched.events.get(c, {}):
                    held = {"lin": np.array(sched.events[c]["lin"]), "ang": np.array(sched.events[c]["ang"])}
                lin.append(held["lin"])
                ang.append(held["ang"])
            lin_d, ang_d = torch.from_numpy(np.ascontiguousarray(np.stack(lin))).cuda(), torch.from_numpy(np.ascontiguousarray(np.stack(ang))).cuda()
            torch.cuda.synchronize()
            k.step_k(c1 - c0, velocity=(lin_d.data_ptr(), ang_d.data_ptr()))
            k.synchronize()
            for c in range(c0, c1):
                q, qd = k.step_k_joints(c - c0)
                assert q.tobytes() == joints[c][0].tobytes() and qd.tobytes() == joints[c][1].tobytes(), f"step_k, {label}, cycle {c}"
            assert state_bytes(k) == after[c1 - 1], f"step_k, {label}, state after cycle {c1 - 1}"
            del lin_d, ang_d
        parity_report(f"[wave paths 6x3 loop forms {label}] resident loop ({len(bounds) - 1} launches) and step_k ({len(starts)} launches) byte-identical to single "
                      "launches; wave-cycles " + "; ".join(t.line(g.id) for g in W.loop_guards()))
        for e in (a, b, k):
            e.close()
    missing = W.loop_missing(total)
    assert not missing, f"fewer than {W.K_MIN} wave-cycles (or launches) of (guard, class, count): {missing}"
