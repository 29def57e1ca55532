"""CPU (-m "not gpu"): the table of wave-uniform shortcuts (tests/wave_paths.py) against the sources, and the scenarios against the table - on the oracle alone.

1. Source scan: every `__all(` / `__any(` / `__ballot(` of csrc/shc_cycle.hpp, shc_walk_front_body.hpp and shc_cycle_kernel.hpp is named by exactly one entry
   (guard or exempt) - by file, enclosing function, quoted text and occurrence - and every entry names a line.  A new or reworded vote fails here until
   someone classifies it.
2. Coverage: the scenarios of every morphology, run through OracleBatch and classified, reach K_MIN wave-cycles of every class each guard can have:
   both uniform sides, and one robot against the rest in the first group, the last group and the partial wave.
"""
import os
import shutil

import pytest

import wave_paths as W

CYCLES = 150


def test_every_wave_vote_in_the_sources_is_in_the_table():
    found = W.scan_sources()
    assert len(found) == len(W.GUARDS) + len(W.EXEMPT) and {f[0] for f in found} == set(W.FILES), "the scan lost the sources"
    problems = W.match_sources(found)
    assert not problems, "\n".join(problems)
    ids = [g.id for g in W.GUARDS]
    assert len(ids) == len(set(ids))
    for g in W.GUARDS:
        assert all(c in W.REQUIRED and reason for c, reason in g.waived.items()), g.id
    assert all(e[4] for e in W.EXEMPT), "every exempt site says why"


def test_the_scan_notices_a_missing_entry_and_a_new_vote(tmp_path):
    found = W.scan_sources()
    fewer = [g for g in W.GUARDS if g.id != "walk.steady"]
    assert any("steady" in p for p in W.match_sources(found, guards=fewer))
    for f in W.FILES:
        shutil.copy(os.path.join(W.CSRC, f), tmp_path / f)
    with open(tmp_path / "shc_cycle.hpp", "a") as fh:
        fh.write("__device__ __forceinline__ bool new_shortcut(bool b) {\n  return __all(b);\n}\n")
    problems = W.match_sources(W.scan_sources(str(tmp_path)))
    assert len(problems) == 1 and "new_shortcut" in problems[0] and "matches 0 entries" in problems[0]


def test_wave_of_and_the_designated_robots():
    assert W.wave_of([0, 9, 10, 19, 20, 24], 6).tolist() == [0, 0, 1, 1, 2, 2]
    assert W.wave_of([20, 21, 41, 42], 3).tolist() == [0, 1, 1, 2]
    assert [W.batch_size(L) for L in (3, 5, 6, 7, 8)] == [53, 30, 25, 23, 20]
    assert W.designated(25, 6, "first").tolist() == [0, 10, 24] and W.designated(25, 6, "last").tolist() == [9, 19, 24]
    assert W.designated(20, 8, "inner").tolist() == [4, 12, 19]


def test_classify_wave():
    import numpy as np
    v = lambda *a: np.array(a, dtype=np.int8)
    Y, N, U, A = W.YES, W.NO, W.UNSURE, W.ABSENT
    assert W.classify_wave("all", v(Y, Y, Y)) == (W.UNIFORM_TAKEN, None)
    assert W.classify_wave("all", v(N, N, A)) == (W.UNIFORM_NOT_TAKEN, None)
    assert W.classify_wave("all", v(Y, A, N, Y)) == ("LONE", 2)
    assert W.classify_wave("all", v(N, Y, N))[0] == W.MIXED          # one YES among NOs does not change what an __all does
    assert W.classify_wave("any", v(N, Y, N)) == ("LONE", 1)
    assert W.classify_wave("any", v(Y, Y, N))[0] == W.MIXED
    assert W.classify_wave("any", v(Y, U, N))[0] == W.UNDECIDED
    assert W.classify_wave("any", v(A, A))[0] == W.NOT_REACHED


@pytest.mark.parametrize("name", list(W.MORPHS))
def test_the_scenarios_reach_every_side_of_every_guard(name):
    guards = W.guards_of(name)
    assert guards
    total = W.Tally()
    for kind, position in W.MORPHS[name][3]:
        p, n, inp, sched = W.build_scenario(name, kind, position, CYCLES)
        rpw = 64 // p.leg_count
        assert n == 2 * rpw + (rpw + 1) // 2 and max(sched.events) < CYCLES <= 150   # two full waves and a partial one (25 hexapods)
        ob = W.oracle_run(p, n, inp, sched, CYCLES)
        total.merge(W.tally_run(p, sched, W.as_np(ob.get_state()), CYCLES, guards))
    missing = total.missing(guards)
    assert not missing, f"{name}: fewer than {W.K_MIN} wave-cycles of (guard, class, count): {missing}\n" + "\n".join(total.line(g.id) for g in guards)


def test_the_loop_plan_reaches_every_side_of_the_memo_guards():
    """The resident loop's memos (bracket memo, odometry cache) on the oracle's trajectory of the plan the GPU test runs: hits, misses that one robot causes in the
    first / last group and in the partial wave, hits right after a miss."""
    from oracle_lib import OracleBatch
    p, n = W.loop_params(), W.batch_size(6)
    plan = W.loop_plan(n)
    ob = OracleBatch(p, n)
    ob.set_velocity(*plan[0])
    ob.step(W.LOOP_HISTORY, 8)
    records = []
    for lin, ang in plan:
        ob.set_velocity(lin, ang)
        records.append(W.as_np(ob.get_state()))
        ob.step(1, 8)
    records.append(W.as_np(ob.get_state()))
    t = W.tally_loop(p, records, plan, W.memo_guards())
    assert not W.loop_missing(t, W.memo_guards()), (W.loop_missing(t, W.memo_guards()), [t.line(g.id) for g in W.memo_guards()])


def test_the_loop_runs_reach_every_side_of_the_loop_only_guards():
    """The 6 x 3 scenarios as the GPU test cuts them into resident launches, on the oracle's trajectory: the resident-only vote sites and the memos."""
    total = W.Tally()
    for kind, position in W.MORPHS["6x3-loop"][3]:
        p, n, inp, sched = W.build_scenario("6x3-loop", kind, position, CYCLES)
        ob = W.oracle_run(p, n, inp, sched, CYCLES)
        total.merge(W.tally_loop_run(p, sched, W.as_np(ob.get_state()), CYCLES))
    missing = W.loop_missing(total)
    assert not missing, (missing, [total.line(g.id) for g in W.loop_guards()])
