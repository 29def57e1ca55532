"""CPU: the case table of tests/test_gpu_loop_forms.py - which loop kernels that module promises to launch - held to the host probe of
csrc/shc_cycle_select.hpp (tests/cycle_select_probe.hip: select_features, KernelTable, has_*()), without a card: every recipe lands on its feature
word, the table lists every word of every KernelTable that has a loop form in the default build, the batch sizes put a partly filled seventh group
into the last workgroup, and a word written down as unreachable is one no shc_params can select."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_loop_forms as T
from test_cycle_select import GOLDEN_MORPHOLOGIES, probe, selected, table  # noqa: F401  (probe: the fixture that compiles the host probe)


def test_the_table_covers_every_morphology():
    assert T.MORPHOLOGIES == sorted(GOLDEN_MORPHOLOGIES) and len(T.MORPHOLOGIES) == 12
    assert {legs: T.batch_size(legs) for legs in range(3, 9)} == {3: 137, 4: 105, 5: 79, 6: 66, 7: 59, 8: 53}
    for legs in range(3, 9):
        rpw, n = T.robots_per_wave(legs), T.batch_size(legs)
        groups = -(-n // rpw)
        assert groups == 7 and 0 < n - 6 * rpw < rpw            # seven groups: the last workgroup holds one, partly filled
    assert all(isinstance(why, str) and why for why in T.KNOWN_UNLAUNCHED.values())   # (empty today; an entry carries its reason)
    assert len(T.CASES) == len(set(T.CASES)) and len(T.WORD_CASES) == len(set(T.WORD_CASES))


def test_form_predicates_are_the_headers(probe):   # noqa: F811
    for legs, joints in T.MORPHOLOGIES:
        for word in table(probe, legs, joints):
            want = (T.FORM_RESIDENT if T.has_resident(word) else 0) | (T.FORM_BATCH if T.has_batch(word) else 0) | (T.FORM_TWO_WAVE if T.has_two_wave(word) else 0)
            assert int(probe.shc_select_probe_forms(word)) & 7 == want, (legs, joints, hex(word))
    assert {k for k in T.CASES if T.logged_form(*k) == "resident3"} == {(6, 3, w, "two_waves") for w in (T.F_C2, T.F_C2 | T.F_TIPF)}


@pytest.mark.parametrize("legs,joints", T.MORPHOLOGIES)
def test_the_table_lists_every_loop_word_of_the_kernel_table(probe, legs, joints):   # noqa: F811
    with_loop_form = {w for w in table(probe, legs, joints) if int(probe.shc_select_probe_forms(w)) & (T.FORM_RESIDENT | T.FORM_BATCH | T.FORM_TWO_WAVE)}
    assert set(T.loop_words(legs, joints)) == with_loop_form, sorted(hex(w) for w in set(T.loop_words(legs, joints)) ^ with_loop_form)
    assert T.expected_log(legs, joints) | {(form, legs, joints, w) for (l, j, w) in T.UNREACHABLE if (l, j) == (legs, joints) for form in ("resident", "batch")} \
        == T.shipped_loop_kernels(probe, legs, joints)


@pytest.mark.parametrize("case", T.WORD_CASES, ids=T.word_id)
def test_every_recipe_selects_its_feature_word(probe, case):   # noqa: F811
    legs, joints, word = case
    p = T.case_params(legs, joints, word)
    assert int(selected(probe, legs, joints)[T.configuration_index(p, bool(word & T.F_TIPF))]) == word
    if word & T.F_TIPF:   # (until a joint torque has been supplied the kernels without the estimate run)
        assert int(selected(probe, legs, joints)[T.configuration_index(p, False)]) == word & ~T.F_TIPF
    plan = T.input_plan(p, word, 5, 20)
    assert (plan["effort"] is not None) == bool(word & T.F_TIPF) and (plan["imu"] is not None) == bool(word & T.F_IMU)
    assert (plan["force"] is not None) == bool(word & (T.F_ADM | T.F_ROUGH))
    again = T.input_plan(p, word, 5, 20)   # the plan is a function of the case alone: engine A, engine B and the oracle see the same cycles
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(plan["velocity"], again["velocity"]))


@pytest.mark.parametrize("key", sorted(T.UNREACHABLE), ids=lambda k: T.word_id(k))
def test_an_unreachable_word_is_one_no_parameter_set_selects(probe, key):   # noqa: F811
    """Every configuration of the enumeration that selects the word has rough_terrain without gravity_aligned; cycle_params() of shc_engine.hip sets
    gravity_aligned = tips_rotation_tracked = NJ > 3 && (gravity_aligned_tips || rough_terrain_mode), so for these legs it builds none of them - and the
    recipe that would be the word's lands on the runtime-flag kernel with rough terrain and tip rotations, which has no loop form."""
    legs, joints, word = key
    assert joints > 3
    sel = selected(probe, legs, joints)
    hits = np.flatnonzero(sel == np.uint32(word))
    assert hits.size and all(i >> 7 & 1 and not i >> 9 & 1 for i in hits)
    p = T.case_params(legs, joints, word)
    got = int(sel[T.configuration_index(p, bool(word & T.F_TIPF))])
    assert got == T.F_DYN | T.F_ROT | T.F_TERRAIN and not T.has_resident(got) and not T.has_batch(got)
    assert C.c_uint32(probe.shc_select_probe_forms(got)).value & 7 == 0
