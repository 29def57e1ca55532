"""CPU: which fused cycle kernel every configuration runs on (csrc/shc_cycle_select.hpp: select_features, KernelTable), enumerated through
the host probe tests/cycle_select_probe.hip and held to a recorded table - for all 12 morphologies, the 7 feature switches x rough_terrain x
tip_align x gravity_aligned x (joint_control == 2) x RT_MANUAL_LEGS x the generic flag: 8 192 configurations per morphology, every one compared.

The expected feature words (tests/golden/cycle_select_golden.npz: `morphologies` (12, 2) int32, `features` (12, 8192) uint32, configuration i
as the probe's select_configuration() decodes it) do not come from the code under test.  They were recorded once from the decision tree this
header replaced, launch_cycle_feat of shc_cycle_inst.hip at commit f5ec9e4: a scratch copy of that file in which `#include "shc_cycle_kernel.hpp"`
became `#include "shc_cycle_launch.hpp"` and the body of launch_cycle<L, NJ, F> became `g_recorded = F;`, with an extern "C" loop appended that
builds the CycleParams / CycleLaunch of configuration i exactly as select_configuration() does, presets g_recorded to 0xFFFFFFFF, calls
shc_launch_loop_L_NJ and stores g_recorded; compiled for the host once per morphology (-DSHC_INST_L -DSHC_INST_NJ -DSHC_INST_PART=1), the twelve
rows stacked in the order of SHC_FOR_EACH_MORPHOLOGY and saved with numpy.savez_compressed.  The old tree resolved every configuration (no
0xFFFFFFFF in the table: asserted below)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = np.load(os.path.join(HERE, "golden", "cycle_select_golden.npz"))
GOLDEN_MORPHOLOGIES = [tuple(int(v) for v in row) for row in GOLDEN["morphologies"]]

# Feature words a KernelTable may list although no configuration of the enumeration selects them: {(legs, joints, word): why it is kept}.
KEPT_UNSELECTED = {}


def header_morphologies():
    text = open(os.path.join(ROOT, "syropod_highlevel_controller_amd", "csrc", "shc_cycle_launch.hpp")).read()
    line = re.search(r"^#define SHC_FOR_EACH_MORPHOLOGY\(X\)(.*)$", text, flags=re.M).group(1)
    return [(int(l), int(nj)) for l, nj in re.findall(r"X\((\d+), (\d+)\)", line)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from syropod_highlevel_controller_amd import engine
    so = engine.compile_with_product_flags(os.path.join(HERE, "cycle_select_probe.hip"), os.path.join(str(tmp_path_factory.mktemp("cycle_select")), "libcycle_select_probe.so"))
    P = C.CDLL(so)
    up = C.POINTER(C.c_uint32)
    P.shc_select_probe_enumerate.argtypes = [C.c_int, C.c_int, up]
    P.shc_select_probe_table.argtypes = [C.c_int, C.c_int, up, C.c_int]
    P.shc_select_probe_forms.argtypes = [C.c_uint32]
    P.shc_select_probe_forms.restype = C.c_uint32
    return P


def selected(P, legs, joints):
    out = np.zeros(P.shc_select_probe_configurations(), dtype=np.uint32)
    assert P.shc_select_probe_enumerate(legs, joints, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0, (legs, joints)
    return out


def table(P, legs, joints):
    out = np.zeros(64, dtype=np.uint32)
    n = P.shc_select_probe_table(legs, joints, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out))
    assert 0 < n <= len(out), (legs, joints, n)
    return [int(v) for v in out[:n]]


def test_morphology_lists_agree():
    """engine.MORPHOLOGIES (what build_library compiles), SHC_FOR_EACH_MORPHOLOGY (what the host side dispatches over) and the recorded table"""
    from syropod_highlevel_controller_amd import engine
    assert [tuple(m) for m in engine.MORPHOLOGIES] == header_morphologies()
    assert GOLDEN_MORPHOLOGIES == header_morphologies()
    assert len(GOLDEN_MORPHOLOGIES) == 12 and GOLDEN["features"].shape == (12, 8192) and GOLDEN["features"].dtype == np.uint32
    assert not (GOLDEN["features"] == 0xFFFFFFFF).any(), "a configuration the old decision tree never resolved"


@pytest.mark.parametrize("legs,joints", GOLDEN_MORPHOLOGIES)
def test_selection_equals_the_recorded_decision_tree(probe, legs, joints):
    want = GOLDEN["features"][GOLDEN_MORPHOLOGIES.index((legs, joints))]
    got = selected(probe, legs, joints)
    assert got.shape == want.shape == (8192,)
    differ = np.flatnonzero(got != want)
    assert differ.size == 0, f"{legs} x {joints}: {differ.size} configurations select another kernel, the first: " + ", ".join(
        f"{i:#06x}: {int(got[i]):#010x} (recorded {int(want[i]):#010x})" for i in differ[:8])


@pytest.mark.parametrize("legs,joints", GOLDEN_MORPHOLOGIES)
def test_selection_and_kernel_table_cover_each_other(probe, legs, joints):
    listed = table(probe, legs, joints)
    assert len(set(listed)) == len(listed), "a feature word is listed twice"
    chosen = set(int(v) for v in selected(probe, legs, joints))
    assert chosen <= set(listed), f"selected without a kernel: {sorted(hex(f) for f in chosen - set(listed))}"
    idle = set(listed) - chosen - {f for (l, nj, f) in KEPT_UNSELECTED if (l, nj) == (legs, joints)}
    assert not idle, f"kernels no configuration selects: {sorted(hex(f) for f in idle)}"


def test_kernel_counts(probe):
    """nothing added to the library, nothing dropped: 15 feature words for each BASELINE morphology, 8 for every other ("Kernel specialisation")"""
    assert {m: len(table(probe, *m)) for m in GOLDEN_MORPHOLOGIES} == {m: 15 if m in ((6, 3), (8, 5)) else 8 for m in GOLDEN_MORPHOLOGIES}


def test_form_predicates(probe):
    """the forms of the feature words the headline configurations run on (default build: no SHC_GENERIC_LOOP_FORMS)"""
    DYN, ROT, ROUGH, MLEGS = 1 << 31, 1 << 30, 1 << 29, 1 << 27
    C2, C3 = 0x41, 0x59
    RES, BATCH, TWO, HALF = 1, 2, 4, 8
    forms = probe.shc_select_probe_forms
    assert forms(C2) == forms(C3) == forms(C3 | 0x20) == RES | BATCH | TWO
    assert forms(C2 | ROT) == forms(C3 | ROT) == RES | BATCH | HALF
    assert forms(C2 | ROUGH) == RES | BATCH
    assert forms(DYN) == RES | TWO
    assert forms(DYN | ROT) == forms(DYN | ROUGH) == 0
    assert forms(DYN | MLEGS) == forms(DYN | ROT | MLEGS) == 0
