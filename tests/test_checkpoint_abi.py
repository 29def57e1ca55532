"""Device checkpoints, the part that needs no GPU: the exported symbols, the NULL-argument answers and the one classification of every
leg / robot field index (state, input, output, LDS-only) that the restore kernel's plane lists are generated from."""
import ctypes as C

import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG

SYMBOLS = ["shc_engine_checkpoint_create", "shc_engine_checkpoint_update", "shc_checkpoint_destroy", "shc_engine_restore_instances", "shc_checkpoint_bytes"]
STATE, INPUT, OUTPUT, LDS_ONLY = range(4)


def leg_fields(nj):
    """Fields<NJ> (csrc/shc_cycle.hpp) restated: name -> (first index, length), and COUNT."""
    nje = (nj + 1) & ~1
    order = [("Q", nj), ("QD", nj), ("TIP", 3), ("TVEL", 3), ("SORG", 3), ("SVEL", 3), ("TORG", 3), ("DFLT", 3), ("TARG", 3), ("STRD", 3), ("ADM", 2), ("TF", 4),
             ("FORCE_IN", 4), ("EFFORT_IN", nje), ("POSER_TIP", 4), ("MODEL_TIP", 4), ("ADM_DELTA", 4), ("ORG_DIR", 3), ("CUR_DIR", 3), ("TARG_DIR", 4),
             ("DES_TIP", 4), ("DES_DIR", 4), ("SEQ_ORG", 4), ("SEQ_DIR", 4), ("SEQ_Q0", nje), ("STEP_PLANE", 4), ("MEAS_Q", nje)]
    at, out = 0, {}
    for name, k in order:
        out[name] = (at, k)
        at += k
    return out, at


ROBOT_FIELDS = {"VLIN": (0, 2), "VANG": (2, 1), "PLANE": (3, 3), "PNORM": (6, 3), "PLANE_PREV": (9, 3), "PNORM_PREV": (12, 3), "OWPP": (15, 7), "VIN": (22, 2), "WIN": (24, 1),
                "MPOSE": (25, 7), "TVI": (32, 3), "RVI": (35, 3), "ABSE": (38, 3), "VERR": (41, 3), "GYRO": (44, 3), "IMUQ": (47, 4), "APREV": (51, 4), "CPOSE": (55, 7),
                "WPP": (62, 7), "ODOM": (69, 4), "INCL": (73, 2), "TALIGN": (75, 7), "OTALIGN": (82, 7)}
ROBOT_COUNT = 89


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS + ["shc_debug_checkpoint_field_class"]:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.shc_abi_version() == 6


def test_null_arguments_are_refused():
    lib = engine.lib()
    out = C.c_void_p()
    assert lib.shc_engine_checkpoint_create(None, C.byref(out)) == SHC_ERR_INVALID_ARG and not out.value
    assert lib.shc_engine_checkpoint_create(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_checkpoint_update(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_checkpoint_destroy(None) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_restore_instances(None, None, None, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_engine_restore_instances(None, None, None, 1) == SHC_ERR_INVALID_ARG
    assert lib.shc_checkpoint_bytes(None) == 0


@pytest.mark.parametrize("nj", [3, 4, 5])
def test_every_leg_field_has_exactly_one_class_and_the_inputs_are_the_held_inputs(nj):
    cls = engine.lib().shc_debug_checkpoint_field_class
    fields, count = leg_fields(nj)
    got = [cls(nj, 0, f) for f in range(count)]
    assert all(c in (STATE, INPUT, OUTPUT, LDS_ONLY) for c in got), got
    assert cls(nj, 0, count) == -1 and cls(nj, 0, -1) == -1
    inputs = {f for name in ("FORCE_IN", "EFFORT_IN") for f in range(fields[name][0], sum(fields[name]))}
    assert {f for f, c in enumerate(got) if c == INPUT} == inputs
    assert LDS_ONLY not in got
    for name in ("POSER_TIP", "MODEL_TIP", "ADM_DELTA"):
        assert all(got[f] == OUTPUT for f in range(fields[name][0], sum(fields[name]))), name
    for name in ("Q", "QD", "TF", "DES_TIP", "SEQ_Q0", "STEP_PLANE", "MEAS_Q"):   # incl. the tail [DES_TIP, COUNT) of the auxiliary blob
        assert all(got[f] == STATE for f in range(fields[name][0], sum(fields[name]))), name


def test_every_robot_field_has_exactly_one_class_and_the_inputs_are_the_held_inputs():
    cls = engine.lib().shc_debug_checkpoint_field_class
    assert sum(k for _, k in ROBOT_FIELDS.values()) == ROBOT_COUNT
    got = [cls(3, 1, f) for f in range(ROBOT_COUNT)]
    assert all(c in (STATE, INPUT, OUTPUT, LDS_ONLY) for c in got), got
    assert cls(3, 1, ROBOT_COUNT) == -1
    span = lambda names: {f for name in names for f in range(ROBOT_FIELDS[name][0], sum(ROBOT_FIELDS[name]))}
    assert {f for f, c in enumerate(got) if c == INPUT} == span(("VIN", "WIN", "GYRO", "IMUQ"))
    assert {f for f, c in enumerate(got) if c == LDS_ONLY} == span(("WPP",))
    assert {f for f, c in enumerate(got) if c == OUTPUT} == span(("CPOSE", "INCL"))
