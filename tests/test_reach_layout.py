"""No GPU: the reach probe (include/shc_batch.h, "Reach probe") as far as it goes without a device - the exported symbols, the ABI version, the
size of shc_reach_spec, the layout of a candidate's block (shc_reach_width / shc_reach_column against the header's rule restated here and
against engine.reach_columns), every refusal a spec earns without a handle, the NULL-handle answers and the Python layer's own refusal of
host arrays and other element types (no call here reaches a device)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, engine
from syropod_highlevel_controller_amd.engine import REACH_FIELD_NAMES, REACH_FIELDS, SHC_ERR_INVALID_ARG, BatchEngine, ReachSpec, reach_columns, reach_spec
from syropod_highlevel_controller_amd.fleet import MixedFleet

SYMBOLS = ("shc_reach_width", "shc_reach_column", "shc_engine_probe_reach", "shc_fleet_probe_reach_device")


def width_of(name, dof):
    return {"fraction": 1, "limit_proximity": 1, "tip": 3, "q": dof}[name]


def test_symbols_are_exported_declared_once_and_listed():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        assert s in engine.HEADER.functions, f"{s} is declared once"   # (the reader refuses a second declaration)
        getattr(lib, s)
    assert lib.shc_abi_version() == 6
    assert REACH_FIELD_NAMES == ("fraction", "limit_proximity", "tip", "q")           # the order of the enum
    assert [REACH_FIELDS[k] for k in REACH_FIELD_NAMES] == list(range(4))
    for name, value in zip(("SHC_REACH_FRACTION", "SHC_REACH_LIMIT_PROXIMITY", "SHC_REACH_TIP", "SHC_REACH_Q", "SHC_REACH_FIELD_COUNT"), range(5)):
        assert engine.HEADER.constants[name] == value, name
    for cls in (BatchEngine, MixedFleet):
        assert callable(cls.probe_reach)


def test_sizeof_the_spec():
    # 11 int32, 4 bytes of alignment, two int64, a double: the library's own static_assert holds the C side to the same numbers
    assert C.sizeof(ReachSpec) == 72
    assert (ReachSpec.dtype.offset, ReachSpec.legs.offset, ReachSpec.dof.offset, ReachSpec.candidates.offset, ReachSpec.steps.offset,
            ReachSpec.reserved.offset) == (20, 24, 28, 32, 36, 40)
    assert (ReachSpec.row_stride.offset, ReachSpec.target_row_stride.offset, ReachSpec.pad.offset) == (48, 56, 64)
    # ... and the library reads the members where the mirror puts them: a spec that is valid but for one member is refused for that member
    lib = engine.lib()
    for member, value, word in (("candidates", 65, b"candidates"), ("steps", 4097, b"steps"), ("reserved", 1, b"reserved"), ("dtype", 2, b"dtype"),
                                ("target_row_stride", 17, b"target_row_stride"), ("row_stride", 11, b"row_stride"), ("legs", 9, b"legs"), ("dof", 7, b"dof")):
        spec = reach_spec(("fraction", "tip"), 6, 3, 2, 16)
        assert lib.shc_reach_width(C.byref(spec)) == 6 * 4
        setattr(spec, member, value)
        assert lib.shc_reach_width(C.byref(spec)) < 0, member
        assert word in lib.shc_last_error(), (member, lib.shc_last_error())


SELECTIONS = [sel for k in range(1, 5) for sel in itertools.permutations(REACH_FIELD_NAMES, k)]   # every subset in every order: 64
assert len(SELECTIONS) == 64


@pytest.mark.parametrize("legs,dof", [(6, 3), (8, 5), (4, 4)])
def test_width_and_columns_follow_the_row_rule(legs, dof):
    lib = engine.lib()
    for fields in SELECTIONS:
        spec = reach_spec(fields, legs, dof, 3, 16)
        cols, width = reach_columns(fields, legs, dof)
        assert lib.shc_reach_width(C.byref(spec)) == width == legs * sum(width_of(f, dof) for f in fields)
        # the rule of the header restated: fields in the order given, every field per leg, leg-major
        at, seen = 0, []
        for name in fields:
            w = width_of(name, dof)
            assert cols[name] == slice(at, at + legs * w), (fields, name)
            col = lambda leg, k: lib.shc_reach_column(C.byref(spec), REACH_FIELDS[name], leg, k)
            for leg in range(legs):
                for k in range(w):
                    assert col(leg, k) == at + leg * w + k, (fields, name, leg, k)
                    seen.append(at + leg * w + k)
            assert col(0, w) == -1 and col(0, -1) == -1 and col(legs, 0) == -1 and col(-1, 0) == -1
            at += legs * w
        assert at == width and seen == list(range(width))                             # every column belongs to exactly one component
        for name in set(REACH_FIELD_NAMES) - set(fields):
            assert lib.shc_reach_column(C.byref(spec), REACH_FIELDS[name], 0, 0) == -1    # absent
        assert lib.shc_reach_column(C.byref(spec), 4, 0, 0) == -1 and lib.shc_reach_column(C.byref(spec), -1, 0, 0) == -1
    # candidates, steps, strides, dtype and pad do not move a column: the width is that of ONE candidate's block
    fields = ("tip", "fraction", "q")
    width = legs * (4 + dof)
    for cands, steps, stride, tstride, dtype in ((1, 1, 0, 0, "float64"), (64, 4096, 64 * width, 64 * legs * 3, "float32"), (5, 7, 5 * width + 3, 5 * legs * 3 + 1, "float64")):
        assert lib.shc_reach_width(C.byref(reach_spec(fields, legs, dof, cands, steps, dtype, stride, tstride, pad=-7.0))) == width


def test_known_widths():
    assert reach_columns(("fraction", "limit_proximity"), 6, 3)[1] == 12              # the default selection of probe_reach for a hexapod
    assert reach_columns(("fraction", "limit_proximity", "tip"), 6, 3)[1] == 30
    assert reach_columns(REACH_FIELD_NAMES, 8, 5)[1] == 80
    assert reach_columns(REACH_FIELD_NAMES, 8, 6)[1] == 88                            # the largest block


GOOD = ("fraction", "q")


def refused():
    ok = lambda **kw: reach_spec(GOOD, 6, 3, **{"candidates": 4, "steps": 16, **kw})
    out = {}
    for what, count in (("no field", 0), ("5 fields", 5), ("a negative field count", -1)):
        s = ok()
        s.n_fields = count
        out[what] = s
    out["an unknown field"] = reach_spec((0, 4), 6, 3, 4, 16)
    out["a negative field"] = reach_spec((0, -1), 6, 3, 4, 16)
    out["a repeated field"] = reach_spec(("fraction", "q", "fraction"), 6, 3, 4, 16)
    for what, dtype in (("an unknown dtype", 2), ("a negative dtype", -1)):
        s = ok()
        s.dtype = dtype
        out[what] = s
    s = ok()
    s.reserved = 1
    out["reserved != 0"] = s
    out["legs above SHC_MAX_LEGS"] = reach_spec(GOOD, 9, 3, 4, 16)
    out["no legs"] = reach_spec(GOOD, 0, 3, 4, 16)
    out["dof above SHC_MAX_JOINTS"] = reach_spec(GOOD, 6, 7, 4, 16)
    out["no joints"] = reach_spec(GOOD, 6, 0, 4, 16)
    out["no candidate"] = ok(candidates=0)
    out["a negative candidate count"] = ok(candidates=-1)
    out["65 candidates"] = ok(candidates=65)
    out["no step"] = ok(steps=0)
    out["a negative step count"] = ok(steps=-3)
    out["4097 steps"] = ok(steps=4097)
    out["a row stride below a block"] = ok(row_stride=6 * 4 - 1)
    out["a row stride below candidates x the block"] = ok(row_stride=4 * 6 * 4 - 1)
    out["a negative row stride"] = ok(row_stride=-1)
    out["a target row stride below candidates x legs x 3"] = ok(target_row_stride=4 * 18 - 1)
    out["a negative target row stride"] = ok(target_row_stride=-1)
    return out


@pytest.mark.parametrize("case", list(refused()))
def test_spec_level_refusals(case):
    lib = engine.lib()
    assert lib.shc_reach_width(C.byref(reach_spec(GOOD, 6, 3, 4, 16, row_stride=4 * 24, target_row_stride=4 * 18))) == 24   # the bounds themselves pass
    assert lib.shc_reach_width(C.byref(reach_spec(GOOD, 6, 3, 64, 4096))) == 24
    spec = refused()[case]
    assert lib.shc_reach_width(C.byref(spec)) < 0, case
    assert lib.shc_last_error()
    assert lib.shc_reach_column(C.byref(spec), 0, 0, 0) == -1
    assert lib.shc_reach_width(None) < 0 and lib.shc_reach_column(None, 0, 0, 0) == -1
    # ... and by the calls, before they look at anything else (the handle is refused first: no device is touched)
    buf = (C.c_double * 8)()
    assert lib.shc_engine_probe_reach(None, 0, 1, C.byref(spec), buf, buf) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_probe_reach_device(None, C.byref(spec), buf, buf) == SHC_ERR_INVALID_ARG


def test_reach_columns_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        reach_columns(("tip", "tip"), 6, 3)
    with pytest.raises(ValueError):
        reach_columns(("tip", "reach"), 6, 3)
    with pytest.raises(ValueError):
        reach_columns(("tip",), 9, 3)
    with pytest.raises(ValueError):
        reach_columns(("q",), 6, 7)


def test_null_handles_are_refused_with_a_message():
    lib = engine.lib()
    spec = reach_spec(("fraction", "limit_proximity", "tip"), 6, 3, 8, 16)
    buf = (C.c_double * 8)()   # (never dereferenced: the handle is refused first)
    lib.shc_reach_width(C.byref(spec))
    for call in (lambda: lib.shc_engine_probe_reach(None, 0, 1, C.byref(spec), buf, buf), lambda: lib.shc_engine_probe_reach(None, 0, 0, None, None, None),
                 lambda: lib.shc_fleet_probe_reach_device(None, C.byref(spec), buf, buf), lambda: lib.shc_fleet_probe_reach_device(None, None, None, None)):
        assert call() == SHC_ERR_INVALID_ARG
        assert b"NULL" in lib.shc_last_error()


def handles_without_a_device():
    """A BatchEngine view and a MixedFleet around no handle at all: the refusals below are decided before the library is asked."""
    eng = BatchEngine.view(0, default_hexapod_params("tripod"), 4)
    fleet = MixedFleet.__new__(MixedFleet)
    fleet.L, fleet.h, fleet.n, fleet.max_legs, fleet.max_dof = engine.lib(), None, 4, 8, 5
    return eng, fleet


class DeviceArray:
    """Stands for a device tensor of any element type where there is no device: the calls below are refused before the pointer is used."""

    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (1 << 20, False), "strides": None, "version": 3}


def test_numpy_arrays_and_float16_are_a_type_error():
    for who, legs in zip(handles_without_a_device(), (6, 8)):
        with pytest.raises(TypeError, match="device arrays only"):
            who.probe_reach(np.zeros((4, 2, legs, 3), dtype=np.float32), 16)
        with pytest.raises(TypeError, match="device arrays only"):
            who.probe_reach(DeviceArray((4, 2, legs, 3), "<f4"), 16, out=np.zeros((4, 2, 2 * legs), dtype=np.float32))
        with pytest.raises(TypeError, match="device arrays only"):
            who.probe_reach([[[[0.0] * 3] * legs] * 2] * 4, 16)                          # no device array at all
        with pytest.raises(TypeError, match="float32 or float64"):
            who.probe_reach(DeviceArray((4, 2, legs, 3), "<f2"), 16)                      # float16
        with pytest.raises(TypeError, match="float32 or float64"):
            who.probe_reach(DeviceArray((4, 2, legs, 3), "<f4"), 16, out=DeviceArray((4, 2, 2 * legs), "<f2"))
        with pytest.raises(TypeError, match="element type of targets"):
            who.probe_reach(DeviceArray((4, 2, legs, 3), "<f4"), 16, out=DeviceArray((4, 2, 2 * legs), "<f8"))
        # shapes: a ValueError, again before the library is asked
        with pytest.raises(ValueError):
            who.probe_reach(DeviceArray((4, 2, legs * 3), "<f4"), 16)                     # three dimensions
        with pytest.raises(ValueError):
            who.probe_reach(DeviceArray((4, 2, legs - 1, 3), "<f4"), 16)                  # another row geometry
        with pytest.raises(ValueError):
            who.probe_reach(DeviceArray((3, 2, legs, 3), "<f4"), 16)                      # a robot short
        with pytest.raises(ValueError):
            who.probe_reach(DeviceArray((4, 2, legs, 3), "<f4"), 16, out=DeviceArray((4, 2, 2 * legs + 1), "<f4"))
