"""No GPU: the row layout of the foothold pass (include/shc_batch.h, "Foothold pass") - shc_foothold_width / shc_foothold_column against
engine.foothold_columns, which computes the same layout on its own, and every refusal a spec earns without a handle."""
import ctypes as C

import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import FH_FIELD_NAMES, FH_FIELDS, foothold_columns, foothold_spec

WIDTH = {"position": 3, "rotation": 4, "transform": 7, "swing_clearance": 1, "frame_is_odom_ideal": 1, "defined": 1}
SYMBOLS = ("shc_foothold_width", "shc_foothold_column", "shc_engine_set_footholds", "shc_engine_get_footholds", "shc_fleet_set_footholds_device",
           "shc_fleet_get_footholds_device")
PERMUTED = ("defined", "transform", "position", "frame_is_odom_ideal", "rotation", "swing_clearance")


def test_the_symbols_exist():
    L = engine.lib()
    for sym in SYMBOLS:
        assert sym in engine.EXPORTED_SYMBOLS
        getattr(L, sym)
        assert sym in engine.HEADER.functions, f"{sym} is declared once"   # (the reader refuses a second declaration)
    assert FH_FIELD_NAMES == tuple(WIDTH)                                            # the order of the enum
    assert [FH_FIELDS[k] for k in FH_FIELD_NAMES] == list(range(6))
    assert C.sizeof(engine.FootholdSpec) == 64 and engine.FootholdSpec.row_stride.offset == 48 and engine.FootholdSpec.pad.offset == 56
    assert L.shc_abi_version() == 6


SPECS = [((name,), legs) for name in FH_FIELD_NAMES for legs in (3, 6, 8)] + [(FH_FIELD_NAMES, legs) for legs in (3, 6, 8)] + \
        [(PERMUTED, legs) for legs in (3, 6, 8)] + [(("transform", "defined"), 6), (("position", "defined"), 1)]


@pytest.mark.parametrize("fields,legs", SPECS)
def test_width_and_columns_agree_with_foothold_columns(fields, legs):
    L = engine.lib()
    cols, width = foothold_columns(fields, legs)
    spec = foothold_spec(fields, legs)
    assert L.shc_foothold_width(C.byref(spec)) == width == legs * sum(WIDTH[f] for f in fields)
    # the layout worked out here, from the header's rule alone: fields in the order given, every field per leg, leg-major
    at, seen = 0, []
    for name in fields:
        w = WIDTH[name]
        assert cols[name] == slice(at, at + legs * w), name
        for leg in range(legs):
            for k in range(w):
                c = L.shc_foothold_column(C.byref(spec), FH_FIELDS[name], leg, k)
                assert c == at + leg * w + k, (name, leg, k)
                seen.append(c)
        col = lambda leg, k: L.shc_foothold_column(C.byref(spec), FH_FIELDS[name], leg, k)
        assert col(0, w) == -1 and col(0, -1) == -1 and col(legs, 0) == -1 and col(-1, 0) == -1
        at += legs * w
    assert at == width and seen == list(range(width))                               # every column belongs to exactly one component
    for name in set(FH_FIELD_NAMES) - set(fields):
        assert L.shc_foothold_column(C.byref(spec), FH_FIELDS[name], 0, 0) == -1      # absent
    assert L.shc_foothold_column(C.byref(spec), 6, 0, 0) == -1 and L.shc_foothold_column(C.byref(spec), -1, 0, 0) == -1
    # row_stride, dtype, record, mode and pad do not move a column
    for stride, dtype, which, mode in ((0, "float64", 1, "request"), (width, "float32", 2, "refresh_transform"), (width + 11, "float64", 0, "request")):
        assert L.shc_foothold_width(C.byref(foothold_spec(fields, legs, dtype, which, mode, stride, pad=-7.0))) == width


def test_known_widths():
    assert foothold_columns(FH_FIELD_NAMES, 6)[1] == 6 * 17
    assert foothold_columns(FH_FIELD_NAMES, 8)[1] == 8 * 17                          # the largest row
    assert foothold_columns(("position",), 6)[1] == 18


GOOD = ("position", "defined")


def refused():
    ok = lambda **kw: foothold_spec(GOOD, 6, **kw)
    out = {}
    s = ok()
    s.n_fields = 0
    out["no field"] = s
    s = ok()
    s.n_fields = 7
    out["7 fields"] = s
    s = ok()
    s.n_fields = -1
    out["a negative field count"] = s
    out["an unknown field"] = foothold_spec((0, 6), 6)
    out["a negative field"] = foothold_spec((0, -1), 6)
    out["a repeated field"] = foothold_spec(("position", "defined", "position"), 6)
    s = ok()
    s.dtype = 2
    out["an unknown dtype"] = s
    out["an unknown record"] = ok(which=3)
    out["a negative record"] = ok(which=-1)
    out["an unknown mode"] = ok(mode=2)
    s = ok()
    s.reserved = 1
    out["reserved != 0"] = s
    out["legs above SHC_MAX_LEGS"] = foothold_spec(GOOD, 9)
    out["no legs"] = foothold_spec(GOOD, 0)
    out["a row stride below the width"] = ok(row_stride=6 * 4 - 1)
    out["a negative row stride"] = ok(row_stride=-1)
    return out


@pytest.mark.parametrize("case", list(refused()))
def test_spec_level_refusals(case):
    L = engine.lib()
    assert L.shc_foothold_width(C.byref(foothold_spec(GOOD, 6, row_stride=6 * 4))) == 24
    spec = refused()[case]
    assert L.shc_foothold_width(C.byref(spec)) < 0, case
    assert L.shc_last_error()
    assert L.shc_foothold_column(C.byref(spec), 0, 0, 0) == -1
    assert L.shc_foothold_width(None) < 0


def test_foothold_columns_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        foothold_columns(("position", "position"), 6)
    with pytest.raises(ValueError):
        foothold_columns(("position", "pose"), 6)
    with pytest.raises(ValueError):
        foothold_columns(("position",), 9)
