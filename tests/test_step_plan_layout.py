"""No GPU: the row layout of the step plan pass (include/shc_step_plan.h, which include/shc_batch.h includes) - shc_plan_width / shc_plan_column against
engine.plan_columns, which computes the same layout on its own, against the header's rule restated here, and every refusal a spec earns without a
handle."""
import ctypes as C
import os
import subprocess

import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import PLAN_FIELD_NAMES, PLAN_FIELDS, SHC_ERR_INVALID_ARG, plan_columns, plan_spec

ROBOT = {"walk_plane": 3, "walk_plane_normal": 3}
LEG = {"swing_1_nodes": 15, "swing_2_nodes": 15, "stance_nodes": 15, "default_tip": 3, "target_tip": 3, "stride_vector": 3, "swing_clearance": 3,
       "iteration": 1, "iterations": 1}


def test_the_symbols_exist():
    L = engine.lib()
    assert engine.PLAN_SYMBOLS == ["shc_plan_width", "shc_plan_column", "shc_engine_get_step_plan", "shc_fleet_get_step_plan_device"]
    for sym in engine.PLAN_SYMBOLS:
        assert getattr(L, sym).argtypes is not None
    assert L.shc_plan_width.restype is C.c_int64 and L.shc_engine_get_step_plan.argtypes == [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    assert len(PLAN_FIELD_NAMES) == 12 and set(ROBOT) | set(LEG) | {"path"} == set(PLAN_FIELD_NAMES)
    assert C.sizeof(engine.PlanSpec) == 88   # 17 int32, 4 bytes of alignment, int64, double
    assert PLAN_FIELDS["swing_1_nodes"] == 0 and PLAN_FIELDS["path"] == 9 and PLAN_FIELDS["walk_plane"] == 10 and engine.PLAN_MAX_HORIZON == 16
    assert L.shc_abi_version() == 6        # the pass adds calls and changes none


SPECS = [((name,), legs, h) for name in PLAN_FIELD_NAMES for legs in (3, 6, 8) for h in (1, 16)]
SPECS += [(PLAN_FIELD_NAMES, legs, h) for legs in (3, 6, 8) for h in (1, 16)]
SPECS += [(tuple(reversed(PLAN_FIELD_NAMES)), 8, 16), (("walk_plane", "path", "iteration", "swing_2_nodes", "stride_vector"), 6, 12),
          (("stance_nodes", "swing_clearance"), 6, 0), (("default_tip",), 1, 0)]


@pytest.mark.parametrize("fields,legs,horizon", SPECS)
def test_width_and_columns_agree_with_plan_columns(fields, legs, horizon):
    L = engine.lib()
    cols, width = plan_columns(fields, legs, horizon)
    spec = plan_spec(fields, legs, horizon)
    assert L.shc_plan_width(C.byref(spec)) == width
    # the layout worked out here, from the header's rule alone: fields in the order given, per-leg fields leg-major
    at, seen = 0, []
    for name in fields:
        w = ROBOT.get(name) or (3 * horizon if name == "path" else LEG[name])
        n_legs = 1 if name in ROBOT else legs
        assert cols[name] == slice(at, at + n_legs * w), name
        for leg in range(n_legs):
            for k in range(w):
                c = L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], leg, k)
                assert c == at + leg * w + k, (name, leg, k)
                seen.append(c)
        assert L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], 0, w) == -1 and L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], 0, -1) == -1
        if name in ROBOT:
            assert L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], 5, 0) == at      # leg is ignored for robot fields
        else:
            assert L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], legs, 0) == -1
        at += n_legs * w
    assert at == width and seen == list(range(width))                                 # every column belongs to exactly one component
    for name in set(PLAN_FIELD_NAMES) - set(fields):
        assert L.shc_plan_column(C.byref(spec), PLAN_FIELDS[name], 0, 0) == -1          # absent
    assert L.shc_plan_column(C.byref(spec), 12, 0, 0) == -1 and L.shc_plan_column(C.byref(spec), -1, 0, 0) == -1
    # row_stride, dtype and pad do not move a column; without SHC_PLAN_PATH the horizon does not either
    for stride, dtype in ((0, "float64"), (width, "float32"), (width + 11, "float64")):
        assert L.shc_plan_width(C.byref(plan_spec(fields, legs, horizon, dtype, stride, pad=-7.0))) == width
    if "path" not in fields:
        assert L.shc_plan_width(C.byref(plan_spec(fields, legs, 16))) == L.shc_plan_width(C.byref(plan_spec(fields, legs, 0))) == width


def test_the_path_is_sample_major():
    L = engine.lib()
    spec = plan_spec(("iteration", "path"), 6, 5)
    assert L.shc_plan_width(C.byref(spec)) == 6 + 6 * 15
    for leg in range(6):
        for h in range(1, 6):
            for k in range(3):
                assert L.shc_plan_column(C.byref(spec), PLAN_FIELDS["path"], leg, 3 * (h - 1) + k) == 6 + leg * 15 + 3 * (h - 1) + k
    spec = plan_spec(("swing_1_nodes",), 6)
    assert L.shc_plan_column(C.byref(spec), 0, 2, 3 * 4 + 1) == 2 * 15 + 13            # node 4, component y of leg 2


def refused():
    ok = lambda **kw: plan_spec(("swing_1_nodes", "walk_plane"), 6, **kw)
    out = {}
    for count, what in ((0, "no field"), (13, "13 fields"), (-1, "a negative field count")):
        s = ok()
        s.n_fields = count
        out[what] = s
    out["an unknown field"] = plan_spec((0, 12), 6)
    out["a negative field"] = plan_spec((0, -1), 6)
    out["a repeated field"] = plan_spec(("stance_nodes", "walk_plane", "stance_nodes"), 6)
    s = ok()
    s.dtype = 2
    out["an unknown dtype"] = s
    s = ok()
    s.reserved = 1
    out["reserved != 0"] = s
    out["legs above SHC_MAX_LEGS"] = plan_spec(("swing_1_nodes", "walk_plane"), 9)
    out["no legs"] = plan_spec(("swing_1_nodes", "walk_plane"), 0)
    out["a row stride below the width"] = ok(row_stride=6 * 15 + 3 - 1)
    out["a negative row stride"] = ok(row_stride=-1)
    out["a horizon of 17"] = ok(horizon=17)
    out["a horizon of 17 with the path"] = plan_spec(("path",), 6, 17)
    out["a negative horizon"] = ok(horizon=-1)
    out["a horizon of 0 with the path named"] = plan_spec(("swing_1_nodes", "path"), 6, 0)
    return out


@pytest.mark.parametrize("case", list(refused()))
def test_spec_level_refusals(case):
    L = engine.lib()
    assert L.shc_plan_width(C.byref(plan_spec(("swing_1_nodes", "walk_plane"), 6, 16, row_stride=6 * 15 + 3))) == 93   # the bounds themselves pass
    assert L.shc_plan_width(C.byref(plan_spec(("path",), 8, 16))) == 8 * 48 and L.shc_plan_width(C.byref(plan_spec(("path",), 8, 1))) == 24
    spec = refused()[case]
    assert L.shc_plan_width(C.byref(spec)) < 0, case
    assert L.shc_last_error()
    assert L.shc_plan_column(C.byref(spec), 0, 0, 0) == -1
    assert L.shc_plan_width(None) < 0 and L.shc_plan_column(None, 0, 0, 0) == -1


def test_calls_without_a_handle_are_refused():
    L = engine.lib()
    spec, buf = plan_spec(("stride_vector",), 6), (C.c_double * 64)()
    assert L.shc_engine_get_step_plan(None, 0, 1, C.byref(spec), buf, 0) == SHC_ERR_INVALID_ARG
    assert L.shc_fleet_get_step_plan_device(None, C.byref(spec), buf) == SHC_ERR_INVALID_ARG


def test_plan_columns_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        plan_columns(("path", "path"), 6, 4)
    with pytest.raises(ValueError):
        plan_columns(("path", "nodes"), 6, 4)
    with pytest.raises(ValueError):
        plan_columns(("path",), 9, 4)
    with pytest.raises(ValueError):
        plan_columns(("path",), 6, 0)
    with pytest.raises(ValueError):
        plan_columns(("path",), 6, 17)


def test_the_header_and_its_mirror(tmp_path):
    """include/shc_step_plan.h as tests/test_abi_header.py holds include/shc_batch.h: the reader finds its four prototypes and its struct, the
    field names are the enum's own order, and the host C compiler judges the ctypes mirror - through shc_batch.h alone and with this header first."""
    from syropod_highlevel_controller_amd import cheader
    from test_abi_header import _host_c_compiler
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    header = cheader.read(os.path.join(inc, "shc_step_plan.h"))
    assert list(header.structs) == list(engine.PLAN_STRUCT_MIRRORS) == ["shc_plan_spec"] and len(header.functions) == 4
    assert header.enum_of("SHC_PLAN_FIELD_COUNT") == tuple("SHC_PLAN_" + name.upper() for name in PLAN_FIELD_NAMES) + ("SHC_PLAN_FIELD_COUNT",)
    assert not set(header.functions) & set(engine.EXPORTED_SYMBOLS) and not set(header.constants) & set(cheader.read(os.path.join(inc, "shc_batch.h")).constants)
    fields, mirror = header.structs["shc_plan_spec"], engine.PlanSpec
    assert [f for f, _ in mirror._fields_] == [f for _, f, _ in fields]
    asserts = [f'_Static_assert(sizeof(shc_plan_spec) == {C.sizeof(mirror)}, "sizeof");']
    for f, typ in mirror._fields_:
        asserts.append(f'_Static_assert(offsetof(shc_plan_spec, {f}) == {getattr(mirror, f).offset}, "offsetof {f}");')
        asserts.append(f'_Static_assert(sizeof(((shc_plan_spec *)0)->{f}) == {C.sizeof(typ)}, "sizeof {f}");')
    for k, first in enumerate(("shc_batch.h", "shc_step_plan.h")):
        src = tmp_path / f"plan_mirror_{k}.c"
        src.write_text("\n".join(["#include <stddef.h>", f'#include "{first}"'] + asserts + ["int (*use)(shc_engine *, int64_t, int64_t, const shc_plan_spec *, void *, int) = shc_engine_get_step_plan;"]) + "\n")
        cmd = _host_c_compiler() + ["-std=c11", "-I", inc, "-c", "-o", str(tmp_path / f"plan_mirror_{k}.o"), str(src)]
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, f"{' '.join(cmd)}\n{built.stderr[-4000:]}"
