"""No GPU: the row layout of the action pass (include/shc_batch.h, "Action pass") - shc_act_width / shc_act_column against
engine.action_columns, which computes the same layout on its own, and every refusal a spec earns without a handle."""
import ctypes as C

import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import ACT_FIELD_NAMES, ACT_FIELDS, act_spec, action_columns

ROBOT = {"linear_xy": 2, "angular": 1, "imu_orientation": 4, "imu_angular_velocity": 3, "pose_translation_velocity": 3, "pose_rotation_velocity": 3}
SYMBOLS = ("shc_act_width", "shc_act_column", "shc_engine_set_actions", "shc_fleet_set_actions_device")


def test_the_symbols_exist():
    L = engine.lib()
    for sym in SYMBOLS:
        assert sym in engine.EXPORTED_SYMBOLS
        getattr(L, sym)
        assert sym in engine.HEADER.functions, f"{sym} is declared once"   # (the reader refuses a second declaration)
    assert ACT_FIELD_NAMES == tuple(ROBOT) + ("tip_force", "joint_effort")          # the order of the enum
    assert [ACT_FIELDS[k] for k in ACT_FIELD_NAMES] == list(range(8))
    assert C.sizeof(engine.ActSpec) == 64 and engine.ActSpec.row_stride.offset == 56   # 13 int32, 4 bytes of alignment, int64
    assert L.shc_abi_version() == 6


SPECS = [
    (ACT_FIELD_NAMES, 6, 3),                                                                       # everything, in declaration order
    (("joint_effort", "angular", "tip_force", "imu_angular_velocity", "linear_xy", "pose_rotation_velocity"), 6, 3),   # not in declaration order, halves of pairs
    (ACT_FIELD_NAMES, 8, 6),                                                                       # the largest row geometry
    (tuple(reversed(ACT_FIELD_NAMES)), 8, 6),
    (("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "tip_force", "joint_effort"), 6, 3),          # the 46 columns of a policy's row
    (("tip_force", "imu_orientation"), 7, 5),
    (("joint_effort",), 1, 1),
    (("imu_orientation",), 6, 3),
]


@pytest.mark.parametrize("fields,legs,dof", SPECS)
def test_width_and_columns_agree_with_action_columns(fields, legs, dof):
    L = engine.lib()
    cols, width = action_columns(fields, legs, dof)
    spec = act_spec(fields, legs, dof)
    assert L.shc_act_width(C.byref(spec)) == width
    # the layout worked out here, from the header's rule alone: fields in the order given, per-leg fields leg-major
    at, seen = 0, []
    for name in fields:
        w = ROBOT.get(name) or (dof if name == "joint_effort" else 3)
        n_legs = 1 if name in ROBOT else legs
        assert cols[name] == slice(at, at + n_legs * w), name
        for leg in range(n_legs):
            for k in range(w):
                c = L.shc_act_column(C.byref(spec), ACT_FIELDS[name], leg, k)
                assert c == at + leg * w + k, (name, leg, k)
                seen.append(c)
        assert L.shc_act_column(C.byref(spec), ACT_FIELDS[name], 0, w) == -1 and L.shc_act_column(C.byref(spec), ACT_FIELDS[name], 0, -1) == -1
        if name in ROBOT:
            assert L.shc_act_column(C.byref(spec), ACT_FIELDS[name], 5, 0) == at      # leg is ignored for robot fields
        else:
            assert L.shc_act_column(C.byref(spec), ACT_FIELDS[name], legs, 0) == -1 and L.shc_act_column(C.byref(spec), ACT_FIELDS[name], -1, 0) == -1
        at += n_legs * w
    assert at == width and seen == list(range(width))                               # every column belongs to exactly one component
    for name in set(ACT_FIELD_NAMES) - set(fields):
        assert L.shc_act_column(C.byref(spec), ACT_FIELDS[name], 0, 0) == -1          # absent
    assert L.shc_act_column(C.byref(spec), 8, 0, 0) == -1 and L.shc_act_column(C.byref(spec), -1, 0, 0) == -1
    # row_stride and dtype do not move a column
    for stride, dtype in ((0, "float64"), (width, "float32"), (width + 11, "float64")):
        assert L.shc_act_width(C.byref(act_spec(fields, legs, dof, dtype, stride))) == width


def test_known_widths():
    assert action_columns(ACT_FIELD_NAMES, 6, 3)[1] == 16 + 18 + 18
    assert action_columns(ACT_FIELD_NAMES, 8, 6)[1] == 16 + 24 + 48
    assert action_columns(SPECS[4][0], 6, 3)[1] == 46


def refused():
    ok = lambda **kw: act_spec(("linear_xy", "tip_force"), 6, 3, **kw)
    out = {}
    s = ok()
    s.n_fields = 0
    out["no field"] = s
    s = ok()
    s.n_fields = 9
    out["9 fields"] = s
    s = ok()
    s.n_fields = -1
    out["a negative field count"] = s
    out["an unknown field"] = act_spec((0, 8), 6, 3)
    out["a negative field"] = act_spec((0, -1), 6, 3)
    out["a repeated field"] = act_spec(("linear_xy", "tip_force", "linear_xy"), 6, 3)
    s = ok()
    s.dtype = 2
    out["an unknown dtype"] = s
    s = ok()
    s.reserved = 1
    out["reserved != 0"] = s
    out["legs above SHC_MAX_LEGS"] = act_spec(("linear_xy", "tip_force"), 9, 3)
    out["dof above SHC_MAX_JOINTS"] = act_spec(("linear_xy", "tip_force"), 6, 7)
    out["no legs"] = act_spec(("linear_xy", "tip_force"), 0, 3)
    out["no joints"] = act_spec(("linear_xy", "tip_force"), 6, 0)
    out["a row stride below the width"] = ok(row_stride=2 + 6 * 3 - 1)
    out["a negative row stride"] = ok(row_stride=-1)
    return out


@pytest.mark.parametrize("case", list(refused()))
def test_spec_level_refusals(case):
    L = engine.lib()
    assert L.shc_act_width(C.byref(act_spec(("linear_xy", "tip_force"), 6, 3, row_stride=2 + 6 * 3))) == 20
    spec = refused()[case]
    assert L.shc_act_width(C.byref(spec)) < 0, case
    assert L.shc_last_error()
    assert L.shc_act_column(C.byref(spec), 0, 0, 0) == -1
    assert L.shc_act_width(None) < 0


def test_action_columns_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        action_columns(("angular", "angular"), 6, 3)
    with pytest.raises(ValueError):
        action_columns(("angular", "velocity"), 6, 3)
    with pytest.raises(ValueError):
        action_columns(("angular",), 9, 3)
