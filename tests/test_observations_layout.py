"""No GPU: the row layout of the observation pass (include/shc_batch.h, "Observation pass") - shc_obs_width / shc_obs_column against
engine.observation_columns, which computes the same layout on its own, and every refusal a spec earns without a handle."""
import ctypes as C

import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import OBS_FIELD_NAMES, OBS_FIELDS, obs_spec, observation_columns

ROBOT = {"body_pose": 7, "desired_velocity": 3, "pose_euler": 3, "odom_to_base_link": 7, "walk_state": 1}
JOINT = ("q", "qd", "joint_effort")
LEG = {"walker_tip": 3, "target_tip": 3, "poser_tip": 3, "model_tip": 3, "tip_force": 3, "admittance_delta": 3, "virtual_stiffness": 1,
       "stance_progress": 1, "swing_progress": 1, "time_to_swing_end": 1, "step_state": 1}


def test_the_symbols_exist():
    L = engine.lib()
    for sym in ("shc_obs_width", "shc_obs_column", "shc_engine_get_observations", "shc_fleet_get_observations_device"):
        assert sym in engine.EXPORTED_SYMBOLS
        getattr(L, sym)
    assert len(OBS_FIELD_NAMES) == 19 and set(ROBOT) | set(JOINT) | set(LEG) == set(OBS_FIELD_NAMES)
    assert C.sizeof(engine.ObsSpec) == 168   # 37 int32, 4 bytes of alignment, int64, double
    assert OBS_FIELDS["q"] == 0 and OBS_FIELDS["body_pose"] == 14 and OBS_FIELDS["walk_state"] == 18


SPECS = [
    (OBS_FIELD_NAMES, 6, 3),                                                                      # everything, in declaration order
    (("q", "qd", "model_tip", "stance_progress", "swing_progress", "body_pose", "desired_velocity"), 6, 3),   # the learner-sized selection
    (("walk_state", "tip_force", "body_pose", "qd", "step_state", "pose_euler", "q"), 6, 3),      # leg and robot fields mixed, not in declaration order
    (("swing_progress", "joint_effort", "odom_to_base_link"), 8, 6),                              # the largest row geometry
    (("model_tip", "q", "virtual_stiffness"), 7, 5),                                              # legs / dof larger than a 4 x 4 robot needs
    (tuple(reversed(OBS_FIELD_NAMES)), 8, 5),
    (("time_to_swing_end",), 1, 1),
]


@pytest.mark.parametrize("fields,legs,dof", SPECS)
def test_width_and_columns_agree_with_observation_columns(fields, legs, dof):
    L = engine.lib()
    cols, width = observation_columns(fields, legs, dof)
    spec = obs_spec(fields, legs, dof)
    assert L.shc_obs_width(C.byref(spec)) == width
    # the layout worked out here, from the header's rule alone: fields in the order given, per-leg fields leg-major
    at, seen = 0, []
    for name in fields:
        w = ROBOT.get(name) or (dof if name in JOINT else LEG[name])
        n_legs = 1 if name in ROBOT else legs
        assert cols[name] == slice(at, at + n_legs * w), name
        for leg in range(n_legs):
            for k in range(w):
                c = L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], leg, k)
                assert c == at + leg * w + k, (name, leg, k)
                seen.append(c)
        assert L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], 0, w) == -1 and L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], 0, -1) == -1
        if name in ROBOT:
            assert L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], 5, 0) == at      # leg is ignored for robot fields
        else:
            assert L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], legs, 0) == -1
        at += n_legs * w
    assert at == width and seen == list(range(width))                               # every column belongs to exactly one component
    for name in set(OBS_FIELD_NAMES) - set(fields):
        assert L.shc_obs_column(C.byref(spec), OBS_FIELDS[name], 0, 0) == -1          # absent
    assert L.shc_obs_column(C.byref(spec), 19, 0, 0) == -1 and L.shc_obs_column(C.byref(spec), -1, 0, 0) == -1
    # row_stride and dtype do not move a column
    for stride, dtype in ((0, "float64"), (width, "float32"), (width + 11, "float64")):
        assert L.shc_obs_width(C.byref(obs_spec(fields, legs, dof, dtype, stride))) == width


def refused():
    ok = lambda **kw: obs_spec(("q", "body_pose"), 6, 3, **kw)
    out = {}
    s = ok()
    s.n_fields = 0
    out["no field"] = s
    s = ok()
    s.n_fields = 33
    out["33 fields"] = s
    s = ok()
    s.n_fields = -1
    out["a negative field count"] = s
    out["an unknown field"] = obs_spec((0, 19), 6, 3)
    out["a negative field"] = obs_spec((0, -1), 6, 3)
    out["a repeated field"] = obs_spec(("q", "body_pose", "q"), 6, 3)
    s = ok()
    s.dtype = 2
    out["an unknown dtype"] = s
    s = ok()
    s.reserved = 1
    out["reserved != 0"] = s
    out["legs above SHC_MAX_LEGS"] = obs_spec(("q", "body_pose"), 9, 3)
    out["dof above SHC_MAX_JOINTS"] = obs_spec(("q", "body_pose"), 6, 7)
    out["no legs"] = obs_spec(("q", "body_pose"), 0, 3)
    out["no joints"] = obs_spec(("q", "body_pose"), 6, 0)
    out["a row stride below the width"] = ok(row_stride=6 * 3 + 7 - 1)
    out["a negative row stride"] = ok(row_stride=-1)
    return out


@pytest.mark.parametrize("case", list(refused()))
def test_spec_level_refusals(case):
    L = engine.lib()
    assert L.shc_obs_width(C.byref(obs_spec(("q", "body_pose"), 6, 3, row_stride=6 * 3 + 7))) == 25
    spec = refused()[case]
    assert L.shc_obs_width(C.byref(spec)) < 0, case
    assert L.shc_last_error()
    assert L.shc_obs_column(C.byref(spec), 0, 0, 0) == -1
    assert L.shc_obs_width(None) < 0


def test_observation_columns_refuses_what_the_library_refuses():
    with pytest.raises(ValueError):
        observation_columns(("q", "q"), 6, 3)
    with pytest.raises(ValueError):
        observation_columns(("q", "velocity"), 6, 3)
    with pytest.raises(ValueError):
        observation_columns(("q",), 9, 3)
