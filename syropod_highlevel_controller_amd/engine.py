"""ctypes binding of the C ABI (include/shc_batch.h, libshc_batch.so) — host-side mirror of the per-cycle call
surface of the reference's StateController::loop for a batch of robots.

Plumbing only: numpy arrays (host) or raw device pointers (e.g. ``torch.Tensor.data_ptr()``) go straight to the
C entry points.  There is NO CPU fallback: creating an engine without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os
import time
import subprocess
import sys
from typing import NamedTuple, Optional

import numpy as np

from . import arrays, cheader
from .params import (FEAT_DEFAULT, FRAME_IDS, HEADER, BodyFrames, ExternalTarget, InstanceState, JointParams, LegFrames, LegSnapshot, LegStateMsg,
                     LinkParams, Params, StepCycle, Tables, _shc)

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("SHC_LIB") or os.path.join(_HERE, "libshc_batch.so")
_SRC = os.path.join(_HERE, "csrc")
_INC = os.path.join(os.path.dirname(_HERE), "include")

(SHC_OK, SHC_ERR_INVALID_ARG, SHC_ERR_NO_DEVICE, SHC_ERR_HIP, SHC_ERR_UNSUPPORTED, SHC_ERR_UNSTABLE, SHC_ERR_BUSY,
 SHC_ERR_TIMEOUT) = _shc("OK", "ERR_INVALID_ARG", "ERR_NO_DEVICE", "ERR_HIP", "ERR_UNSUPPORTED", "ERR_UNSTABLE", "ERR_BUSY", "ERR_TIMEOUT")

EXPORTED_SYMBOLS = list(HEADER.functions)  # every prototype of include/shc_batch.h
PLAN_HEADER = cheader.read(os.path.join(_INC, "shc_step_plan.h"))   # the step plan pass: a header of its own, which shc_batch.h includes
PLAN_SYMBOLS = list(PLAN_HEADER.functions)


def _struct_dtype(struct) -> np.dtype:
    """The numpy structured dtype of a ctypes structure of doubles / double arrays: names, offsets and item size follow the structure's own
    field list, so a field added to the C struct's mirror is a field of the arrays too."""
    names, formats, offsets = [], [], []
    for name, typ in struct._fields_:
        shape, base = [], typ
        while base is not C.c_double:   # double, double[k] or double[j][k]
            assert issubclass(base, C.Array), name
            shape.append(base._length_)
            base = base._type_
        names.append(name)
        formats.append((np.float64, tuple(shape)) if shape else np.float64)
        offsets.append(getattr(struct, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": C.sizeof(struct)})


LEG_STATE_MSG_DTYPE = _struct_dtype(LegStateMsg)  # what BatchEngine.leg_state_msgs / MixedFleet.leg_state_msgs return
LEG_FRAMES_DTYPE, BODY_FRAMES_DTYPE = _struct_dtype(LegFrames), _struct_dtype(BodyFrames)  # ... and what frame_transforms returns


# shc_engine_scan_health (include/shc_batch.h): the SHC_HEALTH_* bits of shc_robot_health.flags / shc_health_criteria.select
HEALTH_IK_DEVIATION, HEALTH_POSITION_LIMIT, HEALTH_SPEED_LIMIT, HEALTH_NEAR_LIMIT, HEALTH_TIP_DEVIATION, HEALTH_NONFINITE = _shc(
    "HEALTH_IK_DEVIATION", "HEALTH_POSITION_LIMIT", "HEALTH_SPEED_LIMIT", "HEALTH_NEAR_LIMIT", "HEALTH_TIP_DEVIATION", "HEALTH_NONFINITE")
HEALTH_ALL = HEALTH_IK_DEVIATION | HEALTH_POSITION_LIMIT | HEALTH_SPEED_LIMIT | HEALTH_NEAR_LIMIT | HEALTH_TIP_DEVIATION | HEALTH_NONFINITE


class HealthCriteria(C.Structure):
    """shc_health_criteria: which flags select a robot, and the thresholds of NEAR_LIMIT / TIP_DEVIATION."""
    _fields_ = [("select", C.c_uint32), ("reserved", C.c_uint32), ("near_limit_proximity", C.c_double), ("tip_deviation", C.c_double)]


class RobotHealth(C.Structure):
    """shc_robot_health: 32 bytes, no padding."""
    _fields_ = [("min_limit_proximity", C.c_double), ("max_tip_deviation", C.c_double), ("max_speed_ratio", C.c_double), ("flags", C.c_uint32),
                ("leg_masks", C.c_uint32)]


# what BatchEngine.scan_health / MixedFleet.scan_health return; leg_masks: byte 0 IK deviation, 1 position limit, 2 speed limit, 3 non-finite, bit l = leg l
ROBOT_HEALTH_DTYPE = np.dtype({"names": [k for k, _ in RobotHealth._fields_], "formats": [np.float64, np.float64, np.float64, np.uint32, np.uint32],
                               "offsets": [getattr(RobotHealth, k).offset for k, _ in RobotHealth._fields_], "itemsize": C.sizeof(RobotHealth)})


class CycleInputs(C.Structure):
    """shc_cycle_inputs (include/shc_batch.h): what the callbacks of one loop iteration delivered; NULL = not received."""
    _fields_ = [(k, C.c_void_p) for k in ("linear_xy", "angular", "imu_orientation_wxyz", "imu_angular_velocity", "pose_translation_velocity",
                                           "pose_rotation_velocity", "pose_reset_mode", "tip_force", "joint_effort")] + [("on_device", C.c_int32), ("publish", C.c_int32),
                                                                                                                  ("direct", C.c_int32), ("reserved_", C.c_int32)]


FLEET_INPUTS = ("linear_xy", "angular", "imu_orientation_wxyz", "imu_angular_velocity", "pose_translation_velocity", "pose_rotation_velocity", "tip_force",
                "joint_effort")


class FleetInputs(C.Structure):
    """shc_fleet_inputs: device arrays in the caller's instance order; NULL = that input is held."""
    _fields_ = [(k, C.c_void_p) for k in FLEET_INPUTS]


class FleetOutputs(C.Structure):
    """shc_fleet_outputs: device buffers in the caller's instance order; NULL = not asked for.  criteria is a host pointer."""
    _fields_ = [(k, C.c_void_p) for k in ("q", "qd", "walk_state", "leg_state_msgs", "leg_frames", "body_frames")] + [("frame", C.c_int32), ("reserved", C.c_int32),
                                                                                                                 ("health", C.c_void_p),
                                                                                                                 ("criteria", C.POINTER(HealthCriteria))]


# The row passes (include/shc_batch.h: "Observation pass", "Action pass", "Foothold pass"): SHC_OBS_* / SHC_ACT_* / SHC_FH_* by name, in the order
# of the enums
OBS_FIELD_NAMES = ("q", "qd", "joint_effort", "walker_tip", "target_tip", "poser_tip", "model_tip", "tip_force", "admittance_delta", "virtual_stiffness",
                   "stance_progress", "swing_progress", "time_to_swing_end", "step_state",
                   "body_pose", "desired_velocity", "pose_euler", "odom_to_base_link", "walk_state")
OBS_FIELDS = {name: i for i, name in enumerate(OBS_FIELD_NAMES)}
OBS_MAX_FIELDS, = _shc("OBS_MAX_FIELDS")
OBS_DTYPES = dict(zip(("float64", "float32"), _shc("OBS_F64", "OBS_F32")))
_DTYPE_IDS = {np.dtype(name): value for name, value in OBS_DTYPES.items()}   # (an array's own dtype object: no name to spell out per call)
ACT_FIELD_NAMES = ("linear_xy", "angular", "imu_orientation", "imu_angular_velocity", "pose_translation_velocity", "pose_rotation_velocity", "tip_force",
                   "joint_effort")
ACT_FIELDS = {name: i for i, name in enumerate(ACT_FIELD_NAMES)}
FH_FIELD_NAMES = ("position", "rotation", "transform", "swing_clearance", "frame_is_odom_ideal", "defined")  # every field is per leg
FH_FIELDS = {name: i for i, name in enumerate(FH_FIELD_NAMES)}
FH_MODES = dict(zip(("request", "refresh_transform"), _shc("FH_REQUEST", "FH_REFRESH_TRANSFORM")))
REACH_FIELD_NAMES = ("fraction", "limit_proximity", "tip", "q")  # SHC_REACH_*: every field is per leg
REACH_FIELDS = {name: i for i, name in enumerate(REACH_FIELD_NAMES)}
PLAN_FIELD_NAMES = ("swing_1_nodes", "swing_2_nodes", "stance_nodes", "default_tip", "target_tip", "stride_vector", "swing_clearance", "iteration",
                    "iterations", "path", "walk_plane", "walk_plane_normal")  # SHC_PLAN_*: ten per-leg fields, then two per-robot fields
PLAN_FIELDS = {name: i for i, name in enumerate(PLAN_FIELD_NAMES)}
PLAN_MAX_HORIZON = PLAN_HEADER.constants["SHC_PLAN_MAX_HORIZON"]


class ObsSpec(C.Structure):
    """shc_obs_spec: which fields, in which order, as which element type, for which row geometry."""
    _fields_ = [("n_fields", C.c_int32), ("fields", C.c_int32 * OBS_MAX_FIELDS), ("dtype", C.c_int32), ("legs", C.c_int32), ("dof", C.c_int32),
                ("reserved", C.c_int32), ("row_stride", C.c_int64), ("pad", C.c_double)]


class ActSpec(C.Structure):
    """shc_act_spec: which input groups, in which order, as which element type, for which row geometry."""
    _fields_ = [("n_fields", C.c_int32), ("fields", C.c_int32 * len(ACT_FIELD_NAMES)), ("dtype", C.c_int32), ("legs", C.c_int32), ("dof", C.c_int32),
                ("reserved", C.c_int32), ("row_stride", C.c_int64)]


class FootholdSpec(C.Structure):
    """shc_foothold_spec: which members of the requests, in which order, as which element type, for which row geometry, record and mode."""
    _fields_ = [("n_fields", C.c_int32), ("fields", C.c_int32 * len(FH_FIELD_NAMES)), ("dtype", C.c_int32), ("legs", C.c_int32), ("which", C.c_int32),
                ("mode", C.c_int32), ("reserved", C.c_int32), ("row_stride", C.c_int64), ("pad", C.c_double)]


class ReachSpec(C.Structure):
    """shc_reach_spec: which results, in which order, as which element type, for which row geometry, how many candidates and steps."""
    _fields_ = [("n_fields", C.c_int32), ("fields", C.c_int32 * len(REACH_FIELD_NAMES)), ("dtype", C.c_int32), ("legs", C.c_int32), ("dof", C.c_int32),
                ("candidates", C.c_int32), ("steps", C.c_int32), ("reserved", C.c_int32), ("row_stride", C.c_int64), ("target_row_stride", C.c_int64),
                ("pad", C.c_double)]


class PlanSpec(C.Structure):
    """shc_plan_spec: which members of the steppers' plan, in which order, as which element type, for which row geometry and path horizon."""
    _fields_ = [("n_fields", C.c_int32), ("fields", C.c_int32 * len(PLAN_FIELD_NAMES)), ("dtype", C.c_int32), ("legs", C.c_int32), ("horizon", C.c_int32),
                ("reserved", C.c_int32), ("row_stride", C.c_int64), ("pad", C.c_double)]


# every struct of include/shc_batch.h that has a body, and its ctypes mirror (tests/test_abi_header.py holds each to the header, member by member)
STRUCT_MIRRORS = {
    "shc_joint_params": JointParams, "shc_link_params": LinkParams, "shc_params": Params, "shc_step_cycle": StepCycle, "shc_tables": Tables,
    "shc_cycle_inputs": CycleInputs, "shc_leg_state_msg": LegStateMsg, "shc_leg_frames": LegFrames, "shc_body_frames": BodyFrames,
    "shc_leg_snapshot": LegSnapshot, "shc_instance_state": InstanceState, "shc_external_target": ExternalTarget,
    "shc_health_criteria": HealthCriteria, "shc_robot_health": RobotHealth, "shc_fleet_inputs": FleetInputs, "shc_fleet_outputs": FleetOutputs,
    "shc_obs_spec": ObsSpec, "shc_act_spec": ActSpec, "shc_foothold_spec": FootholdSpec, "shc_reach_spec": ReachSpec,
}
PLAN_STRUCT_MIRRORS = {"shc_plan_spec": PlanSpec}   # ... and of include/shc_step_plan.h (tests/test_step_plan_layout.py holds it to that header)


class _RowPass(NamedTuple):
    """What tells one row pass from another on this side: names in enum order and their enum values, columns of the per-robot fields, columns
    per leg of the per-leg fields, the per-leg fields of ``dof`` columns, the ctypes struct and the library's width / column functions; own:
    members of the struct that no layout depends on but a valid spec needs; scale, unit: the member that stands where ``dof`` stands
    elsewhere, and the columns each count of it is worth."""
    names: tuple
    index: dict
    robot: dict
    leg: dict
    joint: tuple
    struct: type
    width: str
    column: str
    own: tuple = ()
    scale: str = "dof"
    unit: int = 1


_ROW_PASSES = {
    "observation": _RowPass(OBS_FIELD_NAMES, OBS_FIELDS, {"body_pose": 7, "desired_velocity": 3, "pose_euler": 3, "odom_to_base_link": 7, "walk_state": 1},
                            {"walker_tip": 3, "target_tip": 3, "poser_tip": 3, "model_tip": 3, "tip_force": 3, "admittance_delta": 3, "virtual_stiffness": 1,
                             "stance_progress": 1, "swing_progress": 1, "time_to_swing_end": 1, "step_state": 1},
                            ("q", "qd", "joint_effort"), ObsSpec, "shc_obs_width", "shc_obs_column"),
    "action": _RowPass(ACT_FIELD_NAMES, ACT_FIELDS, {"linear_xy": 2, "angular": 1, "imu_orientation": 4, "imu_angular_velocity": 3,
                                                     "pose_translation_velocity": 3, "pose_rotation_velocity": 3},
                       {"tip_force": 3}, ("joint_effort",), ActSpec, "shc_act_width", "shc_act_column"),
    "foothold": _RowPass(FH_FIELD_NAMES, FH_FIELDS, {}, {"position": 3, "rotation": 4, "transform": 7, "swing_clearance": 1, "frame_is_odom_ideal": 1,
                                                         "defined": 1}, (), FootholdSpec, "shc_foothold_width", "shc_foothold_column"),
    "reach": _RowPass(REACH_FIELD_NAMES, REACH_FIELDS, {}, {"fraction": 1, "limit_proximity": 1, "tip": 3}, ("q",), ReachSpec, "shc_reach_width",
                      "shc_reach_column", (("candidates", 1), ("steps", 1))),
    "plan": _RowPass(PLAN_FIELD_NAMES, PLAN_FIELDS, {"walk_plane": 3, "walk_plane_normal": 3},
                     {"swing_1_nodes": 15, "swing_2_nodes": 15, "stance_nodes": 15, "default_tip": 3, "target_tip": 3, "stride_vector": 3,
                      "swing_clearance": 3, "iteration": 1, "iterations": 1}, ("path",), PlanSpec, "shc_plan_width", "shc_plan_column", (), "horizon", 3),
}


def _row_spec(kind: str, fields, dtype, row_stride):
    """The spec struct of a list of field names or enum integers, but for the members of its own that the caller sets (this runs once per call of
    a pass: no more work than the assignments).  Nothing is checked here: the library judges the spec."""
    p = _ROW_PASSES[kind]
    index = p.index
    ids = [index[f] if isinstance(f, str) else int(f) for f in fields]
    st = p.struct()
    st.n_fields = len(ids)
    head = ids[:p.struct.fields.size // 4]
    st.fields[:len(head)] = head
    st.dtype = dtype if isinstance(dtype, int) else _DTYPE_IDS[dtype] if dtype in _DTYPE_IDS else OBS_DTYPES[np.dtype(dtype).name]
    st.row_stride = int(row_stride)
    for member, value in p.own:
        setattr(st, member, value)
    return st


def _row_columns(kind: str, fields, legs: int, dof: int):
    """({name: slice}, width) of a row of the pass for the row geometry (legs, dof): a per-leg field's slice reshapes to (legs, width per leg),
    leg-major.  Computed here and checked against the library's own answer (its width and column functions)."""
    p, legs = _ROW_PASSES[kind], int(legs)
    names = [f if isinstance(f, str) else p.names[int(f)] for f in fields]
    cols, at = {}, 0
    for name in names:
        if name in cols:
            raise ValueError(f"{kind} field {name!r} is named twice")
        if name not in p.names:
            raise ValueError(f"unknown {kind} field {name!r} (one of {', '.join(p.names)})")
        w = p.robot[name] if name in p.robot else legs * (int(dof) * p.unit if name in p.joint else p.leg[name])
        cols[name] = slice(at, at + w)
        at += w
    L, spec = lib(), _row_spec(kind, names, "float32", 0)
    spec.legs = legs
    if p.joint:
        setattr(spec, p.scale, int(dof))
    column = getattr(L, p.column)
    width = int(getattr(L, p.width)(C.byref(spec)))
    if width < 0:
        msg = L.shc_last_error()
        raise ValueError(f"{kind} spec refused: {msg.decode() if msg else ''}")
    for name, sl in cols.items():
        last = (0, sl.stop - sl.start - 1) if name in p.robot else (legs - 1, (sl.stop - sl.start) // legs - 1)
        if width != at or column(C.byref(spec), p.index[name], 0, 0) != sl.start or column(C.byref(spec), p.index[name], *last) != sl.stop - 1:
            raise ShcError(f"{kind}_columns and the library disagree on {name!r}")
    return cols, at


def obs_spec(fields, legs: int, dof: int, dtype="float32", row_stride: int = 0, pad: float = 0.0) -> ObsSpec:
    """The shc_obs_spec of a list of field names (OBS_FIELDS) or SHC_OBS_* integers.  Nothing is checked here: the library judges the spec."""
    st = _row_spec("observation", fields, dtype, row_stride)
    st.legs, st.dof, st.pad = int(legs), int(dof), float(pad)
    return st


def observation_columns(fields, legs: int, dof: int):
    """({name: slice}, width) of a row of observations(fields) for the row geometry (legs, dof): a per-leg field's slice reshapes to (legs, width
    per leg), leg-major.  Computed here and checked against the library's own answer (shc_obs_width / shc_obs_column)."""
    return _row_columns("observation", fields, legs, dof)


def act_spec(fields, legs: int, dof: int, dtype="float32", row_stride: int = 0) -> ActSpec:
    """The shc_act_spec of a list of field names (ACT_FIELDS) or SHC_ACT_* integers.  Nothing is checked here: the library judges the spec."""
    st = _row_spec("action", fields, dtype, row_stride)
    st.legs, st.dof = int(legs), int(dof)
    return st


def action_columns(fields, legs: int, dof: int):
    """({name: slice}, width) of a row of set_actions(fields) for the row geometry (legs, dof): the slice of tip_force reshapes to (legs, 3), that
    of joint_effort to (legs, dof), leg-major.  Computed here and checked against the library's own answer (shc_act_width / shc_act_column)."""
    return _row_columns("action", fields, legs, dof)


def foothold_spec(fields, legs: int, dtype="float32", which: int = 0, mode="request", row_stride: int = 0, pad: float = 0.0) -> FootholdSpec:
    """The shc_foothold_spec of a list of field names (FH_FIELDS) or SHC_FH_* integers.  Nothing is checked here: the library judges the spec."""
    st = _row_spec("foothold", fields, dtype, row_stride)
    st.legs, st.which, st.mode, st.pad = int(legs), int(which), FH_MODES[mode] if isinstance(mode, str) else int(mode), float(pad)
    return st


def foothold_columns(fields, legs: int):
    """({name: slice}, width) of a row of set_footholds(fields) / footholds(fields) for a row geometry of ``legs`` legs: a field's slice reshapes
    to (legs, width per leg), leg-major.  Computed here and checked against the library's own answer (shc_foothold_width / shc_foothold_column)."""
    return _row_columns("foothold", fields, legs, 0)


def reach_spec(fields, legs: int, dof: int, candidates: int, steps: int, dtype="float32", row_stride: int = 0, target_row_stride: int = 0,
               pad: float = float("nan")) -> ReachSpec:
    """The shc_reach_spec of a list of field names (REACH_FIELDS) or SHC_REACH_* integers.  Nothing is checked here: the library judges the spec."""
    st = _row_spec("reach", fields, dtype, row_stride)
    st.legs, st.dof, st.candidates, st.steps = int(legs), int(dof), int(candidates), int(steps)
    st.target_row_stride, st.pad = int(target_row_stride), float(pad)
    return st


def reach_columns(fields, legs: int, dof: int):
    """({name: slice}, width D) of ONE candidate's block of probe_reach(fields) for the row geometry (legs, dof): a field's slice reshapes to
    (legs, width per leg), leg-major.  Computed here and checked against the library's own answer (shc_reach_width / shc_reach_column)."""
    return _row_columns("reach", fields, legs, dof)


def plan_spec(fields, legs: int, horizon: int = 0, dtype="float32", row_stride: int = 0, pad: float = float("nan")) -> PlanSpec:
    """The shc_plan_spec of a list of field names (PLAN_FIELDS) or SHC_PLAN_* integers.  Nothing is checked here: the library judges the spec."""
    st = _row_spec("plan", fields, dtype, row_stride)
    st.legs, st.horizon, st.pad = int(legs), int(horizon), float(pad)
    return st


def plan_columns(fields, legs: int, horizon: int = 0):
    """({name: slice}, width) of a row of step_plan(fields, horizon) for a row geometry of ``legs`` legs: a per-leg field's slice reshapes to
    (legs, width per leg), leg-major - the node fields to (legs, 5, 3), path to (legs, horizon, 3).  Computed here and checked against the
    library's own answer (shc_plan_width / shc_plan_column)."""
    return _row_columns("plan", fields, legs, horizon)


# What each tensor-shaped argument takes (arrays.Need; arrays.read is the one reader).  The 2-D calls refuse with a ValueError; the K-cycle,
# resident and reach calls have no host form and say so with a TypeError ("device arrays only"), the reach probe for another element type too.
_ROWS = arrays.Need(ndim=2, dense_from=1)                                     # (n, >= width): rows contiguous, rows apart - a view of some columns
_ROWS_VIEW, _ROWS_COPY = _ROWS._replace(host="view"), _ROWS._replace(host="copy")   # ... or a numpy array: as it is / a contiguous copy
_ROWS_DEVICE_ONLY = _ROWS._replace(not_device=TypeError)
_CYCLES = arrays.Need(ndim=3, dense_from=2, not_device=TypeError, empty=arrays.DIMENSION)   # (K, n, >= width): the same one level up
_REACH_TARGETS = arrays.Need(ndim=4, dense_from=1, not_device=TypeError, wrong_type=TypeError, empty=arrays.NOTHING)   # dense behind the robots
_REACH_OUT = _REACH_TARGETS._replace(ndim=3)
_FLOAT64, _INT32 = arrays.Need(types=("<f8",)), arrays.Need(types=("<i4",))   # an exact shape (given to read), contiguous
_RECORDS = arrays.Need(types=None)                                            # exactly so many bytes of any element type, contiguous
_OUT_RECORDS = arrays.Need(types=None, exact=False, integer=True, empty=arrays.NOTHING)   # at least so many bytes, or an integer pointer
_OUT_INT64, _OUT_INT32 = _OUT_RECORDS._replace(types=("<i8",)), _OUT_RECORDS._replace(types=("<i4",))
_SOURCE_MAP = arrays.Need(types=("<i8",), host="cast")                        # int64 (n,) on the device, or whatever numpy makes one from
_ONE_INT64 = arrays.Need(types=("<i8",))                                      # one int64 on the device (8 bytes, whatever the shape)


def _geometry(who, legs, dof):
    """The row geometry of a call: the caller's, else the engine's own / the fleet's largest."""
    return who.legs if legs is None else legs, who.dof if dof is None else dof


def _cycle_stride(a) -> int:
    """Elements between the cycles of a 3-D array; 0 for a single cycle (and for none)."""
    return a.strides[0] if a.shape[0] > 1 else 0


def _pointer(a, what: str, need, shape=None, nbytes=None):
    """The pointer of an optional array argument (None stays None)."""
    return None if a is None else arrays.read(a, what, need, shape, nbytes).pointer


_WIDTH_OF = {p.struct: p.width for p in _ROW_PASSES.values()}   # the library's width function of each spec struct


def _row_width(who, spec, what: str) -> int:
    """The library's width of a row of the spec, where an array is made to it: a spec the library refuses is an error here."""
    width = int(getattr(who.L, _WIDTH_OF[type(spec)])(C.byref(spec)))
    if width < 0:
        _check(SHC_ERR_INVALID_ARG, what)
    return width


def _row_pass(who, what: str, a, need, spec, lead: tuple, dtype=None):
    """The steps around every row pass, written once, for BatchEngine and MixedFleet (``who``) and the 2-D, 3-D and reach shapes: read the
    array ``a`` as ``need`` says - or, a None, make a torch tensor (*lead, width) of ``dtype`` on who's device; build the spec from the
    array's element type and the stride of its rows (``spec(dtype, row stride)``: one of obs_spec / act_spec / foothold_spec / reach_spec
    with the call's own members); ask the library for the width; hold the array to lead[-1] rows of at least that many columns (a spec the
    library refuses, width < 0, is left to the call).  Returns (the array read, the spec, the tensor made here or None)."""
    made = None
    if a is None:
        a = made = _new_device_array(lead + (_row_width(who, spec(dtype, 0), what),), dtype, who.device)
    a = arrays.read(a, what, need)
    st = spec(a.dtype, a.strides[need.dense_from - 1])
    width = int(getattr(who.L, _WIDTH_OF[type(st)])(C.byref(st)))
    if a.shape[-2] != lead[-1] or (0 <= width > a.shape[-1]):
        raise ValueError(f"{what} has the shape {a.shape}, {lead[-1]} rows of at least {width} columns are expected")
    return a, st, made


def _new_device_array(shape, dtype, device):
    """An uninitialised torch tensor on the engine's device: what step_k_observations returns when it is given no array to fill."""
    import torch
    return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda" if device is None else f"cuda:{device}")


def _probe_reach(who, call: str, targets, steps, fields, out, first, count, pad, legs, dof):
    """BatchEngine / MixedFleet.probe_reach: ``call`` is the library's entry point - an engine's, which takes a range, or a fleet's.  The
    arrays are judged before the library is asked."""
    legs, dof = _geometry(who, legs, dof)
    ranged, n = isinstance(who, BatchEngine), who.n
    t = arrays.read(targets, "probe_reach: targets", _REACH_TARGETS)
    rows, cands = t.shape[:2]
    if t.shape[2:] != (int(legs), 3):
        raise ValueError(f"probe_reach: targets has the shape {t.shape}, (count, C, {int(legs)}, 3) is expected")
    first, count = int(first), (n - int(first) if ranged else n) if count is None else int(count)
    if rows != count or (not ranged and (first != 0 or count != n)):
        raise ValueError(f"probe_reach: targets has {rows} rows for the robots [{first}, {first + count}) of {n}" + ("" if ranged else " (a fleet takes every robot)"))

    def spec_of(dtype, row_stride):
        if dtype != t.dtype:
            raise TypeError(f"probe_reach: out takes the element type of targets ({t.dtype.name}), got {dtype.name}")
        return reach_spec(fields, legs, dof, cands, steps, dtype, row_stride, t.strides[0], pad)
    width = _row_width(who, spec_of(t.dtype, 0), call)
    o, spec, made = _row_pass(who, "probe_reach: out", out, _REACH_OUT, spec_of, (rows, cands), t.dtype)
    if o.shape != (rows, cands, width):
        raise ValueError(f"probe_reach: out has the shape {o.shape}, {(rows, cands, width)} is expected")
    if rows > 0:   # (an empty tensor has no buffer to speak of, and count = 0 is a no-op in the library)
        _check(getattr(who.L, call)(*((who.h, first, count) if ranged else (who.h,)), C.byref(spec), t.pointer, o.pointer), call)
    return out if made is None else made


def _step_k_rows(who, call: str, what: str, fields, dtype, out, first, count, pad, legs, dof):
    """The ring of the latest K-cycle launch as rows, for BatchEngine / MixedFleet.step_k_observations and .step_k_kinematics: ``call`` is the
    library's entry point (an engine's or a fleet's).  out: a 3-D device array to fill (count None: as many cycles as it has; returns None);
    without out a new torch tensor of ``dtype`` on who's device is filled and returned."""
    legs, dof = _geometry(who, legs, dof)
    if out is None and count is None:
        raise ValueError(f"{what}: give count, or an array to fill")
    a, spec, made = _row_pass(who, f"{what}: out", out, _CYCLES, lambda dt, stride: obs_spec(fields, legs, dof, dt, stride, pad),
                              (max(int(count or 0), 0), who.n), dtype)
    count = a.shape[0] if count is None else int(count)
    if count > a.shape[0]:
        raise ValueError(f"{what}: out has {a.shape[0]} cycles, {count} are asked for")
    _check(getattr(who.L, call)(who.h, int(first), count, C.byref(spec), a.pointer, _cycle_stride(a)), call)
    return made


class DeviceRecords:
    """A (cycles, n) DEVICE array of 32-byte shc_robot_health records: ``__cuda_array_interface__`` names the bytes (ROBOT_HEALTH_DTYPE's
    fields), ``tensor`` is the float64 torch tensor (cycles, n, 4) that owns them, ``numpy()`` their host copy as ROBOT_HEALTH_DTYPE."""

    def __init__(self, tensor):
        self.tensor, self.shape, self.dtype = tensor, tuple(tensor.shape[:2]), ROBOT_HEALTH_DTYPE
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": "|V32", "descr": ROBOT_HEALTH_DTYPE.descr, "data": (tensor.data_ptr(), False),
                                         "strides": None, "version": 3}

    def numpy(self):
        return self.tensor.cpu().numpy().view(ROBOT_HEALTH_DTYPE).reshape(self.shape)


def _step_k_health(who, call: str, select, near_limit_proximity, first, count, health, first_hit):
    """BatchEngine / MixedFleet.step_k_health: ``call`` is the library's entry point; a cycle has who.n records."""
    for name, a in (("health", health), ("first_hit", first_hit)):
        if isinstance(a, np.ndarray):
            raise TypeError(f"step_k_health: {name}: device arrays only (e.g. a torch tensor); the K-cycle launches have no host form")
    if count is None:
        shape = () if health is None else arrays.read(health, "step_k_health: health", _OUT_RECORDS).shape
        if len(shape) < 2:
            raise ValueError("step_k_health: give count, or a health array of (count, n, ..) to fill")
        count = shape[0]
    count, n = int(count), who.n
    if health is None:
        health = DeviceRecords(_new_device_array((max(count, 0), n, 4), np.float64, who.device))
    if first_hit is None:
        first_hit = _new_device_array((n,), np.int32, who.device)
    crit = HealthCriteria(int(select), 0, float(near_limit_proximity), 0.0)
    _check(getattr(who.L, call)(who.h, int(first), count, C.byref(crit), _pointer(health, "health", _OUT_RECORDS, nbytes=max(count, 0) * n * 32),
                                _pointer(first_hit, "first_hit", _OUT_INT32, nbytes=n * 4)), call)
    return health, first_hit


class ShcError(RuntimeError):
    pass


MORPHOLOGIES = [(3, 3), (4, 3), (4, 4), (4, 5), (5, 3), (6, 3), (6, 4), (6, 5), (7, 3), (8, 3), (8, 4), (8, 5)]  # SHC_FOR_EACH_MORPHOLOGY
_OBJ = os.path.join(_HERE, "_build")


def _sources():
    out = [os.path.join(_SRC, f) for f in sorted(os.listdir(_SRC)) if f.endswith((".hip", ".hpp"))]
    out += [os.path.join(_INC, "shc_batch.h"), os.path.join(_INC, "shc_step_plan.h")]
    return out


# -disable-machine-licm: MachineLICM hoists the materialisation of ~100 FP64 literals (polynomial coefficients of
# sincos / atan2, tolerances) out of the n_cycles loop and pins them in VGPRs for the whole launch (256 VGPRs + scratch
# spills); re-materialising them at use keeps the hexapod kernel free of scratch.
# -amdgpu-sched-strategy=max-ilp: at one or two waves per SIMD (the resident loops: two or, in the three-role form of the hexapod loop - 384-thread workgroups,
# walker / model / helper wavefront per robot group - three wavefronts per robot group, a helper sharing its SIMD with a model wavefront) the cycle is bound by dependent-issue latency (FP64
# dependent ops issue every 8 clocks, LDS reads return after ~60); the ILP-first scheduler spends the spare VGPRs
# (the occupancy target of 2 waves/SIMD allows 256) on overlapping independent chains.
_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value",
          "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp"] + os.environ.get("SHC_EXTRA_FLAGS", "").split()  # (development builds)


def compile_with_product_flags(src: str, out: str, extra=()) -> str:
    """Compile one HIP source into the shared library `out` with exactly the flags the shipped kernels are built with (optimisation
    level, fp-contraction default, scheduler options), so that a probe which includes the product's headers exercises the arithmetic
    the engine runs (tests/math_probe.hip).  Include paths inside `src` are relative to the source, as in the product's own units."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + _FLAGS + list(extra) + ["-shared", "-o", out, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stderr[-4000:]}")
    return out


def _translation_units():
    """(object name, source, extra defines): the host side + small kernels, and the fused cycle kernels of each morphology - two objects each:
    the launch forms (part 0) and the loop forms (part 1: resident, batch), so that a build has twice as many units to spread over the cores.
    SHC_GENERIC_LOOP_FORMS=1 in the environment adds the loop forms of the runtime-flag kernel families (shc_cycle_inst.hip)."""
    tus = [("shc_engine.o", os.path.join(_SRC, "shc_engine.hip"), [])]
    generic = ["-DSHC_GENERIC_LOOP_FORMS=1"] if os.environ.get("SHC_GENERIC_LOOP_FORMS", "0") not in ("", "0") else []
    for l, nj in MORPHOLOGIES:
        for part, tag in ((0, "launch"), (1, "loop")):
            tus.append((f"shc_cycle_{l}_{nj}_{tag}.o", os.path.join(_SRC, "shc_cycle_inst.hip"),
                        [f"-DSHC_INST_L={l}", f"-DSHC_INST_NJ={nj}", f"-DSHC_INST_PART={part}"] + (generic if part == 1 else [])))
    return tus


def _source_hash() -> str:
    """Content hash of everything the library is built from (sources, ABI header, flags).  A hash, not mtimes: the in-tree
    .so travels to the GPU box in a snapshot that does not keep modification times."""
    import hashlib
    h = hashlib.sha256((" ".join(_FLAGS) + repr(MORPHOLOGIES) + repr([(n, d) for n, _, d in _translation_units()])).encode())
    for s in _sources():
        with open(s, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _include_closure(src: str):
    """The files one translation unit is built from: the source and, transitively, every `#include "..."` it names (system headers are the toolchain's)."""
    import re
    seen, todo = [], [os.path.realpath(src)]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.append(f)
        with open(f, "r", errors="replace") as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), flags=re.M):
                todo.append(os.path.realpath(os.path.join(os.path.dirname(f), inc)))
    return sorted(seen)


def _tu_hash(src: str, defines) -> str:
    """Hash of what one object depends on: its source and the headers it includes (transitively), flags, defines - a change to a header only the
    host side includes (init chain, sequences, fleets, snapshots) rebuilds shc_engine.o alone, not the cycle kernels of twelve morphologies."""
    import hashlib
    h = hashlib.sha256((" ".join(_FLAGS + list(defines))).encode())
    for s in _include_closure(src):
        with open(s, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build_library(force: bool = False, verbose: bool = False, jobs: Optional[int] = None, resource_report: Optional[str] = None) -> str:
    """Compile the library for gfx950 (in-tree libshc_batch.so) unless the existing one was built from exactly these sources:
    one object per translation unit (host side; the cycle kernels of each morphology) compiled in parallel, objects whose
    inputs did not change are reused.  hipcc cross-compiles without a GPU.  resource_report: a file that receives hipcc's
    -Rpass-analysis=kernel-resource-usage remarks (scripts/regs.py reads it)."""
    stamp = _SO + ".srchash"
    want = _source_hash()
    have_stamp = os.path.exists(stamp) and open(stamp).read().strip() == want
    if not force and os.path.exists(_SO) and have_stamp:
        return _SO
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    import shutil
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        if os.path.exists(_SO):  # a prebuilt library on a host without the compiler: the sizeof checks in lib() guard ABI drift
            import warnings
            warnings.warn("libshc_batch.so carries no matching source stamp and hipcc is not available: loading it as it is")
            return _SO
        raise FileNotFoundError(f"{_SO} is missing and {hipcc} is not available to build it")
    os.makedirs(_OBJ, exist_ok=True)
    # several ranks of one node may get here at once (torch.distributed.run): one of them builds, the others wait and find the stamp
    import fcntl
    lock = open(_SO + ".lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        if not force and os.path.exists(_SO) and os.path.exists(stamp) and open(stamp).read().strip() == want:
            return _SO
        return _build_locked(force, verbose, jobs, resource_report, hipcc, stamp, want)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _build_locked(force, verbose, jobs, resource_report, hipcc, stamp, want):
    from concurrent.futures import ThreadPoolExecutor
    todo, objs = [], []
    for name, src, defines in _translation_units():
        obj = os.path.join(_OBJ, name)
        objs.append(obj)
        th = _tu_hash(src, defines)
        ostamp = obj + ".srchash"
        if force or resource_report or not (os.path.exists(obj) and os.path.exists(ostamp) and open(ostamp).read().strip() == th):
            todo.append((obj, src, defines, th))

    # longest first: the two BASELINE morphologies carry twice the kernels of the others (feature-exact families, half kernels) and the host side is the
    # third-longest unit; started last they would run alone at the end (measured on 8 cores: 150 s in source order, the longest unit alone 82 s)
    weight = {"shc_cycle_8_5_loop.o": 0, "shc_cycle_8_5_launch.o": 0, "shc_cycle_6_3_loop.o": 1, "shc_cycle_6_3_launch.o": 1, "shc_engine.o": 2}
    todo.sort(key=lambda job: (weight.get(os.path.basename(job[0]), 3), job[0]))

    def compile_one(job):
        obj, src, defines, th = job
        cmd = [hipcc] + _FLAGS + list(defines) + ["-c", "-o", obj, src]
        if resource_report:
            cmd.append("-Rpass-analysis=kernel-resource-usage")
        if verbose:
            print(" ".join(cmd), flush=True)
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise subprocess.CalledProcessError(r.returncode, cmd, r.stdout, r.stderr[-4000:])
        if verbose or os.environ.get("SHC_BUILD_TIMES"):
            print(f"[shc build] {os.path.basename(obj)} {time.perf_counter() - t0:.1f} s", flush=True)
        with open(obj + ".srchash", "w") as f:
            f.write(th + "\n")
        return r.stderr

    with ThreadPoolExecutor(max_workers=jobs or min(len(todo) or 1, os.cpu_count() or 1)) as ex:
        try:
            reports = list(ex.map(compile_one, todo))
        except subprocess.CalledProcessError as e:
            raise RuntimeError(f"hipcc failed: {' '.join(e.cmd)}\n{e.stderr}") from None
    if resource_report:
        with open(resource_report, "w") as f:
            f.write("".join(reports))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", _SO] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(want + "\n")
    return _SO


_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _share_torch_hip_runtime():
    """PyTorch wheels bundle a HIP runtime of their own.  A process that initialises /opt/rocm's runtime first (libshc_batch.so links against it) and
    imports torch afterwards ends up with two runtimes, and the second one finds no device ("No HIP GPUs are available", measured on the GPU box).
    Loaded the other way round both share torch's - the configuration tests/ and bench.py have always run in.  So: when torch is installed but not
    imported yet, its libamdhip64.so is loaded first (one dlopen, no torch import); the library then binds to it by SONAME and a later
    `import torch` finds its runtime already in place.  SHC_OWN_HIP_RUNTIME=1 keeps /opt/rocm's (a process that never imports torch)."""
    if "torch" in sys.modules or os.environ.get("SHC_OWN_HIP_RUNTIME"):
        return
    import warnings
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if not (spec and spec.submodule_search_locations):
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if not os.path.exists(cand):
            return
        # The library is linked against /opt/rocm's runtime by SONAME: only a bundled runtime of the SAME SONAME can stand in for it (a different one would be
        # loaded next to it - two runtimes after all), and code objects built by one ROCm release are run by the other's runtime only within that ABI.
        needed, bundled = _elf_soname(_SO, b"libamdhip64.so", needed=True), _elf_soname(cand, b"libamdhip64.so", needed=False)
        if needed and bundled and needed != bundled:
            warnings.warn(f"torch bundles HIP runtime {bundled} but libshc_batch.so is linked against {needed}: not pre-loading torch's runtime "
                          "(import torch BEFORE the engine in a process that needs both, or set SHC_OWN_HIP_RUNTIME=1 to silence this)")
            return
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        if os.environ.get("SHC_VERBOSE"):
            print(f"[shc] HIP runtime shared with torch: {cand} ({bundled or 'SONAME unknown'})", file=sys.stderr)
    except OSError as exc:  # the bundled runtime would not load: /opt/rocm's it is, and a later `import torch` may then find no device - say so
        warnings.warn(f"could not pre-load torch's bundled HIP runtime ({exc}); import torch before the engine if this process uses both")


def _elf_soname(path: str, stem: bytes, needed: bool):
    """The `stem`.N string an ELF file names - its DT_NEEDED entry (needed=True) or its own DT_SONAME; found by scanning the dynamic string table's bytes
    (no ELF parser in the image: both are NUL-terminated strings that start with the stem).  None when nothing matches."""
    import re
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    names = sorted(set(m.group(0).decode() for m in re.finditer(re.escape(stem) + rb"(\.\d+)+(?=\x00)", blob)))
    return names[0] if names else None


def lib():
    """Load libshc_batch.so, (re)building it first when it is missing or was built from different sources."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        L = C.CDLL(_SO if os.environ.get("SHC_LIB") else build_library())
        cheader.bind(L, HEADER.functions)
        cheader.bind(L, PLAN_HEADER.functions)
        # a binding whose struct layouts disagree with the library must not run
        for name, typ in (("shc_sizeof_params", Params), ("shc_sizeof_tables", Tables), ("shc_sizeof_instance_state", InstanceState)):
            if getattr(L, name)() != C.sizeof(typ):
                raise ShcError(f"{name}() = {getattr(L, name)()} but the ctypes mirror has {C.sizeof(typ)} bytes")
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != SHC_OK:
        msg = lib().shc_last_error()
        raise ShcError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def device_count() -> int:
    return lib().shc_device_count()


def generate_tables(params: Params) -> Tables:
    """Host init chain of the product (start-up solve, workspace search, walkspace, limits)."""
    t = Tables()
    _check(lib().shc_generate_tables(C.byref(params), C.byref(t)), "shc_generate_tables")
    return t


def _host(a, dtype=np.float64):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def generate_tables_batch(params_list, device: int = 0):
    """Init chain of many morphologies in one go on the GPU.  Returns (list of Tables, status array)."""
    n = len(params_list)
    arr = (Params * n)(*params_list)
    out = (Tables * n)()
    status = (C.c_int32 * n)()
    _check(lib().shc_generate_tables_batch(arr, n, out, status, device), "shc_generate_tables_batch")
    return list(out), np.array(status[:], dtype=np.int32)


class Checkpoint:
    """The state of every robot of an engine, kept in device memory (shc_engine_checkpoint_create): what ``BatchEngine.restore`` resets or clones
    robots from.  A context manager; ``close()`` after the engine's ``close()`` is a no-op for the caller."""

    def __init__(self, engine: "BatchEngine"):
        self.engine, self.L, self.h = engine, engine.L, None
        h = C.c_void_p()
        _check(self.L.shc_engine_checkpoint_create(engine.h, C.byref(h)), "checkpoint_create")
        self.h = h

    def update(self):
        """Capture the engine's state again into the same device storage: stream-ordered copies, no host wait."""
        _check(self.L.shc_engine_checkpoint_update(self.engine.h, self.h), "checkpoint_update")

    @property
    def nbytes(self) -> int:
        return int(self.L.shc_checkpoint_bytes(self.h)) if self.h else 0

    def close(self):
        if getattr(self, "h", None):
            self.L.shc_checkpoint_destroy(self.h)   # (a handle whose engine is gone holds nothing on the device: this frees the handle itself)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchEngine:
    """A batch of ``n`` robots of one morphology/gait advancing through control cycles on one MI355X."""

    def __init__(self, params: Params, n: int, device: int = 0, stream: int = 0, tables: Optional[Tables] = None):
        self.L = lib()
        if self.L.shc_device_count() < 1:
            raise ShcError("no HIP device visible: the batched engine has no CPU fallback")
        self.params, self.n = Params.from_buffer_copy(params), int(n)   # (the engine's own: adjust_parameter updates it)
        self.legs, self.dof = params.leg_count, max(params.leg_dof[l] for l in range(params.leg_count))   # joint arrays are [legs][longest leg's DOF]
        self.features = FEAT_DEFAULT
        h = C.c_void_p()
        if tables is None:
            _check(self.L.shc_engine_create(C.byref(params), self.n, device, C.c_void_p(stream), C.byref(h)), "shc_engine_create")
        else:
            _check(self.L.shc_engine_create_with_tables(C.byref(params), C.byref(tables), self.n, device, C.c_void_p(stream),
                                                        C.byref(h)), "shc_engine_create_with_tables")
        self.h, self.device = h, int(device)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owned", True):
                self.L.shc_engine_destroy(self.h)
            self.h = None

    @classmethod
    def view(cls, handle: int, params: Params, n: int):
        """A non-owning view of an engine somebody else created (a part of a fleet: shc_fleet_part) - for device-resident I/O and state records
        through the shc_engine_* calls; closing the view leaves the engine alone."""
        self = cls.__new__(cls)
        self.L, self.h, self._owned = lib(), C.c_void_p(handle), False
        self.params, self.n, self.device = params, int(n), None
        self.legs, self.dof = params.leg_count, max(params.leg_dof[l] for l in range(params.leg_count))
        self.features = FEAT_DEFAULT
        return self

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration
    def set_stream(self, stream: int):
        _check(self.L.shc_engine_set_stream(self.h, C.c_void_p(stream)), "set_stream")

    def set_features(self, features: int):
        _check(self.L.shc_engine_set_features(self.h, features), "set_features")
        self.features = int(features)

    def tables(self) -> Tables:
        t = Tables()
        _check(self.L.shc_engine_get_tables(self.h, C.byref(t)), "get_tables")
        return t

    # -- inputs (host numpy arrays)
    def set_velocity(self, linear_xy=None, angular=None):
        a, b = _host(linear_xy), _host(angular)
        _check(self.L.shc_engine_set_velocity(self.h, _p(a), _p(b), 0), "set_velocity")

    def set_imu(self, quat_wxyz=None, gyro=None):
        a, b = _host(quat_wxyz), _host(gyro)
        _check(self.L.shc_engine_set_imu(self.h, _p(a), _p(b), 0), "set_imu")

    def set_tip_force(self, force):
        a = _host(force)
        _check(self.L.shc_engine_set_tip_force(self.h, _p(a), 0), "set_tip_force")

    def set_joint_effort(self, effort):
        a = _host(effort)
        _check(self.L.shc_engine_set_joint_effort(self.h, _p(a), 0), "set_joint_effort")

    def set_pose_input(self, translation_velocity=None, rotation_velocity=None):
        a, b = _host(translation_velocity), _host(rotation_velocity)
        _check(self.L.shc_engine_set_pose_input(self.h, _p(a), _p(b), 0), "set_pose_input")

    def set_pose_reset_mode(self, mode):
        a = _host(mode, np.int32)
        _check(self.L.shc_engine_set_pose_reset_mode(self.h, _p(a), 0), "set_pose_reset_mode")

    def set_actions(self, actions, fields, legs: Optional[int] = None, dof: Optional[int] = None):
        """Chosen input groups (names of ACT_FIELDS, in column order) of every instance from one 2-D array of n rows in one device pass
        (shc_engine_set_actions); ``action_columns(fields, legs, dof)`` names the columns.  The engine is left as the device setters leave it when
        they are given the columns as float64 arrays; groups not named are held.  actions: a float32 / float64 device array
        (``__cuda_array_interface__``; a view of some columns of a wider array will do) of at least the width in columns, read on the engine's
        stream without a host wait and never written - or a numpy array, which is copied to the device and waited for.  legs / dof (default: the
        engine's) may be larger than the robot's: the columns of legs and joints it lacks are ignored."""
        legs, dof = _geometry(self, legs, dof)
        a, spec, _ = _row_pass(self, "set_actions: actions", actions, _ROWS_COPY, lambda dt, stride: act_spec(fields, legs, dof, dt, stride), (self.n,))
        _check(self.L.shc_engine_set_actions(self.h, C.byref(spec), a.pointer, a.on_device), "set_actions")

    # -- inputs (device pointers, e.g. torch tensors' data_ptr())
    def set_velocity_device(self, linear_ptr: Optional[int], angular_ptr: Optional[int]):
        _check(self.L.shc_engine_set_velocity(self.h, C.c_void_p(linear_ptr), C.c_void_p(angular_ptr), 1), "set_velocity")

    # -- stepping
    def step(self, n_cycles: int = 1):
        _check(self.L.shc_engine_step(self.h, int(n_cycles)), "step")

    def step_k(self, n_cycles: int, velocity=None, imu=None, tip_force=None, joint_effort=None):
        """K cycles in one launch, cycle k with row k of the K-deep DEVICE arrays (integer device pointers, e.g. torch.Tensor.data_ptr()):
        velocity = (linear [K][n][2], angular [K][n]), imu = (quat [K][n][4], gyro [K][n][3]), tip_force [K][n][legs][3],
        joint_effort [K][n][legs][dof]; None = held (shc_engine_step_k)."""
        ci = CycleInputs()
        if velocity is not None:
            ci.linear_xy, ci.angular = velocity[0] or None, velocity[1] or None
        if imu is not None:
            ci.imu_orientation_wxyz, ci.imu_angular_velocity = imu[0] or None, imu[1] or None
        if tip_force is not None:
            ci.tip_force = int(tip_force)
        if joint_effort is not None:
            ci.joint_effort = int(joint_effort)
        ci.on_device = 1
        _check(self.L.shc_engine_step_k(self.h, int(n_cycles), C.byref(ci)), "shc_engine_step_k")

    def step_k_joints(self, k: int):
        """q, qd [n][legs * dof] of cycle k of the latest step_k (host arrays)."""
        q = np.empty((self.n, self.legs * self.dof), dtype=np.float64)
        qd = np.empty_like(q)
        _check(self.L.shc_engine_get_step_k_joint_state(self.h, int(k), _p(q), _p(qd), 0), "shc_engine_get_step_k_joint_state")
        return q, qd

    def step_k_actions(self, actions, fields, legs: Optional[int] = None, dof: Optional[int] = None):
        """K = ``actions.shape[0]`` cycles in one launch, cycle k with the rows ``actions[k]`` (shc_engine_step_k_actions): ``step_k`` driven by one
        3-D float32 / float64 DEVICE array (K, n, at least A columns) - ``action_columns(fields, legs, dof)`` names the columns; a view
        ``big[:, :, 5:5 + A]`` of a wider tensor will do.  The engine is left as ``step_k`` leaves it when given the columns as float64 arrays;
        groups not named are held; velocity and IMU are named in pairs, the pose inputs are refused.  Read on the engine's stream without a host
        wait: the array may be rewritten once that stream has passed the call.  A numpy array is a TypeError (device arrays only)."""
        legs, dof = _geometry(self, legs, dof)
        a, spec, _ = _row_pass(self, "step_k_actions: actions", actions, _CYCLES, lambda dt, stride: act_spec(fields, legs, dof, dt, stride), (self.n,))
        _check(self.L.shc_engine_step_k_actions(self.h, a.shape[0], C.byref(spec), a.pointer, _cycle_stride(a)), "shc_engine_step_k_actions")

    def step_k_observations(self, fields=("q", "qd"), dtype="float32", out=None, first: int = 0, count: Optional[int] = None, pad: float = 0.0,
                            legs: Optional[int] = None, dof: Optional[int] = None):
        """q / qd (``fields``: "q", "qd" or both, in column order) of cycles [first, first + count) of the latest ``step_k`` /
        ``step_k_actions`` as one (count, n, D) DEVICE array in one pass (shc_engine_get_step_k_observations):
        ``observation_columns(fields, legs, dof)`` names the columns, every value is what ``step_k_joints(first + k)`` holds, cast to the
        element type, ``pad`` where the row geometry (legs, dof) is larger than the robot.  out: a 3-D float32 / float64 device array (a view
        of some columns of a wider one will do) whose first D columns are filled on the engine's stream without a host wait - count None: as
        many cycles as it has; returns None.  Without out (give count) a new torch tensor of ``dtype`` on the engine's device is filled and
        returned."""
        return _step_k_rows(self, "shc_engine_get_step_k_observations", "step_k_observations", fields, dtype, out, first, count, pad, legs, dof)

    def step_k_kinematics(self, fields=("q", "qd", "model_tip"), dtype="float32", out=None, first: int = 0, count: Optional[int] = None, pad: float = 0.0,
                          legs: Optional[int] = None, dof: Optional[int] = None):
        """``step_k_observations`` with the foot tips: ``fields`` is any of "q", "qd" and "model_tip" (in column order), and model_tip of cycle
        first + k is what ``observations(("model_tip",))`` gives on an engine whose joints are those of that cycle - FK(q) in the robot frame,
        3 columns per leg, ``pad`` where the robot has no such leg (shc_engine_get_step_k_kinematics).  One pass over the ring of the latest
        ``step_k`` / ``step_k_actions`` on the engine's stream, no host wait; nothing is written into the engine.  out, count and the return
        value as ``step_k_observations``; a numpy array is a TypeError (device arrays only)."""
        return _step_k_rows(self, "shc_engine_get_step_k_kinematics", "step_k_kinematics", fields, dtype, out, first, count, pad, legs, dof)

    def step_k_health(self, select: int = 0, near_limit_proximity: float = 0.0, first: int = 0, count: Optional[int] = None, health=None, first_hit=None):
        """The joint-limit half of ``scan_health`` for cycles [first, first + count) of the latest ``step_k`` / ``step_k_actions`` in one pass
        over its ring (shc_engine_scan_step_k_health): returns the DEVICE arrays (health, first_hit).  health: (count, n) records of
        ROBOT_HEALTH_DTYPE's bytes - min_limit_proximity, max_speed_ratio, bytes 1 and 2 of leg_masks and the flags HEALTH_POSITION_LIMIT,
        HEALTH_SPEED_LIMIT, HEALTH_NEAR_LIMIT (below ``near_limit_proximity``) and HEALTH_NONFINITE (joints only) are live, max_tip_deviation
        is 0.  first_hit: int32 (n,), the first cycle of the launch within the range whose flags meet ``select``, or -1.  select with
        HEALTH_IK_DEVIATION or HEALTH_TIP_DEVIATION is refused: the ring holds joints.  health / first_hit: device buffers to fill (integer
        pointers or objects with ``__cuda_array_interface__``; count None: health.shape[0]), returned as given; else a new ``DeviceRecords`` /
        torch tensor.  On the engine's stream, no host wait; a numpy array is a TypeError (device arrays only)."""
        return _step_k_health(self, "shc_engine_scan_step_k_health", select, near_limit_proximity, first, count, health, first_hit)

    def synchronize(self):
        _check(self.L.shc_engine_synchronize(self.h), "synchronize")

    def join(self):
        """Order the engine's stream after both halves of earlier split steps (large batches; no host wait)."""
        _check(self.L.shc_engine_join(self.h), "join")

    # -- resident mode: the control loop kept on the chip (shc_engine_resident_*)
    def resident_begin(self, ring_depth: int = 16, max_cycles: int = 1 << 24, idle_timeout_ms: int = 0):
        _check(self.L.shc_engine_resident_begin(self.h, int(ring_depth), int(max_cycles), int(idle_timeout_ms)), "resident_begin")

    def resident_bind_inputs(self, input_set: int, velocity=None, imu=None, tip_force=None, joint_effort=None):
        """Bind device arrays (integer pointers) as input set 0 .. 3 for direct posts; before resident_begin."""
        ci = CycleInputs()
        if velocity is not None:
            ci.linear_xy, ci.angular = velocity[0] or None, velocity[1] or None
        if imu is not None:
            ci.imu_orientation_wxyz, ci.imu_angular_velocity = imu[0] or None, imu[1] or None
        ci.tip_force = None if tip_force is None else int(tip_force)
        ci.joint_effort = None if joint_effort is None else int(joint_effort)
        ci.on_device = 1
        _check(self.L.shc_engine_resident_bind_inputs(self.h, int(input_set), C.byref(ci)), "resident_bind_inputs")

    def resident_direct_poster(self, input_set: int, velocity=False, imu=False, tip_force=False, joint_effort=False):
        """A bound C call that posts the named groups of bound input set `input_set` as a DIRECT cycle (no kernel launch, no copy, released
        at once): the per-iteration call of a host loop without the Python wrapper's per-call marshalling, which costs more than the 3 us
        cycle.  Returns f() -> return code."""
        ci = CycleInputs()
        one = 1  # (any non-NULL value: a direct post only looks at WHICH members are set)
        if velocity:
            ci.linear_xy, ci.angular = one, one
        if imu:
            ci.imu_orientation_wxyz, ci.imu_angular_velocity = one, one
        if tip_force:
            ci.tip_force = one
        if joint_effort:
            ci.joint_effort = one
        ci.on_device, ci.publish, ci.direct = 1, 1, int(input_set) + 1
        f, h, ref = self.L.shc_engine_resident_post, self.h, C.byref(ci)

        def post(_keep=ci):
            return f(h, ref, None)
        return post

    def resident_post(self, velocity=None, imu=None, pose_input=None, pose_reset_mode=None, tip_force=None, joint_effort=None, on_device=False,
                      publish=False, direct=None) -> int:
        """Inputs of the next unposted cycle: velocity = (linear_xy, angular), imu = (quat_wxyz, gyro), pose_input = (translation
        velocity, rotation velocity); host numpy arrays, or integer device pointers with on_device.  direct = k: a launch-free post from
        bound input set k (resident_bind_inputs): the arguments only name the fresh groups (any true value).  Returns the cycle index."""
        if direct is not None:
            on_device = True
            one = 1
            velocity = None if velocity is None else (one, one)
            imu = None if imu is None else (one, one)
            tip_force = None if tip_force is None else one
            joint_effort = None if joint_effort is None else one
        keep = []

        def ptr(a, dtype=np.float64):
            if a is None:
                return None
            if on_device:
                return int(a)
            h = _host(a, dtype)
            keep.append(h)
            return h.ctypes.data

        ci = CycleInputs()
        if velocity is not None:
            ci.linear_xy, ci.angular = ptr(velocity[0]), ptr(velocity[1])
        if imu is not None:
            ci.imu_orientation_wxyz, ci.imu_angular_velocity = ptr(imu[0]), ptr(imu[1])
        if pose_input is not None:
            ci.pose_translation_velocity, ci.pose_rotation_velocity = ptr(pose_input[0]), ptr(pose_input[1])
        ci.pose_reset_mode = ptr(pose_reset_mode, np.int32)
        ci.tip_force, ci.joint_effort = ptr(tip_force), ptr(joint_effort)
        ci.on_device = 1 if on_device else 0
        ci.publish = 1 if publish else 0
        ci.direct = 0 if direct is None else int(direct) + 1
        cyc = C.c_int64(-1)
        _check(self.L.shc_engine_resident_post(self.h, C.byref(ci), C.byref(cyc)), "resident_post")
        return int(cyc.value)

    def resident_publish(self, n_cycles: int = 1):
        _check(self.L.shc_engine_resident_publish(self.h, int(n_cycles)), "resident_publish")

    def resident_wait(self, cycles: int, timeout_ms: int = 0):
        _check(self.L.shc_engine_resident_wait(self.h, int(cycles), int(timeout_ms)), "resident_wait")

    def resident_joints(self, cycle: int):
        q = np.zeros((self.n, self.legs * self.dof))
        qd = np.zeros((self.n, self.legs * self.dof))
        _check(self.L.shc_engine_resident_get_joint_state(self.h, int(cycle), _p(q), _p(qd), 0), "resident_get_joint_state")
        return q, qd

    def resident_joints_async(self, cycle: int, q_ptr: int, qd_ptr: int = 0, timeout_ms: int = 0):
        """Stream-ordered read into device buffers (raw pointers, [n][legs][dof]): queued on the engine's stream behind a device-side
        wait for `cycle`; returns at once."""
        _check(self.L.shc_engine_resident_get_joint_state_async(self.h, int(cycle), C.c_void_p(q_ptr or None), C.c_void_p(qd_ptr or None), int(timeout_ms)),
               "resident_get_joint_state_async")

    def resident_post_actions(self, actions, fields, publish: bool = False, legs: Optional[int] = None, dof: Optional[int] = None) -> int:
        """``resident_post`` for the next unposted cycle from one 2-D float32 / float64 DEVICE array of n rows
        (shc_engine_resident_post_actions): ``action_columns(fields, legs, dof)`` names the columns, a view of some columns of a wider tensor
        will do.  The loop runs as after ``resident_post(on_device=True)`` with the columns as float64 arrays; groups not named are held;
        velocity, IMU and pose fields are named in pairs.  One kernel launch, nothing staged.  The array must be ready on the ENGINE's stream
        and may be overwritten by work queued there behind the call; no host wait.  publish: release the cycle in the same launch.  Refused
        while a stream-ordered read (``resident_observations``, ``resident_joints_async``) of an unpublished cycle is pending.  Returns the
        cycle index.  A numpy array is a TypeError (device arrays only)."""
        legs, dof = _geometry(self, legs, dof)
        a, spec, _ = _row_pass(self, "resident_post_actions: actions", actions, _ROWS_DEVICE_ONLY,
                               lambda dt, stride: act_spec(fields, legs, dof, dt, stride), (self.n,))
        cyc = C.c_int64(-1)
        _check(self.L.shc_engine_resident_post_actions(self.h, C.byref(spec), a.pointer, 1 if publish else 0, C.byref(cyc)), "resident_post_actions")
        return int(cyc.value)

    def resident_observations(self, cycle: int, fields=("q", "qd"), dtype="float32", out=None, pad: float = 0.0, legs: Optional[int] = None,
                              dof: Optional[int] = None, timeout_ms: int = 0):
        """q / qd / model_tip (``fields``, in column order) of iteration ``cycle`` of the resident loop as one (n, D) DEVICE array, stream-ordered
        (shc_engine_resident_get_observations_async): ``observation_columns(fields, legs, dof)`` names the columns; q / qd are what
        ``resident_joints(cycle)`` holds, cast to the element type, model_tip is FK(q) in the robot frame, ``pad`` where the row geometry
        (legs, dof) is larger than the robot.  Queued on the engine's stream behind a device-side wait for the cycle (which may still be
        unpublished; bounded by timeout_ms, 0 = 5 s); returns at once and writes nothing into the engine.  out: a 2-D float32 / float64 device
        array (a view of some columns of a wider one will do) whose first D columns are filled; returns None.  Without out a new torch tensor
        of ``dtype`` on the engine's device is filled and returned.  A numpy array is a TypeError (device arrays only)."""
        legs, dof = _geometry(self, legs, dof)
        a, spec, made = _row_pass(self, "resident_observations: out", out, _ROWS_DEVICE_ONLY,
                                  lambda dt, stride: obs_spec(fields, legs, dof, dt, stride, pad), (self.n,), dtype)
        _check(self.L.shc_engine_resident_get_observations_async(self.h, int(cycle), C.byref(spec), a.pointer, int(timeout_ms)), "resident_observations")
        return made

    def resident_status(self):
        pub, done, run = C.c_int64(), C.c_int64(), C.c_int32()
        _check(self.L.shc_engine_resident_status(self.h, C.byref(pub), C.byref(done), C.byref(run)), "resident_status")
        return int(pub.value), int(done.value), bool(run.value)

    def resident_end(self) -> int:
        ran = C.c_int64(0)
        _check(self.L.shc_engine_resident_end(self.h, C.byref(ran)), "resident_end")
        return int(ran.value)

    # -- outputs
    def joints(self):
        q = np.zeros((self.n, self.legs * self.dof))
        qd = np.zeros((self.n, self.legs * self.dof))
        _check(self.L.shc_engine_get_joint_state(self.h, _p(q), _p(qd), 0), "get_joint_state")
        return q, qd

    def joints_device(self, q_ptr: Optional[int], qd_ptr: Optional[int]):
        _check(self.L.shc_engine_get_joint_state(self.h, C.c_void_p(q_ptr), C.c_void_p(qd_ptr), 1), "get_joint_state")

    def joint_buffer(self):
        """(device pointer, n_doubles) of the engine's own SoA joint-position planes (the all-gather payload)."""
        ptr, n = C.c_void_p(), C.c_int64()
        _check(self.L.shc_engine_joint_buffer(self.h, C.byref(ptr), C.byref(n)), "joint_buffer")
        return ptr.value, n.value

    def joint_index(self, instance: int, leg: int, joint: int) -> int:
        return self.L.shc_engine_joint_index(self.h, instance, leg, joint)

    def leg_state(self):
        out = {k: np.zeros((self.n, self.legs, 3)) for k in ("walker_tip", "poser_tip", "model_tip", "tip_force", "admittance")}
        st = np.zeros((self.n, self.legs), dtype=np.int32)
        _check(self.L.shc_engine_get_leg_state(self.h, _p(out["walker_tip"]), _p(out["poser_tip"]), _p(out["model_tip"]),
                                               _p(out["tip_force"]), _p(out["admittance"]), _p(st), 0), "get_leg_state")
        out["leg_status"] = st
        return out

    def body_state(self):
        pose = np.zeros((self.n, 7))
        vel = np.zeros((self.n, 3))
        ws = np.zeros(self.n, dtype=np.int32)
        _check(self.L.shc_engine_get_body_state(self.h, _p(pose), _p(vel), _p(ws), 0), "get_body_state")
        return pose, vel, ws

    def change_gait(self, new_gait: Params) -> int:
        """StateController::changeGait for the whole batch.  Returns the number of instances still walking (their velocity
        inputs have been zeroed; step on and call again); 0 means the gait was changed."""
        still = C.c_int64(0)
        _check(self.L.shc_engine_change_gait(self.h, C.byref(new_gait), C.byref(still)), "change_gait")
        if still.value == 0:
            self.params = Params.from_buffer_copy(new_gait)
        return int(still.value)

    def adjust_parameter(self, which: int, value: float) -> int:
        """StateController::adjustParameter for the whole batch (which: params.PARAM_*, enum ParameterSelection).  Returns the number of instances
        whose desired velocity is still outside the new limits (step_frequency only: call again after the next cycle); 0 = the value is set.
        self.params follows: the engine stores the value at once, a step_frequency that still waits included (state_controller.cpp:454)."""
        pending = C.c_int64(0)
        _check(self.L.shc_engine_adjust_parameter(self.h, int(which), float(value), C.byref(pending)), "adjust_parameter")
        from .params import PARAM_FIELD
        setattr(self.params, PARAM_FIELD[int(which)], float(value))
        return int(pending.value)

    def leg_state_msg(self, instance: int):
        """Numeric payload of LegState.msg for every leg of one instance (StateController::publishLegState)."""
        arr = (LegStateMsg * self.legs)()
        _check(self.L.shc_engine_read_leg_state_msg(self.h, int(instance), arr), "read_leg_state_msg")
        return list(arr)

    def leg_state_msgs(self, first: int = 0, count: Optional[int] = None, out: Optional[int] = None):
        """publishLegState for instances [first, first + count) in one device pass (shc_engine_get_leg_state_msgs): a structured array of
        shape (count, legs) with the fields of LegStateMsg (LEG_STATE_MSG_DTYPE).  out = a device pointer (integer, 16-byte aligned, room for
        count * legs records of 512 B): the records are written there, ordered on the engine's stream without a host wait; returns None."""
        count = self.n - first if count is None else count
        if out is not None:
            _check(self.L.shc_engine_get_leg_state_msgs(self.h, int(first), int(count), C.c_void_p(int(out)), 1), "get_leg_state_msgs")
            return None
        msgs = np.zeros((max(int(count), 0), self.legs), dtype=LEG_STATE_MSG_DTYPE)
        _check(self.L.shc_engine_get_leg_state_msgs(self.h, int(first), int(count), msgs.ctypes.data_as(C.c_void_p), 0), "get_leg_state_msgs")
        return msgs

    def observations(self, fields, dtype="float32", out=None, first: int = 0, count: Optional[int] = None, pad: float = 0.0, legs: Optional[int] = None,
                     dof: Optional[int] = None):
        """Chosen fields (names of OBS_FIELDS, in column order) of instances [first, first + count) as one (count, D) array in one device pass
        (shc_engine_get_observations); ``observation_columns(fields, legs, dof)`` names the columns.  Every value is the double the matching
        getter returns (joints, leg_state_msgs, frame_transforms, get_body_state, leg_state), cast to ``dtype``; legs / dof (default: the engine's)
        may be larger than the robot's, the columns of legs and joints it lacks then hold ``pad``.  Returns a host array - or, with out = a 2-D
        float32 / float64 device array (``__cuda_array_interface__``; a view of some columns of a wider array will do) of count rows and at least
        D columns, fills its first D columns on the engine's stream without a host wait and returns None: dtype then is the array's."""
        count = self.n - first if count is None else count
        legs, dof = _geometry(self, legs, dof)
        if out is not None:
            a, spec, _ = _row_pass(self, "observations: out", out, _ROWS, lambda dt, stride: obs_spec(fields, legs, dof, dt, stride, pad),
                                   (int(count),))
            _check(self.L.shc_engine_get_observations(self.h, int(first), int(count), C.byref(spec), a.pointer, 1), "get_observations")
            return None
        spec = obs_spec(fields, legs, dof, dtype, 0, pad)
        obs = np.zeros((max(int(count), 0), _row_width(self, spec, "get_observations")), dtype=np.dtype(dtype))
        # (an empty array has no buffer to speak of: count = 0 is a no-op in the library, which still judges the arguments)
        _check(self.L.shc_engine_get_observations(self.h, int(first), int(count), C.byref(spec), obs.ctypes.data_as(C.c_void_p), 0), "get_observations")
        return obs

    def step_plan(self, fields, horizon: int = 0, dtype="float32", out=None, first: int = 0, count: Optional[int] = None, pad: float = float("nan"),
                  legs: Optional[int] = None):
        """What every LegStepper of instances [first, first + count) is doing with its target, as one (count, D) array in one device pass
        (shc_engine_get_step_plan): chosen fields (names of PLAN_FIELDS, in column order) - the control nodes of the two swing curves and the
        stance curve, default and target tip, stride vector, swing clearance, the iteration of the running swing or stance period and its
        length, ``path``: the walker tip after 1 .. ``horizon`` (at most 16) further cycles if the curves stayed as they are, and the steppers'
        walk plane.  ``plan_columns(fields, legs, horizon)`` names the columns; positions are in the frame of the walker tip.  ``pad`` stands
        where a robot has no such leg, a leg is not stepping, a curve does not belong to the leg's period or a path sample lies beyond its end.
        Nothing is written into the engine.  Returns a host array - or, with out = a 2-D float32 / float64 device array
        (``__cuda_array_interface__``; a view of some columns of a wider array will do) of count rows and at least D columns, fills its first D
        columns on the engine's stream without a host wait and returns None: dtype then is the array's."""
        count = self.n - first if count is None else count
        legs = self.legs if legs is None else legs
        if out is not None:
            a, spec, _ = _row_pass(self, "step_plan: out", out, _ROWS, lambda dt, stride: plan_spec(fields, legs, horizon, dt, stride, pad), (int(count),))
            _check(self.L.shc_engine_get_step_plan(self.h, int(first), int(count), C.byref(spec), a.pointer, 1), "get_step_plan")
            return None
        spec = plan_spec(fields, legs, horizon, dtype, 0, pad)
        plan = np.zeros((max(int(count), 0), _row_width(self, spec, "get_step_plan")), dtype=np.dtype(dtype))
        _check(self.L.shc_engine_get_step_plan(self.h, int(first), int(count), C.byref(spec), plan.ctypes.data_as(C.c_void_p), 0), "get_step_plan")
        return plan

    def frame_transforms(self, first: int = 0, count: Optional[int] = None, frame="base_link", legs: bool = True, body: bool = True,
                         out_legs: Optional[int] = None, out_body: Optional[int] = None):
        """publishFrameTransforms for instances [first, first + count) in one device pass (shc_engine_get_frame_transforms): (legs, body),
        structured arrays of shape (count, legs) with the fields of LegFrames (LEG_FRAMES_DTYPE: joint (5, 7), tip (7,)) and of shape (count,)
        with the fields of BodyFrames (BODY_FRAMES_DTYPE); the one not asked for (legs / body = False) is None.  frame: "base_link" (what the
        node broadcasts) or "odom_ideal" (every joint / tip frame composed with odom_to_base_link), or the SHC_FRAME_* integer.  out_legs /
        out_body = device pointers (integers, 16-byte aligned, room for count * legs records of 336 B / count records of 160 B): the records
        are written there, ordered on the engine's stream without a host wait; returns None."""
        count = self.n - first if count is None else count
        frame = FRAME_IDS[frame] if isinstance(frame, str) else int(frame)
        fn = self.L.shc_engine_get_frame_transforms
        if out_legs is not None or out_body is not None:
            ptr = lambda p: None if p is None else C.c_void_p(int(p))
            _check(fn(self.h, int(first), int(count), frame, ptr(out_legs), ptr(out_body), 1), "get_frame_transforms")
            return None
        lf = np.zeros((max(int(count), 0), self.legs), dtype=LEG_FRAMES_DTYPE) if legs else None
        bf = np.zeros(max(int(count), 0), dtype=BODY_FRAMES_DTYPE) if body else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _check(fn(self.h, int(first), int(count), frame, ptr(lf), ptr(bf), 0), "get_frame_transforms")
        return lf, bf

    def get_state(self, first: int = 0, count: Optional[int] = None):
        """Full controller state of instances [first, first + count) as a ctypes array of InstanceState."""
        count = self.n - first if count is None else count
        arr = (InstanceState * count)()
        _check(self.L.shc_engine_get_state(self.h, first, count, arr), "get_state")
        return arr

    def set_state(self, states, first: int = 0):
        """Restore / inject the state of instances [first, first + len(states))."""
        _check(self.L.shc_engine_set_state(self.h, first, len(states), states), "set_state")

    def get_aux_state(self, first: int = 0, count: Optional[int] = None) -> bytes:
        """The rest of a complete checkpoint (manual legs, external targets, sequence / planner state, ...): opaque blobs."""
        count = self.n - first if count is None else count
        buf = C.create_string_buffer(int(self.L.shc_engine_aux_state_bytes(self.h)) * count)
        _check(self.L.shc_engine_get_aux_state(self.h, first, count, buf), "get_aux_state")
        return buf.raw

    def set_aux_state(self, blobs: bytes, first: int = 0):
        per = int(self.L.shc_engine_aux_state_bytes(self.h))
        assert len(blobs) % per == 0
        _check(self.L.shc_engine_set_aux_state(self.h, first, len(blobs) // per, C.c_char_p(blobs)), "set_aux_state")

    def checkpoint(self) -> Checkpoint:
        """A device-resident checkpoint of every robot's state as of now (on the engine's stream)."""
        return Checkpoint(self)

    def restore(self, ck: Checkpoint, source=None):
        """Robot i <- the checkpoint's robot ``source[i]``; an entry < 0 leaves robot i alone.  ``source``: a host int64 array of length n (an entry
        >= n raises), an object with ``__cuda_array_interface__`` (a contiguous int64 array of length n on the engine's device, e.g. a torch tensor:
        read on the engine's stream without a host wait - the writes to it must be ordered before this call on that stream; an entry >= n leaves its
        robot alone), or None for every robot.  Reset from a mask: ``torch.where(done, torch.arange(n), -1)``."""
        a = None if source is None else arrays.read(source, "restore: source", _SOURCE_MAP, (self.n,))
        _check(self.L.shc_engine_restore_instances(self.h, ck.h, a and a.pointer, 1 if a and a.on_device else 0), "restore_instances")

    def scan_health(self, select: int = 0, near_limit_proximity: float = 0.0, tip_deviation: float = 0.0, first: int = 0, count: Optional[int] = None,
                    out_health=None, out_restore_map=None, out_selected=None, out_n_selected=None):
        """The reference's IK warnings per robot in one device pass (shc_engine_scan_health): for instances [first, first + count) a record each
        (ROBOT_HEALTH_DTYPE: min_limit_proximity, max_tip_deviation, max_speed_ratio, flags = HEALTH_* bits, leg_masks), and the robots whose
        flags meet ``select``.  Without out_* arguments: (records, ascending int64 array of the selected instance ids), on the host.  With any
        out_*: the device form - out_health (count records of 32 B, 16-byte aligned), out_restore_map (int64[n]: i for a selected robot of the
        range, -1 elsewhere - what ``restore`` takes), out_selected (int64[count]; entries past the count stay as they are) and out_n_selected
        (int64[1]) are device pointers (integers) or objects with ``__cuda_array_interface__``; they are written on the engine's stream without
        a host wait; returns None."""
        count = self.n - first if count is None else count
        crit = HealthCriteria(int(select), 0, float(near_limit_proximity), float(tip_deviation))
        fn = self.L.shc_engine_scan_health
        if any(o is not None for o in (out_health, out_restore_map, out_selected, out_n_selected)):
            rows = max(int(count), 0)
            _check(fn(self.h, int(first), int(count), C.byref(crit), _pointer(out_health, "out_health", _OUT_RECORDS, nbytes=rows * 32),
                      _pointer(out_restore_map, "out_restore_map", _OUT_INT64, nbytes=self.n * 8),
                      _pointer(out_selected, "out_selected", _OUT_INT64, nbytes=rows * 8),
                      _pointer(out_n_selected, "out_n_selected", _OUT_INT64, nbytes=8), 1), "scan_health")
            return None
        health = np.zeros(max(int(count), 0), dtype=ROBOT_HEALTH_DTYPE)
        selected = np.zeros(max(int(count), 0), dtype=np.int64)
        n_sel = C.c_int64(0)
        _check(fn(self.h, int(first), int(count), C.byref(crit), health.ctypes.data_as(C.c_void_p), None, selected.ctypes.data_as(C.c_void_p),
                  C.cast(C.byref(n_sel), C.c_void_p), 0), "scan_health")
        return health, selected[:n_sel.value].copy()

    # -- per-leg Leg methods (model.h:448-492), batched: instances [first, first + count), leg = -1 for every leg
    def _rows(self, first, count, leg):
        count = self.n - first if count is None else count
        return count, count * (self.legs if leg < 0 else 1)

    def leg_set_desired_tip_pose(self, tip_pose=None, apply_delta=True, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        a = _host(tip_pose)
        assert a is None or a.size == rows * 7
        _check(self.L.shc_leg_set_desired_tip_pose(self.h, first, count, leg, _p(a), int(apply_delta), 0), "leg_set_desired_tip_pose")

    def leg_solve_ik(self, delta, solve_rotation=False, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        a = _host(delta)
        assert a.size == rows * 6
        out = np.zeros((rows, self.dof))
        _check(self.L.shc_leg_solve_ik(self.h, first, count, leg, _p(a), int(solve_rotation), _p(out), 0), "leg_solve_ik")
        return out

    def leg_update_joint_positions(self, joint_delta, simulation=False, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        a = _host(joint_delta)
        assert a.size == rows * self.dof
        out = np.zeros(rows)
        _check(self.L.shc_leg_update_joint_positions(self.h, first, count, leg, _p(a), int(simulation), _p(out), 0), "leg_update_joint_positions")
        return out

    def leg_apply_ik(self, simulation=False, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        out = np.zeros(rows)
        _check(self.L.shc_leg_apply_ik(self.h, first, count, leg, int(simulation), _p(out), 0), "leg_apply_ik")
        return out

    def leg_apply_fk(self, joint_position=None, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        a = _host(joint_position)
        out = np.zeros((rows, 7))
        _check(self.L.shc_leg_apply_fk(self.h, first, count, leg, _p(a), _p(out), 0), "leg_apply_fk")
        return out

    # -- ROS message payloads
    def set_joint_states_msg(self, position=None, velocity=None, effort=None):
        a, b, c = _host(position), _host(velocity), _host(effort)
        _check(self.L.shc_engine_set_joint_states_msg(self.h, _p(a), _p(b), _p(c), 0), "set_joint_states_msg")

    def set_tip_states_msg(self, wrench_force=None, step_plane=None):
        a, b = _host(wrench_force), _host(step_plane)
        _check(self.L.shc_engine_set_tip_states_msg(self.h, _p(a), _p(b), 0), "set_tip_states_msg")

    # -- start-up / shut-down sequences (PoseController::executeSequence, stepToNewStance)
    def begin_sequence_startup(self, joint_positions=None, per_instance=False):
        a = _host(joint_positions)
        _check(self.L.shc_engine_begin_sequence_startup(self.h, _p(a), 1 if per_instance else 0), "begin_sequence_startup")

    def execute_sequence(self, sequence):
        """One executeSequence call per instance; returns the progress rows (-1 generating, 0..99, 100 complete)."""
        pr = np.zeros(self.n, dtype=np.int32)
        _check(self.L.shc_engine_execute_sequence(self.h, int(sequence), _p(pr)), "execute_sequence")
        return pr

    def finish_sequence_startup(self):
        _check(self.L.shc_engine_finish_sequence_startup(self.h), "finish_sequence_startup")

    # -- manual leg manipulation (legStateToggle, updateManual)
    def toggle_leg_state(self, leg_selection):
        """One legStateToggle call per instance (leg_selection[i] = -1: no request).  Returns the result rows."""
        sel = np.ascontiguousarray(leg_selection, dtype=np.int32)
        res = np.zeros(self.n, dtype=np.int32)
        _check(self.L.shc_engine_toggle_leg_state(self.h, _p(sel), _p(res)), "toggle_leg_state")
        return res

    def set_manual_inputs(self, primary_leg=None, primary_velocity=None, primary_position=None, secondary_leg=None, secondary_velocity=None,
                          secondary_position=None):
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        a = [i32(primary_leg), _host(primary_velocity), _host(primary_position), i32(secondary_leg), _host(secondary_velocity), _host(secondary_position)]
        _check(self.L.shc_engine_set_manual_inputs(self.h, *[_p(x) for x in a]), "set_manual_inputs")

    def leg_manipulation_state(self):
        out = np.zeros((self.n, self.legs), dtype=np.int32)
        _check(self.L.shc_engine_get_leg_manipulation_state(self.h, _p(out)), "get_leg_manipulation_state")
        return out

    # -- planner mode (StateController::executePlan)
    def set_planner_mode(self, on):
        _check(self.L.shc_engine_set_planner_mode(self.h, int(bool(on))), "set_planner_mode")

    def set_target_configuration(self, configuration, first=0):
        """targetConfigurationCallback: rows [count][legs][dof]; NaN in a leg's first joint = leg not named."""
        a = np.ascontiguousarray(configuration, dtype=np.float64).reshape(-1, self.legs * self.dof)
        _check(self.L.shc_engine_set_target_configuration(self.h, first, a.shape[0], _p(a)), "set_target_configuration")

    def set_target_body_pose(self, pose, first=0):
        a = np.ascontiguousarray(pose, dtype=np.float64).reshape(-1, 7)
        _check(self.L.shc_engine_set_target_body_pose(self.h, first, a.shape[0], _p(a)), "set_target_body_pose")

    def execute_plan(self):
        """One StateController::loop() in planner mode for every instance -> (progress [n], plan_step [n])."""
        progress, step = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        _check(self.L.shc_engine_execute_plan(self.h, _p(progress), _p(step)), "execute_plan")
        return progress, step

    def pack_legs(self, packed_positions, time_to_pack, unpack=False):
        """One PoseController::packLegs / unpackLegs call; packed_positions [n_pack_steps][legs][dof]."""
        a = np.ascontiguousarray(packed_positions, dtype=np.float64)
        steps = a.size // (self.legs * self.dof)
        pr = C.c_int32(0)
        f = self.L.shc_engine_unpack_legs if unpack else self.L.shc_engine_pack_legs
        _check(f(self.h, _p(a), steps, float(time_to_pack), C.byref(pr)), "pack_legs")
        return pr.value

    def step_to_new_stance(self):
        pr = np.zeros(self.n, dtype=np.int32)
        _check(self.L.shc_engine_step_to_new_stance(self.h, _p(pr)), "step_to_new_stance")
        return pr

    # -- external targets / defaults of rough terrain mode (targetTipPoseCallback, generateExternalTargetTransforms)
    def set_external_target(self, rows, which=0, first=0, count=None, leg=-1):
        """rows: ctypes array of ExternalTarget, one per selected (instance, leg).  Returns how many requests were ignored
        because their robot was STOPPED."""
        count, n_rows = self._rows(first, count, leg)
        assert len(rows) == n_rows
        ignored = C.c_int64(0)
        _check(self.L.shc_engine_set_external_target(self.h, which, first, count, leg, rows, C.byref(ignored)), "set_external_target")
        return ignored.value

    def set_external_transform(self, transform, which=0, first=0, count=None, leg=-1):
        count, n_rows = self._rows(first, count, leg)
        a = _host(transform)
        assert a.size == n_rows * 7
        _check(self.L.shc_engine_set_external_transform(self.h, which, first, count, leg, _p(a)), "set_external_transform")

    def get_external_target(self, which=0, first=0, count=None, leg=-1):
        count, n_rows = self._rows(first, count, leg)
        rows = (ExternalTarget * n_rows)()
        _check(self.L.shc_engine_get_external_target(self.h, which, first, count, leg, rows), "get_external_target")
        return rows

    def set_footholds(self, rows, fields, which=0, mode="request", ignored=None, legs: Optional[int] = None):
        """The requests of every leg of every instance from one 2-D array of n rows in one device pass (shc_engine_set_footholds): fields are
        names of FH_FIELDS in column order, ``foothold_columns(fields, legs)`` names the columns.  Per leg the engine is left as
        ``set_external_target`` (mode "request": "defined" > 0 requests, 0 withdraws, negative or NaN leaves the leg alone; members not named
        take the callback's values) or ``set_external_transform`` (mode "refresh_transform") leaves it.  rows: a float32 / float64 device array
        (``__cuda_array_interface__``; a view of some columns of a wider array will do), read on the engine's stream without a host wait and
        never written; the dropped rows are then ADDED to ``ignored``, a one-element int64 device array the caller zeroes (or None), and None
        is returned.  Or a numpy array, which is copied to the device and waited for: the number of dropped rows is returned.  legs (default:
        the engine's) may be larger than the robot's: the columns of legs it lacks are ignored."""
        legs = self.legs if legs is None else legs
        a, spec, _ = _row_pass(self, "set_footholds: rows", rows, _ROWS_VIEW,
                               lambda dt, stride: foothold_spec(fields, legs, dt, which, mode, stride), (self.n,))
        if a.on_device:
            _check(self.L.shc_engine_set_footholds(self.h, C.byref(spec), a.pointer, 1, _pointer(ignored, "set_footholds: ignored", _ONE_INT64, nbytes=8)),
                   "set_footholds")
            return None
        if ignored is not None:
            raise ValueError("set_footholds: host rows return the count; ignored goes with device rows")
        count = C.c_int64(0)
        _check(self.L.shc_engine_set_footholds(self.h, C.byref(spec), a.pointer, 0, C.cast(C.byref(count), C.c_void_p)), "set_footholds")
        return count.value

    def footholds(self, out=None, fields=FH_FIELD_NAMES, which=0, pad: float = 0.0, dtype="float64", legs: Optional[int] = None):
        """The requests as the steppers / posers hold them now, every leg of every instance as one (n, F) array in one device pass
        (shc_engine_get_footholds): per leg the named columns hold what ``get_external_target(which)`` returns, "defined" and
        "frame_is_odom_ideal" as 0 / 1; the columns of legs the robot lacks (legs > the engine's) hold ``pad``.  Returns a host array of
        ``dtype`` - or, with out = a 2-D float32 / float64 device array of n rows and at least F columns, fills its first F columns on the
        engine's stream without a host wait and returns None (out may also be a numpy array, filled and waited for)."""
        legs = self.legs if legs is None else legs
        if out is None:
            host = np.zeros((self.n, _row_width(self, foothold_spec(fields, legs, dtype, which), "get_footholds")), dtype=np.dtype(dtype))
            self.footholds(host, fields, which, pad, legs=legs)
            return host
        a, spec, _ = _row_pass(self, "footholds: out", out, _ROWS_VIEW,
                               lambda dt, stride: foothold_spec(fields, legs, dt, which, "request", stride, pad), (self.n,))
        _check(self.L.shc_engine_get_footholds(self.h, C.byref(spec), a.pointer, a.on_device), "get_footholds")
        return None

    def probe_reach(self, targets, steps: int, fields=("fraction", "limit_proximity"), out=None, first: int = 0, count: Optional[int] = None,
                    pad: float = float("nan"), legs: Optional[int] = None, dof: Optional[int] = None):
        """Which candidate tip targets every leg can reach from its present joints, in one device pass that writes nothing into the engine
        (shc_engine_probe_reach).  targets: a float32 / float64 DEVICE array (count, C, legs, 3) - for each of the instances
        [first, first + count) C candidate tip positions per leg in the robot frame (the frame of ``leg_set_desired_tip_pose`` and the
        "model_tip" observation); a NaN leaves that leg of that candidate out.  Per (instance, candidate, leg) the tip walks the straight line
        from where it is to the target in ``steps`` steps of ``leg_set_desired_tip_pose`` + ``leg_apply_ik(simulation=True)`` and stops at the
        first step that returns 0.  Returns the DEVICE array (count, C, D) of targets' element type - ``out`` when given, else a new torch
        tensor - with ``reach_columns(fields, legs, dof)`` naming the D columns of a candidate's block: "fraction" (steps that succeeded /
        steps), "limit_proximity" (what the last executed step returned), "tip" (3: where the tip ended), "q" (dof: the joints there);
        ``pad`` where a leg was left out or the row geometry (legs, dof) is larger than the robot.  Both arrays may be views whose robots lie
        further apart (``big[:, :C * D].unflatten(1, (C, D))``).  On the engine's stream, no host wait; a numpy array is a TypeError (device
        arrays only)."""
        return _probe_reach(self, "shc_engine_probe_reach", targets, steps, fields, out, first, count, pad, legs, dof)

    def joint_commands(self):
        """(position, velocity, effort, position_command) of publishDesiredJointState, each [n][legs * dof]."""
        out = [np.zeros((self.n, self.legs * self.dof)) for _ in range(4)]
        _check(self.L.shc_engine_get_joint_commands(self.h, *[_p(o) for o in out], 0), "get_joint_commands")
        return out

    # -- sequences
    def leg_step_to_position(self, target_tip_pose, target_pose, lift_height, time_to_step, apply_delta=True, first=0, count=None, leg=-1):
        """One LegPoser::stepToPosition iteration; returns (poser tip pose rows [.., 7], progress rows)."""
        count, rows = self._rows(first, count, leg)
        a, b = _host(target_tip_pose), _host(target_pose)
        assert (a is None or a.size == rows * 7) and b.size == count * 7
        out, prog = np.zeros((rows, 7)), np.zeros(rows, dtype=np.int32)
        _check(self.L.shc_leg_step_to_position(self.h, first, count, leg, _p(a), _p(b), float(lift_height), float(time_to_step), int(apply_delta),
                                               _p(out), _p(prog), 0), "leg_step_to_position")
        return out, prog

    def leg_transition_configuration(self, desired_configuration, transition_time, first=0, count=None, leg=-1):
        count, rows = self._rows(first, count, leg)
        a = _host(desired_configuration)
        assert a.size == rows * self.dof
        prog = np.zeros(rows, dtype=np.int32)
        _check(self.L.shc_leg_transition_configuration(self.h, first, count, leg, _p(a), float(transition_time), _p(prog), 0),
               "leg_transition_configuration")
        return prog

    def begin_direct_startup(self):
        _check(self.L.shc_engine_begin_direct_startup(self.h), "begin_direct_startup")

    def direct_startup(self) -> int:
        p = C.c_int32(0)
        _check(self.L.shc_engine_direct_startup(self.h, C.byref(p)), "direct_startup")
        return int(p.value)

    def odometry(self):
        """WalkController::getOdometryIdeal per instance: [n][7] (x, y, z, qw, qx, qy, qz)."""
        pose = np.zeros((self.n, 7))
        _check(self.L.shc_engine_get_odometry(self.h, _p(pose), 0), "get_odometry")
        return pose

    def virtual_stiffness(self):
        """Leg::getVirtualStiffness per leg (AdmittanceController::updateStiffness): [n][legs]."""
        k = np.zeros((self.n, self.legs))
        _check(self.L.shc_engine_get_virtual_stiffness(self.h, _p(k), 0), "get_virtual_stiffness")
        return k
