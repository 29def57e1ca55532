"""Mixed-morphology / multi-device batches: thin ctypes view of the C ABI's shc_fleet_* entry points (include/shc_batch.h).

The binning (one engine and one HIP stream per (morphology bin, device)), the contiguous sharding over devices and the
device-to-device all-gather of the joint buffer live in the library (csrc/shc_fleet.hpp); this class only converts numpy
arrays.  Inputs arrive and outputs leave indexed by the caller's instance id, whatever the interleaving pattern - as host
arrays, or (set_inputs / outputs, csrc/shc_fleet_io.hpp; step_k / step_k_joints, csrc/shc_fleet_step_k.hpp: K cycles per launch) as device
arrays that never cross the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import arrays as _arrays, engine as _engine
from .params import Params


class FleetCheckpoint:
    """The state of every robot of a fleet, kept in device memory part by part (shc_fleet_checkpoint_create): what ``MixedFleet.restore`` and
    ``MixedFleet.scan_and_restore`` reset or clone robots from.  A context manager; closed with its fleet (``close()`` afterwards is a no-op
    for the caller).  Mirrors ``engine.Checkpoint``."""

    def __init__(self, fleet: "MixedFleet"):
        self.fleet, self.L, self.h = fleet, fleet.L, None
        h = C.c_void_p()
        _engine._check(self.L.shc_fleet_checkpoint_create(fleet.h, C.byref(h)), "shc_fleet_checkpoint_create")
        self.h = h
        fleet._checkpoints.append(self)

    def update(self):
        """Capture every part's state again into the same device storage: copies on each part's stream, no host wait."""
        _engine._check(self.L.shc_fleet_checkpoint_update(self.fleet.h, self.h), "shc_fleet_checkpoint_update")

    @property
    def nbytes(self) -> int:
        return int(self.L.shc_fleet_checkpoint_bytes(self.h)) if self.h else 0

    def close(self):
        if getattr(self, "h", None):
            self.L.shc_fleet_checkpoint_destroy(self.h)
            self.h = None
            if self in self.fleet._checkpoints:
                self.fleet._checkpoints.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixedFleet:
    def __init__(self, morphologies: Sequence[Params], morph_id, devices: Sequence[int] = (0,)):
        """morphologies[k] describes bin k; morph_id[i] in [0, len(morphologies)) assigns instance i to a bin; every bin is
        sharded over `devices` (repeating a device id gives several shards on that device)."""
        self.L = _engine.lib()
        self._checkpoints = []
        if self.L.shc_device_count() < 1:
            raise _engine.ShcError("no HIP device visible: the batched engine has no CPU fallback")
        self.morph_id = np.ascontiguousarray(morph_id, dtype=np.int32)
        self.n = len(self.morph_id)
        self.params = list(morphologies)
        arr = (Params * len(self.params))(*self.params)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        _engine._check(self.L.shc_fleet_create(arr, len(self.params), self.morph_id.ctypes.data_as(C.c_void_p), self.n,
                                               dev.ctypes.data_as(C.c_void_p), len(dev), C.byref(h)), "shc_fleet_create")
        self.h, self.n_devices = h, len(dev)
        a, b = C.c_int(), C.c_int()
        _engine._check(self.L.shc_fleet_shape(self.h, C.byref(a), C.byref(b)), "shc_fleet_shape")
        self.max_legs, self.max_dof = a.value, b.value

    def close(self):
        for ck in list(getattr(self, "_checkpoints", [])):
            ck.close()
        if getattr(self, "h", None):
            self.L.shc_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parts(self):
        """[(engine handle, morphology, device, instance ids)] of every (bin, device) part."""
        out = []
        for k in range(self.L.shc_fleet_part_count(self.h)):
            e, m, d, n = C.c_void_p(), C.c_int(), C.c_int(), C.c_int64()
            _engine._check(self.L.shc_fleet_part(self.h, k, C.byref(e), C.byref(m), C.byref(d), C.byref(n)), "shc_fleet_part")
            ids = np.zeros(n.value, dtype=np.int64)
            _engine._check(self.L.shc_fleet_part_instances(self.h, k, ids.ctypes.data_as(C.c_void_p)), "shc_fleet_part_instances")
            out.append((e.value, m.value, d.value, ids))
        return out

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def set_velocity(self, linear_xy=None, angular=None):
        """linear_xy [n][2], angular [n]; None holds that input."""
        a, b = _engine._host(linear_xy), _engine._host(angular)
        _engine._check(self.L.shc_fleet_set_velocity(self.h, self._p(a), self._p(b)), "shc_fleet_set_velocity")

    def set_imu(self, orientation_wxyz=None, angular_velocity=None):
        """orientation_wxyz [n][4] (normalised on entry), angular_velocity [n][3]; None holds that input."""
        a, b = _engine._host(orientation_wxyz), _engine._host(angular_velocity)
        assert (a is None or a.shape == (self.n, 4)) and (b is None or b.shape == (self.n, 3))
        _engine._check(self.L.shc_fleet_set_imu(self.h, self._p(a), self._p(b)), "shc_fleet_set_imu")

    def set_pose_input(self, translation_velocity=None, rotation_velocity=None):
        """Manual posing velocities, [n][3] each; None holds that input."""
        a, b = _engine._host(translation_velocity), _engine._host(rotation_velocity)
        assert (a is None or a.shape == (self.n, 3)) and (b is None or b.shape == (self.n, 3))
        _engine._check(self.L.shc_fleet_set_pose_input(self.h, self._p(a), self._p(b)), "shc_fleet_set_pose_input")

    def set_tip_force(self, force_padded):
        """force_padded [n][max_legs][3]; entries beyond a robot's legs are ignored."""
        a = np.ascontiguousarray(force_padded, dtype=np.float64)
        assert a.shape == (self.n, self.max_legs, 3)
        _engine._check(self.L.shc_fleet_set_tip_force(self.h, self._p(a)), "shc_fleet_set_tip_force")

    def set_joint_effort(self, effort_padded):
        """effort_padded [n][max_legs][max_dof]; entries beyond a bin's (legs, dof) are ignored."""
        a = np.ascontiguousarray(effort_padded, dtype=np.float64)
        assert a.shape == (self.n, self.max_legs, self.max_dof)
        _engine._check(self.L.shc_fleet_set_joint_effort(self.h, self._p(a)), "shc_fleet_set_joint_effort")

    def step(self, n_cycles: int = 1):
        _engine._check(self.L.shc_fleet_step(self.h, int(n_cycles)), "shc_fleet_step")

    def synchronize(self):
        _engine._check(self.L.shc_fleet_synchronize(self.h), "shc_fleet_synchronize")

    def joints(self):
        q = np.zeros((self.n, self.max_legs, self.max_dof))
        qd = np.zeros_like(q)
        _engine._check(self.L.shc_fleet_get_joint_state(self.h, self._p(q), self._p(qd)), "shc_fleet_get_joint_state")
        return q, qd

    def walk_state(self):
        ws = np.zeros(self.n, dtype=np.int32)
        _engine._check(self.L.shc_fleet_get_walk_state(self.h, self._p(ws)), "shc_fleet_get_walk_state")
        return ws

    def leg_state_msgs(self):
        """publishLegState of every robot in the caller's instance order: a structured array of shape (n, max_legs) with the fields of
        LegStateMsg; the records of legs a robot does not have are all zero."""
        msgs = np.zeros((self.n, self.max_legs), dtype=_engine.LEG_STATE_MSG_DTYPE)
        _engine._check(self.L.shc_fleet_get_leg_state_msgs(self.h, self._p(msgs)), "shc_fleet_get_leg_state_msgs")
        return msgs

    def frame_transforms(self, frame="base_link", legs: bool = True, body: bool = True):
        """publishFrameTransforms of every robot in the caller's instance order: (legs, body), structured arrays of shape (n, max_legs) with
        the fields of LegFrames - the records of legs a robot does not have all zero - and of shape (n,) with the fields of BodyFrames; the one
        not asked for is None.  frame: "base_link" or "odom_ideal" (BatchEngine.frame_transforms)."""
        frame = _engine.FRAME_IDS[frame] if isinstance(frame, str) else int(frame)
        lf = np.zeros((self.n, self.max_legs), dtype=_engine.LEG_FRAMES_DTYPE) if legs else None
        bf = np.zeros(self.n, dtype=_engine.BODY_FRAMES_DTYPE) if body else None
        _engine._check(self.L.shc_fleet_get_frame_transforms(self.h, frame, None if lf is None else self._p(lf), None if bf is None else self._p(bf)),
                       "shc_fleet_get_frame_transforms")
        return lf, bf

    def scan_health(self, select: int = 0, near_limit_proximity: float = 0.0, tip_deviation: float = 0.0):
        """BatchEngine.scan_health's records for every robot in the caller's instance order (ROBOT_HEALTH_DTYPE, shape (n,)).  Records only:
        ``scan_and_restore`` resets the selected robots in the same pass; selected lists are per engine (parts())."""
        crit = _engine.HealthCriteria(int(select), 0, float(near_limit_proximity), float(tip_deviation))
        health = np.zeros(self.n, dtype=_engine.ROBOT_HEALTH_DTYPE)
        _engine._check(self.L.shc_fleet_scan_health(self.h, C.byref(crit), self._p(health)), "shc_fleet_scan_health")
        return health

    # -- device I/O: the setters and getters above with device arrays (shc_fleet_set_inputs_device / shc_fleet_get_outputs_device)
    def _input_shapes(self):
        n = self.n
        return {"linear_xy": (n, 2), "angular": (n,), "imu_orientation_wxyz": (n, 4), "imu_angular_velocity": (n, 3), "pose_translation_velocity": (n, 3),
                "pose_rotation_velocity": (n, 3), "tip_force": (n, self.max_legs, 3), "joint_effort": (n, self.max_legs, self.max_dof)}

    def set_inputs(self, **arrays):
        """The five setters in one call, from contiguous float64 DEVICE arrays in the caller's instance order (objects with
        ``__cuda_array_interface__``, e.g. torch tensors): linear_xy (n, 2), angular (n,), imu_orientation_wxyz (n, 4), imu_angular_velocity (n, 3),
        pose_translation_velocity (n, 3), pose_rotation_velocity (n, 3), tip_force (n, max_legs, 3), joint_effort (n, max_legs, max_dof).  An
        argument left out (or None) holds that input.  No host wait: the parts read the arrays on streams of their own - ``order_after(stream)``
        first when a stream is still writing them, or finish the writes (``stream.synchronize()``), and keep them untouched until the parts have
        read them (``order_before`` + stream order, or ``synchronize()``)."""
        shapes, st = self._input_shapes(), _engine.FleetInputs()
        for name, a in arrays.items():
            if name not in shapes:
                raise TypeError(f"set_inputs: unknown input {name!r} (one of {', '.join(shapes)})")
            if a is not None:
                setattr(st, name, _arrays.read(a, name, _engine._FLOAT64, shapes[name]).pointer)
        _engine._check(self.L.shc_fleet_set_inputs_device(self.h, C.byref(st)), "shc_fleet_set_inputs_device")

    def outputs(self, q=None, qd=None, walk_state=None, leg_state_msgs=None, leg_frames=None, body_frames=None, health=None, frame="base_link",
                select: int = 0, near_limit_proximity: float = 0.0, tip_deviation: float = 0.0):
        """joints(), walk_state(), leg_state_msgs(), frame_transforms(frame) and scan_health(select, ...) into DEVICE buffers of the caller's, in
        the caller's instance order and byte for byte what those return (NaN padding of q / qd, all-zero records of missing legs): q, qd float64
        (n, max_legs, max_dof); walk_state int32 (n,); leg_state_msgs, leg_frames, body_frames, health: contiguous buffers of any element type
        (uint8, float64, ...) with n * max_legs * 512, n * max_legs * 336, n * 160 and n * 32 bytes, 16-byte aligned.  Only the buffers given are
        written, every entry of them; at least one must be given.  No host wait: complete after ``synchronize()``, or for work queued on a stream
        after ``order_before(stream)``."""
        n, row = self.n, (self.n, self.max_legs, self.max_dof)
        st = _engine.FleetOutputs()
        st.q, st.qd = _engine._pointer(q, "q", _engine._FLOAT64, row), _engine._pointer(qd, "qd", _engine._FLOAT64, row)
        st.walk_state = _engine._pointer(walk_state, "walk_state", _engine._INT32, (n,))
        for name, buf, nbytes in (("leg_state_msgs", leg_state_msgs, n * self.max_legs * _engine.LEG_STATE_MSG_DTYPE.itemsize),
                                  ("leg_frames", leg_frames, n * self.max_legs * _engine.LEG_FRAMES_DTYPE.itemsize),
                                  ("body_frames", body_frames, n * _engine.BODY_FRAMES_DTYPE.itemsize),
                                  ("health", health, n * _engine.ROBOT_HEALTH_DTYPE.itemsize)):
            setattr(st, name, _engine._pointer(buf, name, _engine._RECORDS, nbytes=nbytes))
        st.frame = _engine.FRAME_IDS[frame] if isinstance(frame, str) else int(frame)
        crit = _engine.HealthCriteria(int(select), 0, float(near_limit_proximity), float(tip_deviation))
        st.criteria = C.pointer(crit)
        _engine._check(self.L.shc_fleet_get_outputs_device(self.h, C.byref(st)), "shc_fleet_get_outputs_device")

    def observations(self, out, fields, pad: float = 0.0):
        """Chosen fields (names of ``engine.OBS_FIELDS``, in column order) of every robot into the DEVICE array ``out``, row i = the caller's
        instance i, in one kernel per part with no staging (shc_fleet_get_observations_device).  out: any 2-D float32 / float64 object with
        ``__cuda_array_interface__`` of n rows and at least D columns whose rows are contiguous - a view ``big[:, 5:5 + D]`` of a wider torch tensor
        will do: element type, row stride and the offset pointer are taken from it, and only its first D columns are written.
        ``engine.observation_columns(fields, max_legs, max_dof)`` names the columns; every value is the double the matching member of
        ``outputs()`` / ``joints()`` holds, cast to out's type, and ``pad`` where a morphology has no such leg or joint.  No host wait: complete
        after ``synchronize()``, or for work queued on a stream after ``order_before(stream)``."""
        a, spec, _ = _engine._row_pass(self, "observations: out", out, _engine._ROWS,
                                       lambda dt, stride: _engine.obs_spec(fields, self.max_legs, self.max_dof, dt, stride, pad), (self.n,))
        _engine._check(self.L.shc_fleet_get_observations_device(self.h, C.byref(spec), a.pointer), "shc_fleet_get_observations_device")

    def set_actions(self, actions, fields):
        """Chosen input groups (names of ``engine.ACT_FIELDS``, in column order) of every robot from the DEVICE array ``actions``, row i = the
        caller's instance i, in one kernel per part with no staging (shc_fleet_set_actions_device).  actions: any 2-D float32 / float64 object with
        ``__cuda_array_interface__`` of n rows and at least A columns whose rows are contiguous - a view ``big[:, 5:5 + A]`` of a wider torch tensor
        will do; it is never written.  ``engine.action_columns(fields, max_legs, max_dof)`` names the columns; the fleet is left as ``set_inputs``
        leaves it when given the columns as float64 arrays, groups not named are held, columns of legs and joints a morphology lacks are ignored.
        No host wait, and the stream rules of ``set_inputs``."""
        a, spec, _ = _engine._row_pass(self, "set_actions: actions", actions, _engine._ROWS,
                                       lambda dt, stride: _engine.act_spec(fields, self.max_legs, self.max_dof, dt, stride), (self.n,))
        _engine._check(self.L.shc_fleet_set_actions_device(self.h, C.byref(spec), a.pointer), "shc_fleet_set_actions_device")

    def set_footholds(self, rows, fields, which=0, mode="request", ignored=None):
        """The tip-target requests of every leg of every robot from one 2-D array, row i = the caller's instance i
        (shc_fleet_set_footholds_device): ``BatchEngine.set_footholds`` for a fleet, with the row geometry ``max_legs`` -
        ``engine.foothold_columns(fields, max_legs)`` names the columns, those of legs a morphology lacks are ignored.  rows: a 2-D float32 /
        float64 device array (``__cuda_array_interface__``; a view of some columns of a wider one will do): one kernel per part on the part's
        stream, no staging, no host wait, the stream rules of ``set_inputs``; the dropped rows of every part are ADDED to ``ignored``, a
        one-element int64 device array the caller zeroes (or None); returns None.  Or a numpy array: every part takes its rows through its
        engine's host form, and the number of dropped rows is returned."""
        a, spec, _ = _engine._row_pass(self, "set_footholds: rows", rows, _engine._ROWS_VIEW,
                                       lambda dt, stride: _engine.foothold_spec(fields, self.max_legs, dt, which, mode, stride), (self.n,))
        if a.on_device:
            _engine._check(self.L.shc_fleet_set_footholds_device(self.h, C.byref(spec), a.pointer,
                                                                 _engine._pointer(ignored, "set_footholds: ignored", _engine._ONE_INT64, nbytes=8)),
                           "shc_fleet_set_footholds_device")
            return None
        width = int(self.L.shc_foothold_width(C.byref(spec)))
        if ignored is not None:
            raise ValueError("set_footholds: host rows return the count; ignored goes with device rows")
        count, spec.row_stride = C.c_int64(0), 0
        for e, _m, _d, ids in self.parts():
            part = np.ascontiguousarray(rows[ids, :max(width, 0)])
            _engine._check(self.L.shc_engine_set_footholds(e, C.byref(spec), part.ctypes.data_as(C.c_void_p), 0, C.cast(C.byref(count), C.c_void_p)),
                           "shc_engine_set_footholds")
        return count.value

    def footholds(self, out, fields=_engine.FH_FIELD_NAMES, which=0, pad: float = 0.0):
        """The requests as the steppers / posers hold them now into the 2-D float32 / float64 array ``out``, row i = the caller's instance i
        (shc_fleet_get_footholds_device): ``BatchEngine.footholds`` for a fleet with the row geometry ``max_legs``; ``pad`` where a
        morphology has no such leg; only the first F columns of out are written.  A device array: one kernel per part, no staging, no host
        wait - complete after ``synchronize()``, or for work queued on a stream after ``order_before(stream)``.  A numpy array: filled part by
        part through the engines' host form."""
        a, spec, _ = _engine._row_pass(self, "footholds: out", out, _engine._ROWS_VIEW,
                                       lambda dt, stride: _engine.foothold_spec(fields, self.max_legs, dt, which, "request", stride, pad), (self.n,))
        if a.on_device:
            _engine._check(self.L.shc_fleet_get_footholds_device(self.h, C.byref(spec), a.pointer), "shc_fleet_get_footholds_device")
            return
        width, spec.row_stride = int(self.L.shc_foothold_width(C.byref(spec))), 0
        for e, _m, _d, ids in self.parts():
            part = np.zeros((len(ids), max(width, 0)), dtype=a.dtype)
            _engine._check(self.L.shc_engine_get_footholds(e, C.byref(spec), part.ctypes.data_as(C.c_void_p), 0), "shc_engine_get_footholds")
            out[ids, :part.shape[1]] = part

    def probe_reach(self, targets, steps: int, fields=("fraction", "limit_proximity"), out=None, first: int = 0, count=None, pad: float = float("nan"),
                    legs=None, dof=None):
        """``BatchEngine.probe_reach`` for the fleet, in the caller's instance order (shc_fleet_probe_reach_device): targets is a float32 /
        float64 DEVICE array (n, C, legs, 3), the result the DEVICE array (n, C, D) - ``out`` when given, else a new torch tensor - in the row
        geometry (legs, dof), default ``max_legs`` / ``max_dof``; ``pad`` where a morphology has no such leg or joint.  One kernel per part on
        the part's stream, no staging, nothing written into the fleet; a fleet takes every robot (first = 0, count None or n).  No host wait:
        complete after ``synchronize()``, or for work queued on a stream after ``order_before(stream)``.  A numpy array is a TypeError (device
        arrays only)."""
        return _engine._probe_reach(self, "shc_fleet_probe_reach_device", targets, steps, fields, out, first, count, pad, legs, dof)

    def step_plan(self, out, fields, horizon: int = 0, pad: float = float("nan")):
        """``BatchEngine.step_plan`` for the fleet (shc_fleet_get_step_plan_device): chosen fields (names of ``engine.PLAN_FIELDS``, in column
        order) of every robot's steppers into the DEVICE array ``out``, row i = the caller's instance i, in the row geometry ``max_legs``;
        ``engine.plan_columns(fields, max_legs, horizon)`` names the columns.  out: any 2-D float32 / float64 object with
        ``__cuda_array_interface__`` of n rows and at least D columns whose rows are contiguous - a view of some columns of a wider tensor will
        do; only its first D columns are written.  One kernel per part on the part's stream, no staging, nothing written into the fleet.  No
        host wait: complete after ``synchronize()``, or for work queued on a stream after ``order_before(stream)``."""
        a, spec, _ = _engine._row_pass(self, "step_plan: out", out, _engine._ROWS,
                                       lambda dt, stride: _engine.plan_spec(fields, self.max_legs, horizon, dt, stride, pad), (self.n,))
        _engine._check(self.L.shc_fleet_get_step_plan_device(self.h, C.byref(spec), a.pointer), "shc_fleet_get_step_plan_device")

    def step_k(self, n_cycles: int, **arrays):
        """K = ``n_cycles`` cycles in one launch per part (shc_fleet_step_k), cycle k with row k of K-deep DEVICE arrays: the names of
        ``set_inputs`` with a leading dimension K - linear_xy (K, n, 2), angular (K, n), imu_orientation_wxyz (K, n, 4), imu_angular_velocity
        (K, n, 3), tip_force (K, n, max_legs, 3), joint_effort (K, n, max_legs, max_dof).  An argument left out (or None) holds that input for
        the K cycles; the two pose inputs are refused (set them beforehand: they are held).  The state, the held inputs and every cycle's
        joints are what K rounds of ``set_inputs(row k)``, ``step(1)``, ``outputs(q, qd)`` give.  No host wait, and the stream rules of
        ``set_inputs``; the arrays are free once the parts have read them (``order_before`` + stream order, or ``synchronize()``)."""
        K = int(n_cycles)
        shapes, st = self._input_shapes(), _engine.FleetInputs()
        for name, a in arrays.items():
            if name not in shapes:
                raise TypeError(f"step_k: unknown input {name!r} (one of {', '.join(shapes)})")
            if a is not None:
                setattr(st, name, _arrays.read(a, name, _engine._FLOAT64, (K,) + shapes[name]).pointer)
        _engine._check(self.L.shc_fleet_step_k(self.h, K, C.byref(st)), "shc_fleet_step_k")

    def step_k_joints(self, first: int = 0, count=None, q=None, qd=None):
        """q / qd of cycles [first, first + count) of the latest ``step_k`` into DEVICE buffers of the caller's, float64 (count, n, max_legs,
        max_dof) in the caller's instance order, NaN padded as ``joints()``.  count None: as many cycles as the buffers given have rows (the
        library refuses a range past the latest K).  Only the buffers given are
        written, every entry of them; at least one must be given.  No host wait: complete after ``synchronize()``, or for work queued on a
        stream after ``order_before(stream)``."""
        row = (self.n, self.max_legs, self.max_dof)
        if count is None and (q is not None or qd is not None):   # (the cycles of the first buffer given, whose other extents are the fleet's)
            count = _arrays.read(qd if q is None else q, "qd" if q is None else "q", _engine._FLOAT64, (None,) + row).shape[0]
        shape = (int(count or 0),) + row
        pq, pqd = _engine._pointer(q, "q", _engine._FLOAT64, shape), _engine._pointer(qd, "qd", _engine._FLOAT64, shape)
        _engine._check(self.L.shc_fleet_get_step_k_joints_device(self.h, int(first), int(count), pq, pqd), "shc_fleet_get_step_k_joints_device")

    def step_k_actions(self, actions, fields, legs=None, dof=None):
        """K = ``actions.shape[0]`` cycles in one launch per part, cycle k with the rows ``actions[k]`` in the caller's instance order
        (shc_fleet_step_k_actions_device): ``step_k`` driven by one 3-D float32 / float64 DEVICE array (K, n, at least A columns), a view
        ``big[:, :, 5:5 + A]`` of a wider tensor included.  ``engine.action_columns(fields, legs, dof)`` names the columns (legs / dof default:
        max_legs / max_dof); the fleet is left as ``step_k`` leaves it when given the columns as float64 arrays, groups not named are held,
        columns of legs and joints a morphology lacks are ignored.  No host wait, and the stream rules of ``set_inputs``.  A numpy array is a
        TypeError (device arrays only)."""
        legs, dof = _engine._geometry(self, legs, dof)
        a, spec, _ = _engine._row_pass(self, "step_k_actions: actions", actions, _engine._CYCLES,
                                       lambda dt, stride: _engine.act_spec(fields, legs, dof, dt, stride), (self.n,))
        _engine._check(self.L.shc_fleet_step_k_actions_device(self.h, a.shape[0], C.byref(spec), a.pointer, _engine._cycle_stride(a)),
                       "shc_fleet_step_k_actions_device")

    def step_k_observations(self, fields=("q", "qd"), dtype="float32", out=None, first: int = 0, count=None, pad: float = 0.0, legs=None, dof=None):
        """q / qd of cycles [first, first + count) of the latest ``step_k`` / ``step_k_actions`` as one (count, n, D) DEVICE array in the
        caller's instance order, one kernel per part (shc_fleet_get_step_k_observations_device): every value is what ``step_k_joints`` holds,
        cast to the element type, ``pad`` where a morphology has no such leg or joint.  out: a 3-D float32 / float64 device array (a view of
        some columns of a wider one will do) - count None: as many cycles as it has; returns None.  Without out (give count) a new torch tensor
        of ``dtype`` on the fleet's device is filled and returned.  No host wait: complete after ``synchronize()``, or for work queued on a
        stream after ``order_before(stream)``."""
        return _engine._step_k_rows(self, "shc_fleet_get_step_k_observations_device", "step_k_observations", fields, dtype, out, first, count, pad, legs, dof)

    def step_k_kinematics(self, fields=("q", "qd", "model_tip"), dtype="float32", out=None, first: int = 0, count=None, pad: float = 0.0, legs=None, dof=None):
        """``step_k_observations`` with the foot tips, in the caller's instance order (shc_fleet_get_step_k_kinematics_device): ``fields`` is any
        of "q", "qd" and "model_tip"; model_tip of cycle first + k is FK(q) of that cycle's joints in the robot frame, 3 columns per leg, ``pad``
        where a morphology has no such leg.  One kernel per part, no staging, nothing written into the fleet; out, count, the return value
        and the ordering rules as ``step_k_observations``.  A numpy array is a TypeError (device arrays only)."""
        return _engine._step_k_rows(self, "shc_fleet_get_step_k_kinematics_device", "step_k_kinematics", fields, dtype, out, first, count, pad, legs, dof)

    def step_k_health(self, select: int = 0, near_limit_proximity: float = 0.0, first: int = 0, count=None, health=None, first_hit=None):
        """``BatchEngine.step_k_health`` for the fleet (shc_fleet_scan_step_k_health_device): the DEVICE arrays (health, first_hit) - (count, n)
        records and int32 (n,) - in the caller's instance order, one kernel per part, no staging.  No host wait: complete after
        ``synchronize()``, or for work queued on a stream after ``order_before(stream)``."""
        return _engine._step_k_health(self, "shc_fleet_scan_step_k_health_device", select, near_limit_proximity, first, count, health, first_hit)

    def _first_device(self):
        """The device a tensor the fleet makes itself goes to: that of the first part (asked only when a tensor is made)."""
        return self.parts()[0][2]

    # what the helpers shared with BatchEngine ask either for: the default row geometry, and the device of a tensor made here
    legs, dof, device = property(lambda self: self.max_legs), property(lambda self: self.max_dof), property(_first_device)

    @staticmethod
    def _stream_handle(stream):
        return C.c_void_p(int(getattr(stream, "cuda_stream", stream) or 0))

    def order_after(self, stream):
        """Every part's stream waits for what is queued on ``stream`` now (a raw stream handle or an object with ``.cuda_stream``; 0 / None: the
        default stream): inputs written by kernels on ``stream`` are complete before a following ``set_inputs`` reads them.  No host wait."""
        _engine._check(self.L.shc_fleet_order_after_stream(self.h, self._stream_handle(stream)), "shc_fleet_order_after_stream")

    def order_before(self, stream):
        """``stream`` waits for what is queued on every part's stream now (split steps are joined first): work queued on ``stream`` afterwards
        sees the results of the preceding ``outputs`` and may overwrite the arrays given to ``set_inputs``.  No host wait."""
        _engine._check(self.L.shc_fleet_order_stream_after(self.h, self._stream_handle(stream)), "shc_fleet_order_stream_after")

    def set_io_chunk(self, robots: int = 0):
        """Robots per part and staging pass of the record outputs (0 = the default)."""
        _engine._check(self.L.shc_fleet_set_io_chunk(self.h, int(robots)), "shc_fleet_set_io_chunk")

    @property
    def io_nbytes(self) -> int:
        """Device bytes the device I/O path holds (ids, staging): 0 before its first use."""
        return int(self.L.shc_fleet_io_bytes(self.h)) if self.h else 0

    def checkpoint(self) -> FleetCheckpoint:
        """A device-resident checkpoint of every robot's state as of now (on each part's stream).  The fleet's first one also uploads the tables
        between the caller's order and the parts' (shc_fleet_checkpoint_create)."""
        return FleetCheckpoint(self)

    def restore(self, ck: FleetCheckpoint, source=None):
        """Robot i <- the checkpoint's robot ``source[i]``, both in the caller's order; an entry < 0 leaves robot i alone; None = every robot.
        ``source``: a host int64 array or list of length n - validated first: an entry >= n, of another morphology or of another part raises and
        nothing changes - or an object with ``__cuda_array_interface__`` (a contiguous int64 array of length n on the fleet's one device, e.g. a
        torch tensor): no host wait, an entry that is out of range or of another morphology / part leaves its robot alone.  The parts run on
        streams of their own: finish the writes to a device map first (``torch.cuda.current_stream().synchronize()``)."""
        a = None if source is None else _arrays.read(source, "restore: source", _engine._SOURCE_MAP, (self.n,))
        _engine._check(self.L.shc_fleet_restore_instances(self.h, ck.h, a and a.pointer, 1 if a and a.on_device else 0), "shc_fleet_restore_instances")

    def scan_and_restore(self, ck: FleetCheckpoint, select: int, near_limit_proximity: float = 0.0, tip_deviation: float = 0.0, health: bool = False):
        """step -> scan -> restore without a map crossing the host (shc_fleet_scan_and_restore): the robots whose flags meet ``select``
        (engine.HEALTH_* bits) are reset to the checkpoint on their part's stream, the others keep walking.  Returns the number of robots restored,
        or with ``health=True`` (n_restored, records): scan_health()'s records as they were BEFORE the restore.  select = 0 is a scan only."""
        crit = _engine.HealthCriteria(int(select), 0, float(near_limit_proximity), float(tip_deviation))
        records = np.zeros(self.n, dtype=_engine.ROBOT_HEALTH_DTYPE) if health else None
        n_restored = C.c_int64(0)
        _engine._check(self.L.shc_fleet_scan_and_restore(self.h, ck.h, C.byref(crit), None if records is None else self._p(records), C.byref(n_restored)),
                       "shc_fleet_scan_and_restore")
        return (n_restored.value, records) if health else n_restored.value

    def all_gather_joints(self):
        """Device pointers (one per device slot) of the gathered [n][max_legs][max_dof] joint buffers."""
        bufs = (C.c_void_p * self.n_devices)()
        _engine._check(self.L.shc_fleet_all_gather_joints(self.h, bufs), "shc_fleet_all_gather_joints")
        return [b for b in bufs]
