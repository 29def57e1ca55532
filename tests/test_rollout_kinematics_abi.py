"""Rollout kinematics, the part that needs no GPU: the exported symbols, the ABI version, the struct sizes, the NULL-handle answers and the
Python layer's own refusal of host arrays (no call here reaches a device)."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, BatchEngine, HealthCriteria, ObsSpec, RobotHealth, obs_spec
from syropod_highlevel_controller_amd.fleet import MixedFleet

SYMBOLS = ["shc_engine_get_step_k_kinematics", "shc_engine_scan_step_k_health", "shc_fleet_get_step_k_kinematics_device",
           "shc_fleet_scan_step_k_health_device"]


def test_symbols_are_exported_declared_and_listed():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        assert engine.HEADER.functions[s][0] == "int", f"{s} is not declared in shc_batch.h"
        getattr(lib, s)
    assert lib.shc_abi_version() == 6
    for cls in (BatchEngine, MixedFleet):
        assert callable(cls.step_k_kinematics) and callable(cls.step_k_health)


def test_struct_sizes_are_unchanged():
    # 32 bytes without padding; 37 int32, 4 bytes of alignment, row_stride, pad (the library's own static_asserts hold the C side to the same)
    assert C.sizeof(RobotHealth) == 32 and engine.ROBOT_HEALTH_DTYPE.itemsize == 32
    assert C.sizeof(ObsSpec) == 4 * 37 + 4 + 16
    assert C.sizeof(HealthCriteria) == 24


def test_null_handles_are_refused():
    lib = engine.lib()
    spec = obs_spec(("q", "qd", "model_tip"), 6, 3, "float32")
    buf = (C.c_double * 8)()   # (never dereferenced: the handle is refused first)
    crit = HealthCriteria(engine.HEALTH_POSITION_LIMIT, 0, 0.0, 0.0)
    for name in ("shc_engine_get_step_k_kinematics", "shc_fleet_get_step_k_kinematics_device"):
        assert getattr(lib, name)(None, 0, 1, C.byref(spec), buf, 0) == SHC_ERR_INVALID_ARG, name
        assert lib.shc_last_error(), name
    for name in ("shc_engine_scan_step_k_health", "shc_fleet_scan_step_k_health_device"):
        assert getattr(lib, name)(None, 0, 1, C.byref(crit), buf, buf) == SHC_ERR_INVALID_ARG, name
        assert getattr(lib, name)(None, 0, 1, None, None, None) == SHC_ERR_INVALID_ARG, name
        assert lib.shc_last_error(), name


def handles_without_a_device():
    """A BatchEngine view and a MixedFleet around no handle at all: the refusals below are decided before the library is asked."""
    eng = BatchEngine.view(0, default_hexapod_params("tripod"), 4)
    fleet = MixedFleet.__new__(MixedFleet)
    fleet.L, fleet.h, fleet.n, fleet.max_legs, fleet.max_dof = engine.lib(), None, 4, 8, 5
    return eng, fleet


def test_numpy_arrays_are_a_type_error():
    for who in handles_without_a_device():
        with pytest.raises(TypeError, match="device arrays only"):
            who.step_k_kinematics(out=np.zeros((2, 4, 200), dtype=np.float32))
        with pytest.raises(TypeError, match="device arrays only"):
            who.step_k_health(engine.HEALTH_POSITION_LIMIT, count=2, health=np.zeros((2, 4), dtype=engine.ROBOT_HEALTH_DTYPE))
        with pytest.raises(TypeError, match="device arrays only"):
            who.step_k_health(engine.HEALTH_POSITION_LIMIT, count=2, health=1 << 20, first_hit=np.zeros(4, dtype=np.int32))
