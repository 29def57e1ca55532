"""Rollout tensors, the part that needs no GPU: the four exported symbols and their declarations, the ABI version, the NULL answers (no call
here reaches a device) and what the Python layer refuses before it calls the library."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, BatchEngine, act_spec, obs_spec
from syropod_highlevel_controller_amd.fleet import MixedFleet

SYMBOLS = ["shc_engine_step_k_actions", "shc_engine_get_step_k_observations", "shc_fleet_step_k_actions_device", "shc_fleet_get_step_k_observations_device"]


def test_symbols_are_exported_declared_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
        assert engine.HEADER.functions[s][0] == "int", f"{s} is not declared in include/shc_batch.h"
    assert lib.shc_abi_version() == 6
    for cls in (BatchEngine, MixedFleet):
        assert callable(cls.step_k_actions) and callable(cls.step_k_observations)


def test_null_handles_specs_and_arrays_are_refused():
    lib = engine.lib()
    act = act_spec(("linear_xy", "angular"), 6, 3, "float32")
    obs = obs_spec(("q", "qd"), 6, 3, "float32")
    buf = (C.c_float * 64)()   # (never dereferenced: the handle is refused first)
    for spec_a, spec_o, array in ((C.byref(act), C.byref(obs), buf), (None, None, buf), (C.byref(act), C.byref(obs), None), (None, None, None)):
        assert lib.shc_engine_step_k_actions(None, 1, spec_a, array, 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_engine_get_step_k_observations(None, 0, 1, spec_o, array, 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_step_k_actions_device(None, 1, spec_a, array, 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_fleet_get_step_k_observations_device(None, 0, 1, spec_o, array, 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_last_error()


class FakeDeviceArray:
    """An object with __cuda_array_interface__ and no memory behind it: the layout checks run before anything is dereferenced."""

    def __init__(self, shape, typestr="<f4", strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (4096, False), "version": 3, "strides": strides}


def test_the_python_layer_reads_a_3d_view():
    ptr, dt, cycles, rows, columns, stride, cycle_stride = engine._cycles_array(FakeDeviceArray((5, 23, 46)), "t")
    assert (dt, cycles, rows, columns, stride, cycle_stride) == (np.dtype("float32"), 5, 23, 46, 46, 23 * 46)
    # columns [5, 51) of a (5, 25, 62) tensor, the first 23 rows of each cycle
    view = FakeDeviceArray((5, 23, 46), "<f8", (25 * 62 * 8, 62 * 8, 8))
    assert engine._cycles_array(view, "t")[2:] == (5, 23, 46, 62, 25 * 62)
    assert engine._cycles_array(FakeDeviceArray((1, 1, 46)), "t")[2:] == (1, 1, 46, 46, 0)
    with pytest.raises(TypeError, match="device arrays only"):
        engine._cycles_array(np.zeros((5, 23, 46), dtype=np.float32), "t")
    with pytest.raises(TypeError, match="device arrays only"):
        engine._cycles_array([[[0.0]]], "t")
    for bad in (FakeDeviceArray((23, 46)), FakeDeviceArray((5, 23, 46), "<f2"), FakeDeviceArray((5, 23, 46), "<f4", (23 * 46 * 4, 4, 23 * 4)),
                FakeDeviceArray((5, 23, 46), "<f4", (23 * 46 * 4, 46 * 4 + 2, 4)), FakeDeviceArray((5, 23, 46), "<f4", (22 * 46 * 4, 46 * 4, 4)),
                FakeDeviceArray((5, 23, 46), "<f4", (23 * 46 * 4, 45 * 4, 4))):
        with pytest.raises(ValueError):
            engine._cycles_array(bad, "t")
