"""Rollout tensors, the part that needs no GPU: the four exported symbols and their declarations, the ABI version and the NULL answers (no call
here reaches a device).  What the Python layer reads of a 3-D view, and refuses before it calls the library: tests/test_array_args.py."""
import ctypes as C

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
