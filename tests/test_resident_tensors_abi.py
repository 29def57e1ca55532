"""Resident tensors, the part that needs no GPU: the two exported symbols and their argument types, the unchanged ABI version, the NULL answers
and the Python layer's own refusal of host arrays (no call here reaches a device)."""
import ctypes as C

import numpy as np
import pytest

from syropod_highlevel_controller_amd import default_hexapod_params, engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, BatchEngine, act_spec, obs_spec

SYMBOLS = {
    "shc_engine_resident_post_actions": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "shc_engine_resident_get_observations_async": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int],
}
DECLARED = {
    "shc_engine_resident_post_actions": [("shc_engine *", "e"), ("const struct shc_act_spec *", "spec"), ("const void *", "actions"), ("int", "publish"), ("int64_t *", "cycle")],
    "shc_engine_resident_get_observations_async": [("shc_engine *", "e"), ("int64_t", "cycle"), ("const struct shc_obs_spec *", "spec"), ("void *", "out"), ("int", "timeout_ms")],
}


def test_symbols_are_exported_declared_and_listed():
    lib = engine.lib()
    for s, argtypes in SYMBOLS.items():
        assert s in engine.EXPORTED_SYMBOLS
        assert engine.HEADER.functions[s] == ("int", DECLARED[s]), f"{s} is not declared in shc_batch.h with the arguments of the issue"
        assert list(getattr(lib, s).argtypes) == argtypes, s
    assert lib.shc_abi_version() == 6, "the tensor passes do not bump the ABI version"
    assert callable(BatchEngine.resident_post_actions) and callable(BatchEngine.resident_observations)


def test_null_handle_spec_and_array_are_refused():
    lib = engine.lib()
    act, obs = act_spec(("linear_xy", "angular"), 6, 3, "float32"), obs_spec(("q", "qd", "model_tip"), 6, 3, "float32")
    buf = (C.c_double * 8)()   # (never dereferenced: the handle is refused first)
    cyc = C.c_int64(-7)
    for spec, array in ((C.byref(act), buf), (None, buf), (C.byref(act), None), (None, None)):
        assert lib.shc_engine_resident_post_actions(None, spec, array, 1, C.byref(cyc)) == SHC_ERR_INVALID_ARG
        assert lib.shc_last_error()
    assert lib.shc_engine_resident_post_actions(None, C.byref(act), buf, 0, None) == SHC_ERR_INVALID_ARG
    for spec, array in ((C.byref(obs), buf), (None, buf), (C.byref(obs), None), (None, None)):
        assert lib.shc_engine_resident_get_observations_async(None, 0, spec, array, 0) == SHC_ERR_INVALID_ARG
        assert lib.shc_last_error()
    assert cyc.value == -7, "a refused post wrote the cycle index"


def test_numpy_arrays_are_a_type_error():
    eng = BatchEngine.view(0, default_hexapod_params("tripod"), 4)   # (around no handle at all: refused before the library is asked)
    with pytest.raises(TypeError, match="device arrays only"):
        eng.resident_post_actions(np.zeros((4, 3), dtype=np.float32), ("linear_xy", "angular"))
    with pytest.raises(TypeError, match="device arrays only"):
        eng.resident_post_actions([[0.0] * 3] * 4, ("linear_xy", "angular"), publish=True)
    with pytest.raises(TypeError, match="device arrays only"):
        eng.resident_observations(0, out=np.zeros((4, 36), dtype=np.float32))
