"""Fleet step_k, the part that needs no GPU: the exported symbols, the ABI version, and the NULL-handle answers (no call here reaches a device)."""
import ctypes as C

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, FleetInputs
from syropod_highlevel_controller_amd.fleet import MixedFleet

SYMBOLS = ["shc_fleet_step_k", "shc_fleet_get_step_k_joints_device"]


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.shc_abi_version() == 6
    assert callable(MixedFleet.step_k) and callable(MixedFleet.step_k_joints)


def test_null_handles_are_refused():
    lib = engine.lib()
    rows = FleetInputs()
    assert lib.shc_fleet_step_k(None, 1, C.byref(rows)) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_step_k(None, 1, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_get_step_k_joints_device(None, 0, 1, None, None) == SHC_ERR_INVALID_ARG
    buf = (C.c_double * 8)()   # (never dereferenced: the handle is refused first)
    assert lib.shc_fleet_get_step_k_joints_device(None, 0, 1, buf, buf) == SHC_ERR_INVALID_ARG
