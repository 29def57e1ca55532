"""Fleet checkpoints, the part that needs no GPU: the exported symbols, the ABI version and the NULL-handle answers (no call here reaches a device)."""
import ctypes as C

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG

SYMBOLS = ["shc_fleet_checkpoint_create", "shc_fleet_checkpoint_update", "shc_fleet_checkpoint_destroy", "shc_fleet_checkpoint_bytes",
           "shc_fleet_restore_instances", "shc_fleet_scan_and_restore"]


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.shc_abi_version() == 6


def test_null_handles_are_refused():
    lib = engine.lib()
    out = C.c_void_p()
    assert lib.shc_fleet_checkpoint_create(None, C.byref(out)) == SHC_ERR_INVALID_ARG and not out.value
    assert lib.shc_fleet_checkpoint_create(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_checkpoint_update(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_checkpoint_destroy(None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_checkpoint_bytes(None) == 0
    assert lib.shc_fleet_restore_instances(None, None, None, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_restore_instances(None, None, None, 1) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_scan_and_restore(None, None, None, None, None) == SHC_ERR_INVALID_ARG
