"""Fleet device I/O, the part that needs no GPU: the exported symbols, the ABI version, the size of the two argument structs as the ctypes
mirrors lay them out, and the NULL-handle answers (no call here reaches a device)."""
import ctypes as C

from syropod_highlevel_controller_amd import engine
from syropod_highlevel_controller_amd.engine import SHC_ERR_INVALID_ARG, FleetInputs, FleetOutputs

SYMBOLS = ["shc_fleet_set_inputs_device", "shc_fleet_get_outputs_device", "shc_fleet_order_after_stream", "shc_fleet_order_stream_after",
           "shc_fleet_set_io_chunk", "shc_fleet_io_bytes"]


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = engine.lib()
    for s in SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        getattr(lib, s)
    assert lib.shc_abi_version() == 6


def test_struct_mirrors():
    """shc_fleet_inputs is eight pointers.  shc_fleet_outputs as include/shc_batch.h declares it is six pointers, frame + reserved in one slot, two
    pointers: nine pointer-sized slots, 72 bytes (the library asserts the same sizes and offsets when it is compiled)."""
    assert C.sizeof(C.c_void_p) == 8
    assert C.sizeof(FleetInputs) == 64 and len(FleetInputs._fields_) == 8
    assert C.sizeof(FleetOutputs) == 72
    assert FleetOutputs.frame.offset == 48 and FleetOutputs.reserved.offset == 52 and FleetOutputs.health.offset == 56 and FleetOutputs.criteria.offset == 64
    assert [k for k, _ in FleetInputs._fields_] == list(engine.FLEET_INPUTS)


def test_null_handles_are_refused():
    lib = engine.lib()
    ins, outs = FleetInputs(), FleetOutputs()
    assert lib.shc_fleet_set_inputs_device(None, C.byref(ins)) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_set_inputs_device(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_get_outputs_device(None, C.byref(outs)) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_get_outputs_device(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_order_after_stream(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_order_stream_after(None, None) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_set_io_chunk(None, 0) == SHC_ERR_INVALID_ARG
    assert lib.shc_fleet_io_bytes(None) == 0
