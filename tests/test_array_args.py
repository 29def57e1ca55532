"""The one reader of array arguments (syropod_highlevel_controller_amd/arrays.py) and the calls that state their needs to it; no GPU.

The first half needs no library: a table of cases per role - the 2-D rows of the dense-tensor calls under each host mode, the 3-D cycles of
the K-cycle calls, the reach probe's two arrays, the exact shapes of the fleet's device I/O, its record buffers, scan_health's outputs,
restore's source map and set_footholds' ``ignored`` - each with a literal expected outcome: the tuple of numbers handed on, or the exception
class.  The expectations were produced by running the eight decoders this reader replaced (_rows_array in its device and host forms with
_device_only, _cycles_array, _reach_array, _device_array, _device_records, BatchEngine._device_out, _source_map and _foothold_ignored of the
commit before arrays.py) over this same table.  A case whose outcome is not theirs carries WAS(their outcome): every one of them has a
dimension of extent 1 whose stride - which addresses nothing, and is judged nowhere now - was what refused it (or, for one padded row, went
on to the library as it was); the test holds each marked case to that, and to handing on exactly what the contiguous array of its shape
hands on.

Every ``raise`` of the eight is reached by a case (role: label):
  _rows_array     host type / ndim: rows_view "numpy float16", "numpy 1-D"; host strides: rows_view "numpy every second column of (4, 92)";
                  no device array: rows "a list"; device type / ndim: rows "(4, 46) float16", "1-D (46,)"; device strides: rows "(4, 46) column
                  stride 8"
  _device_only    rows_device_only "numpy (4, 46) float32", "a list"
  _cycles_array   numpy: cycles "a numpy array"; no device array: "a list"; type / ndim: "float16", "2-D"; strides: "columns apart"
  _reach_array    numpy: reach4 "a numpy array"; no device array: "a list"; type: "float16"; ndim: "three dimensions where four are taken";
                  inner: "(4, 2, 6, 3) an inner dimension not dense"; robots: "(4, 2, 6, 3) strides[0] below a row"
  _device_array   no device array: exact "a numpy array"; mismatch: "(4, 2) <f4 where <f8 is taken"
  _device_records no device array: records "a numpy array"; mismatch: "one byte short", "(128,) every second byte"
  _device_out     contiguous: out "non-contiguous"; typestr: "a wrong typestr"; bytes: "too small"
  _source_map     device: source "strided"; host: "numpy of the wrong shape"
  _foothold_ignored  ignored "int32", "not a device array"

The second half goes through the methods themselves, on a BatchEngine view and a MixedFleet around no handle at all: a row short, and a numpy
array where only device arrays are taken, are refused with the class they always were before the library sees a handle."""
import numpy as np
import pytest

from syropod_highlevel_controller_amd import arrays, default_hexapod_params, engine
from syropod_highlevel_controller_amd.engine import BatchEngine
from syropod_highlevel_controller_amd.fleet import MixedFleet


class Dev:
    """An object with __cuda_array_interface__ and no memory behind it: the layout checks run before anything is dereferenced."""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=4096):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class WAS:
    """The outcome of the decoder this case went to before there was one reader."""

    def __init__(self, outcome):
        self.outcome = outcome


def _handed_on(d, a):
    """pointer (or, for a host array, whether it is the caller's or a copy), element type, shape, ..."""
    return (d.pointer.value if d.keep is None else "view" if d.keep is a else "copy", d.dtype.name) + d.shape


# what each role hands on, as the calls in engine.py / fleet.py take it from the Array
def rows(host):
    need = {None: engine._ROWS, "view": engine._ROWS_VIEW, "copy": engine._ROWS_COPY}[host]

    def read(a):
        d = arrays.read(a, "t", need)
        return _handed_on(d, a) + (d.strides[0], int(d.on_device))
    return read


def rows_only(a):
    d = arrays.read(a, "t", engine._ROWS_DEVICE_ONLY)
    return _handed_on(d, a) + (d.strides[0], int(d.on_device))


def cycles(a):
    d = arrays.read(a, "t", engine._CYCLES)
    return _handed_on(d, a) + (d.strides[1], engine._cycle_stride(d))


def reach(ndim):
    def read(a):
        d = arrays.read(a, "t", {4: engine._REACH_TARGETS, 3: engine._REACH_OUT}[ndim])
        return (d.pointer.value, d.dtype.name, list(d.shape), d.strides[0])
    return read


def exact(a, typestr, shape):
    return (arrays.read(a, "t", {"<f8": engine._FLOAT64, "<i4": engine._INT32}[typestr], shape).pointer.value,)


def records(a):
    return (arrays.read(a, "t", engine._RECORDS, nbytes=128).pointer.value,)


def out(a, typestr, items, itemsize):
    p = engine._pointer(a, "t", {None: engine._OUT_RECORDS, "<i8": engine._OUT_INT64, "<i4": engine._OUT_INT32}[typestr], nbytes=items * itemsize)
    return (None if p is None else p.value,)


def source(t):
    a, n = t
    d = None if a is None else arrays.read(a, "t", engine._SOURCE_MAP, (n,))
    return (d and _handed_on(d, a)[0], 1 if d and d.on_device else 0)


def ignored(a):
    p = engine._pointer(a, "t", engine._ONE_INT64, nbytes=8)
    return (None if p is None else p.value,)


ROLES = {"rows": rows(None), "rows_view": rows("view"), "rows_copy": rows("copy"), "rows_device_only": rows_only, "cycles": cycles, "reach4": reach(4),
         "reach3": reach(3), "exact": lambda t: exact(*t), "records": records, "out": lambda t: out(*t), "source": source, "ignored": ignored}

CASES = {
    "rows": [
        ("(0, 46) strides None", lambda: Dev((0, 46)), (4096, 'float32', 0, 46, 46, 1)),
        ("(0, 46) dense", lambda: Dev((0, 46), '<f4', (184, 4)), (4096, 'float32', 0, 46, 46, 1)),
        ("(0, 46) rows padded to 62", lambda: Dev((0, 46), '<f4', (248, 4)), (4096, 'float32', 0, 46, 62, 1)),
        ("(0, 46) row stride no multiple of the item size", lambda: Dev((0, 46), '<f4', (250, 4)), ValueError),
        ("(0, 46) row stride below the width", lambda: Dev((0, 46), '<f4', (180, 4)), ValueError),
        ("(0, 46) column stride 8", lambda: Dev((0, 46), '<f4', (368, 8)), ValueError),
        ("(1, 46) strides None", lambda: Dev((1, 46)), (4096, 'float32', 1, 46, 46, 1)),
        ("(1, 46) dense", lambda: Dev((1, 46), '<f4', (184, 4)), (4096, 'float32', 1, 46, 46, 1)),
        ("(1, 46) rows padded to 62", lambda: Dev((1, 46), '<f4', (248, 4)), (4096, 'float32', 1, 46, 46, 1), WAS((4096, 'float32', 1, 46, 62, 1))),
        ("(1, 46) row stride no multiple of the item size", lambda: Dev((1, 46), '<f4', (250, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) row stride below the width", lambda: Dev((1, 46), '<f4', (180, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) column stride 8", lambda: Dev((1, 46), '<f4', (368, 8)), ValueError),
        ("(4, 1) strides None", lambda: Dev((4, 1)), (4096, 'float32', 4, 1, 1, 1)),
        ("(4, 1) dense", lambda: Dev((4, 1), '<f4', (4, 4)), (4096, 'float32', 4, 1, 1, 1)),
        ("(4, 1) rows padded to 62", lambda: Dev((4, 1), '<f4', (248, 4)), (4096, 'float32', 4, 1, 62, 1)),
        ("(4, 1) row stride no multiple of the item size", lambda: Dev((4, 1), '<f4', (250, 4)), ValueError),
        ("(4, 1) row stride below the width", lambda: Dev((4, 1), '<f4', (0, 4)), ValueError),
        ("(4, 1) column stride 8", lambda: Dev((4, 1), '<f4', (8, 8)), (4096, 'float32', 4, 1, 2, 1), WAS(ValueError)),
        ("(4, 46) strides None", lambda: Dev((4, 46)), (4096, 'float32', 4, 46, 46, 1)),
        ("(4, 46) dense", lambda: Dev((4, 46), '<f4', (184, 4)), (4096, 'float32', 4, 46, 46, 1)),
        ("(4, 46) rows padded to 62", lambda: Dev((4, 46), '<f4', (248, 4)), (4096, 'float32', 4, 46, 62, 1)),
        ("(4, 46) row stride no multiple of the item size", lambda: Dev((4, 46), '<f4', (250, 4)), ValueError),
        ("(4, 46) row stride below the width", lambda: Dev((4, 46), '<f4', (180, 4)), ValueError),
        ("(4, 46) column stride 8", lambda: Dev((4, 46), '<f4', (368, 8)), ValueError),
        ("(1, 46) odd stride 7 on the unit dimension", lambda: Dev((1, 46), '<f4', (7, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) odd stride 999 on the unit dimension", lambda: Dev((1, 46), '<f4', (999, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) unit dimension right, column stride 8", lambda: Dev((1, 46), '<f4', (999, 8)), ValueError),
        ("(4, 1) odd stride 12 on the unit dimension", lambda: Dev((4, 1), '<f4', (4, 12)), (4096, 'float32', 4, 1, 1, 1), WAS(ValueError)),
        ("(4, 1) odd stride 3 on the unit dimension, rows padded", lambda: Dev((4, 1), '<f4', (248, 3)), (4096, 'float32', 4, 1, 62, 1), WAS(ValueError)),
        ("(4, 1) unit dimension odd, row stride no multiple", lambda: Dev((4, 1), '<f4', (6, 12)), ValueError),
        ("(1, 1) both strides odd", lambda: Dev((1, 1), '<f4', (5, 3)), (4096, 'float32', 1, 1, 1, 1), WAS(ValueError)),
        ("(4, 46) float64", lambda: Dev((4, 46), '<f8'), (4096, 'float64', 4, 46, 46, 1)),
        ("(4, 46) float64 rows padded", lambda: Dev((4, 46), '<f8', (496, 8)), (4096, 'float64', 4, 46, 62, 1)),
        ("(4, 46) float64 with float32 strides", lambda: Dev((4, 46), '<f8', (184, 4)), ValueError),
        ("(4, 46) float16", lambda: Dev((4, 46), '<f2'), ValueError),
        ("(4, 46) int64", lambda: Dev((4, 46), '<i8'), ValueError),
        ("1-D (46,)", lambda: Dev((46,)), ValueError),
        ("3-D (2, 4, 46)", lambda: Dev((2, 4, 46)), ValueError),
        ("a list", lambda: [[0.0] * 46] * 4, ValueError),
        ("None", lambda: None, ValueError),
        ("numpy (4, 46) float32", lambda: np.zeros((4, 46), np.float32), ValueError),
        ("numpy (4, 46) float64", lambda: np.zeros((4, 46), np.float64), ValueError),
        ("numpy columns [0, 46) of (4, 62)", lambda: np.zeros((4, 62), np.float32)[:, :46], ValueError),
        ("numpy every second column of (4, 92)", lambda: np.zeros((4, 92), np.float32)[:, ::2], ValueError),
        ("numpy every second column of (0, 92)", lambda: np.zeros((0, 92), np.float32)[:, ::2], ValueError),
        ("numpy every second row of (8, 46)", lambda: np.zeros((8, 46), np.float32)[::2], ValueError),
        ("numpy rows backwards", lambda: np.zeros((4, 46), np.float32)[::-1], ValueError),
        ("numpy (1, 46) of a transposed (46, 1)", lambda: np.zeros((46, 1), np.float32).T, ValueError),
        ("numpy (4, 46) transposed view, columns apart", lambda: np.zeros((46, 4), np.float32).T, ValueError),
        ("numpy float16", lambda: np.zeros((4, 46), np.float16), ValueError),
        ("numpy int64", lambda: np.zeros((4, 46), np.int64), ValueError),
        ("numpy 1-D", lambda: np.zeros(46, np.float32), ValueError),
        ("numpy 3-D", lambda: np.zeros((2, 4, 46), np.float32), ValueError),
    ],
    "rows_view": [
        ("numpy (4, 46) float32", lambda: np.zeros((4, 46), np.float32), ('view', 'float32', 4, 46, 46, 0)),
        ("numpy (4, 46) float64", lambda: np.zeros((4, 46), np.float64), ('view', 'float64', 4, 46, 46, 0)),
        ("numpy columns [0, 46) of (4, 62)", lambda: np.zeros((4, 62), np.float32)[:, :46], ('view', 'float32', 4, 46, 62, 0)),
        ("numpy every second column of (4, 92)", lambda: np.zeros((4, 92), np.float32)[:, ::2], ValueError),
        ("numpy every second column of (0, 92)", lambda: np.zeros((0, 92), np.float32)[:, ::2], ValueError),
        ("numpy every second row of (8, 46)", lambda: np.zeros((8, 46), np.float32)[::2], ('view', 'float32', 4, 46, 92, 0)),
        ("numpy rows backwards", lambda: np.zeros((4, 46), np.float32)[::-1], ValueError),
        ("numpy (1, 46) of a transposed (46, 1)", lambda: np.zeros((46, 1), np.float32).T, ('view', 'float32', 1, 46, 46, 0)),
        ("numpy (4, 46) transposed view, columns apart", lambda: np.zeros((46, 4), np.float32).T, ValueError),
        ("numpy float16", lambda: np.zeros((4, 46), np.float16), ValueError),
        ("numpy int64", lambda: np.zeros((4, 46), np.int64), ValueError),
        ("numpy 1-D", lambda: np.zeros(46, np.float32), ValueError),
        ("numpy 3-D", lambda: np.zeros((2, 4, 46), np.float32), ValueError),
        ("(0, 46) strides None", lambda: Dev((0, 46)), (4096, 'float32', 0, 46, 46, 1)),
        ("(0, 46) dense", lambda: Dev((0, 46), '<f4', (184, 4)), (4096, 'float32', 0, 46, 46, 1)),
        ("(0, 46) rows padded to 62", lambda: Dev((0, 46), '<f4', (248, 4)), (4096, 'float32', 0, 46, 62, 1)),
        ("(0, 46) row stride no multiple of the item size", lambda: Dev((0, 46), '<f4', (250, 4)), ValueError),
        ("(0, 46) row stride below the width", lambda: Dev((0, 46), '<f4', (180, 4)), ValueError),
        ("(0, 46) column stride 8", lambda: Dev((0, 46), '<f4', (368, 8)), ValueError),
        ("(1, 1) both strides odd", lambda: Dev((1, 1), '<f4', (5, 3)), (4096, 'float32', 1, 1, 1, 1), WAS(ValueError)),
        ("(4, 46) float64", lambda: Dev((4, 46), '<f8'), (4096, 'float64', 4, 46, 46, 1)),
        ("(4, 46) float64 rows padded", lambda: Dev((4, 46), '<f8', (496, 8)), (4096, 'float64', 4, 46, 62, 1)),
        ("(4, 46) float64 with float32 strides", lambda: Dev((4, 46), '<f8', (184, 4)), ValueError),
        ("(4, 46) float16", lambda: Dev((4, 46), '<f2'), ValueError),
        ("(4, 46) int64", lambda: Dev((4, 46), '<i8'), ValueError),
        ("1-D (46,)", lambda: Dev((46,)), ValueError),
        ("3-D (2, 4, 46)", lambda: Dev((2, 4, 46)), ValueError),
        ("a list", lambda: [[0.0] * 46] * 4, ValueError),
        ("None", lambda: None, ValueError),
    ],
    "rows_copy": [
        ("numpy (4, 46) float32", lambda: np.zeros((4, 46), np.float32), ('view', 'float32', 4, 46, 46, 0)),
        ("numpy (4, 46) float64", lambda: np.zeros((4, 46), np.float64), ('view', 'float64', 4, 46, 46, 0)),
        ("numpy columns [0, 46) of (4, 62)", lambda: np.zeros((4, 62), np.float32)[:, :46], ('copy', 'float32', 4, 46, 46, 0)),
        ("numpy every second column of (4, 92)", lambda: np.zeros((4, 92), np.float32)[:, ::2], ('copy', 'float32', 4, 46, 46, 0)),
        ("numpy every second column of (0, 92)", lambda: np.zeros((0, 92), np.float32)[:, ::2], ValueError),
        ("numpy every second row of (8, 46)", lambda: np.zeros((8, 46), np.float32)[::2], ('copy', 'float32', 4, 46, 46, 0)),
        ("numpy rows backwards", lambda: np.zeros((4, 46), np.float32)[::-1], ('copy', 'float32', 4, 46, 46, 0)),
        ("numpy (1, 46) of a transposed (46, 1)", lambda: np.zeros((46, 1), np.float32).T, ('view', 'float32', 1, 46, 46, 0)),
        ("numpy (4, 46) transposed view, columns apart", lambda: np.zeros((46, 4), np.float32).T, ('copy', 'float32', 4, 46, 46, 0)),
        ("numpy float16", lambda: np.zeros((4, 46), np.float16), ValueError),
        ("numpy int64", lambda: np.zeros((4, 46), np.int64), ValueError),
        ("numpy 1-D", lambda: np.zeros(46, np.float32), ValueError),
        ("numpy 3-D", lambda: np.zeros((2, 4, 46), np.float32), ValueError),
        ("(1, 46) strides None", lambda: Dev((1, 46)), (4096, 'float32', 1, 46, 46, 1)),
        ("(1, 46) dense", lambda: Dev((1, 46), '<f4', (184, 4)), (4096, 'float32', 1, 46, 46, 1)),
        ("(1, 46) rows padded to 62", lambda: Dev((1, 46), '<f4', (248, 4)), (4096, 'float32', 1, 46, 46, 1), WAS((4096, 'float32', 1, 46, 62, 1))),
        ("(1, 46) row stride no multiple of the item size", lambda: Dev((1, 46), '<f4', (250, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) row stride below the width", lambda: Dev((1, 46), '<f4', (180, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) column stride 8", lambda: Dev((1, 46), '<f4', (368, 8)), ValueError),
        ("1-D (46,)", lambda: Dev((46,)), ValueError),
        ("3-D (2, 4, 46)", lambda: Dev((2, 4, 46)), ValueError),
        ("a list", lambda: [[0.0] * 46] * 4, ValueError),
        ("None", lambda: None, ValueError),
    ],
    "rows_device_only": [
        ("(4, 46) strides None", lambda: Dev((4, 46)), (4096, 'float32', 4, 46, 46, 1)),
        ("(4, 46) dense", lambda: Dev((4, 46), '<f4', (184, 4)), (4096, 'float32', 4, 46, 46, 1)),
        ("(4, 46) rows padded to 62", lambda: Dev((4, 46), '<f4', (248, 4)), (4096, 'float32', 4, 46, 62, 1)),
        ("(4, 46) row stride no multiple of the item size", lambda: Dev((4, 46), '<f4', (250, 4)), ValueError),
        ("(4, 46) row stride below the width", lambda: Dev((4, 46), '<f4', (180, 4)), ValueError),
        ("(4, 46) column stride 8", lambda: Dev((4, 46), '<f4', (368, 8)), ValueError),
        ("(1, 46) odd stride 7 on the unit dimension", lambda: Dev((1, 46), '<f4', (7, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) odd stride 999 on the unit dimension", lambda: Dev((1, 46), '<f4', (999, 4)), (4096, 'float32', 1, 46, 46, 1), WAS(ValueError)),
        ("(1, 46) unit dimension right, column stride 8", lambda: Dev((1, 46), '<f4', (999, 8)), ValueError),
        ("(4, 46) float16", lambda: Dev((4, 46), '<f2'), ValueError),
        ("(4, 46) int64", lambda: Dev((4, 46), '<i8'), ValueError),
        ("1-D (46,)", lambda: Dev((46,)), ValueError),
        ("3-D (2, 4, 46)", lambda: Dev((2, 4, 46)), ValueError),
        ("a list", lambda: [[0.0] * 46] * 4, TypeError),
        ("None", lambda: None, TypeError),
        ("numpy (4, 46) float32", lambda: np.zeros((4, 46), np.float32), TypeError),
    ],
    "cycles": [
        ("(5, 23, 46) strides None", lambda: Dev((5, 23, 46)), (4096, 'float32', 5, 23, 46, 46, 1058)),
        ("columns [5, 51) of (5, 25, 62) float64, 23 rows of each cycle", lambda: Dev((5, 23, 46), '<f8', (25 * 62 * 8, 62 * 8, 8)), (4096, 'float64', 5, 23, 46, 62, 1550)),
        ("(1, 1, 46) strides None", lambda: Dev((1, 1, 46)), (4096, 'float32', 1, 1, 46, 46, 0)),
        ("a numpy array", lambda: np.zeros((5, 23, 46), dtype=np.float32), TypeError),
        ("a list", lambda: [[[0.0]]], TypeError),
        ("2-D", lambda: Dev((23, 46)), ValueError),
        ("float16", lambda: Dev((5, 23, 46), '<f2'), ValueError),
        ("columns apart", lambda: Dev((5, 23, 46), '<f4', (23 * 46 * 4, 4, 23 * 4)), ValueError),
        ("row stride no multiple of the item size", lambda: Dev((5, 23, 46), '<f4', (23 * 46 * 4, 46 * 4 + 2, 4)), ValueError),
        ("cycles closer than rows x row stride", lambda: Dev((5, 23, 46), '<f4', (22 * 46 * 4, 46 * 4, 4)), ValueError),
        ("row stride below the width", lambda: Dev((5, 23, 46), '<f4', (23 * 46 * 4, 45 * 4, 4)), ValueError),
        ("(1, 1, 46) odd outer strides", lambda: Dev((1, 1, 46), '<f4', (7, 999, 4)), (4096, 'float32', 1, 1, 46, 46, 0)),
        ("(1, 23, 46) odd cycle stride", lambda: Dev((1, 23, 46), '<f4', (5, 62 * 4, 4)), (4096, 'float32', 1, 23, 46, 62, 0)),
        ("(5, 1, 46) odd row stride, cycles 62 apart", lambda: Dev((5, 1, 46), '<f4', (62 * 4, 3, 4)), (4096, 'float32', 5, 1, 46, 46, 62)),
        ("(5, 1, 46) odd row stride, cycles below a row apart", lambda: Dev((5, 1, 46), '<f4', (45 * 4, 3, 4)), ValueError),
        ("(5, 23, 1) odd column stride", lambda: Dev((5, 23, 1), '<f4', (23 * 4, 4, 7)), (4096, 'float32', 5, 23, 1, 1, 23)),
        ("(0, 23, 46) odd cycle stride", lambda: Dev((0, 23, 46), '<f4', (5, 46 * 4, 4)), (4096, 'float32', 0, 23, 46, 46, 0)),
        ("(0, 23, 46) columns apart", lambda: Dev((0, 23, 46), '<f4', (23 * 46 * 8, 46 * 8, 8)), ValueError),
        ("cycle stride no multiple of the item size", lambda: Dev((5, 23, 46), '<f4', (23 * 46 * 4 + 2, 46 * 4, 4)), ValueError),
        ("int64", lambda: Dev((5, 23, 46), '<i8'), ValueError),
    ],
    "reach4": [
        ("(4, 2, 6, 3) strides None", lambda: Dev((4, 2, 6, 3)), (4096, 'float32', [4, 2, 6, 3], 36)),
        ("(4, 2, 6, 3) dense", lambda: Dev((4, 2, 6, 3), '<f4', (144, 72, 12, 4)), (4096, 'float32', [4, 2, 6, 3], 36)),
        ("(4, 2, 6, 3) robots further apart", lambda: Dev((4, 2, 6, 3), '<f4', (400, 72, 12, 4)), (4096, 'float32', [4, 2, 6, 3], 100)),
        ("(4, 2, 6, 3) float64 robots further apart", lambda: Dev((4, 2, 6, 3), '<f8', (800, 144, 24, 8)), (4096, 'float64', [4, 2, 6, 3], 100)),
        ("(4, 2, 6, 3) an inner dimension not dense", lambda: Dev((4, 2, 6, 3), '<f4', (400, 72, 16, 4)), ValueError),
        ("(4, 2, 6, 3) last dimension not dense", lambda: Dev((4, 2, 6, 3), '<f4', (288, 144, 24, 8)), ValueError),
        ("(4, 2, 6, 3) strides[0] below a row", lambda: Dev((4, 2, 6, 3), '<f4', (140, 72, 12, 4)), ValueError),
        ("(4, 2, 6, 3) strides[0] no multiple of the item size", lambda: Dev((4, 2, 6, 3), '<f4', (146, 72, 12, 4)), ValueError),
        ("(4, 1, 6, 3) odd stride on the unit dimension", lambda: Dev((4, 1, 6, 3), '<f4', (72, 5, 12, 4)), (4096, 'float32', [4, 1, 6, 3], 18)),
        ("(1, 2, 6, 3) odd stride on the robots", lambda: Dev((1, 2, 6, 3), '<f4', (7, 72, 12, 4)), (4096, 'float32', [1, 2, 6, 3], 36)),
        ("(0, 2, 6, 3) strides None", lambda: Dev((0, 2, 6, 3)), (4096, 'float32', [0, 2, 6, 3], 36)),
        ("(0, 2, 6, 3) strides of anything", lambda: Dev((0, 2, 6, 3), '<f4', (3, 5, 7, 9)), (4096, 'float32', [0, 2, 6, 3], 36)),
        ("(4, 0, 6, 3) strides of anything", lambda: Dev((4, 0, 6, 3), '<f4', (3, 5, 7, 9)), (4096, 'float32', [4, 0, 6, 3], 0)),
        ("float16", lambda: Dev((4, 2, 6, 3), '<f2'), TypeError),
        ("int64", lambda: Dev((4, 2, 6, 3), '<i8'), TypeError),
        ("three dimensions where four are taken", lambda: Dev((4, 2, 18)), ValueError),
        ("a numpy array", lambda: np.zeros((4, 2, 6, 3), np.float32), TypeError),
        ("a list", lambda: [[[[0.0] * 3] * 6] * 2] * 4, TypeError),
    ],
    "reach3": [
        ("(4, 2, 12) strides None", lambda: Dev((4, 2, 12)), (4096, 'float32', [4, 2, 12], 24)),
        ("(4, 2, 12) robots further apart", lambda: Dev((4, 2, 12), '<f4', (400, 48, 4)), (4096, 'float32', [4, 2, 12], 100)),
        ("(4, 2, 12) an inner dimension not dense", lambda: Dev((4, 2, 12), '<f4', (400, 52, 4)), ValueError),
        ("(4, 2, 12) strides[0] below a row", lambda: Dev((4, 2, 12), '<f4', (92, 48, 4)), ValueError),
        ("(4, 1, 12) odd stride on the unit dimension", lambda: Dev((4, 1, 12), '<f4', (48, 5, 4)), (4096, 'float32', [4, 1, 12], 12)),
        ("(0, 2, 12) strides of anything", lambda: Dev((0, 2, 12), '<f4', (3, 5, 7)), (4096, 'float32', [0, 2, 12], 24)),
        ("float16", lambda: Dev((4, 2, 12), '<f2'), TypeError),
        ("four dimensions where three are taken", lambda: Dev((4, 2, 6, 2)), ValueError),
        ("a numpy array", lambda: np.zeros((4, 2, 12), np.float32), TypeError),
    ],
    "exact": [
        ("(4, 2) <f8 strides None", lambda: (Dev((4, 2), '<f8'), '<f8', (4, 2)), (4096,)),
        ("(4, 2) <f8 dense", lambda: (Dev((4, 2), '<f8', (16, 8)), '<f8', (4, 2)), (4096,)),
        ("(4, 2) <f8 other strides", lambda: (Dev((4, 2), '<f8', (32, 8)), '<f8', (4, 2)), ValueError),
        ("(4, 2) <f4 where <f8 is taken", lambda: (Dev((4, 2), '<f4'), '<f8', (4, 2)), ValueError),
        ("(4, 3) where (4, 2) is taken", lambda: (Dev((4, 3), '<f8'), '<f8', (4, 2)), ValueError),
        ("(4,) <i4 strides None", lambda: (Dev((4,), '<i4'), '<i4', (4,)), (4096,)),
        ("(4,) <i4 dense", lambda: (Dev((4,), '<i4', (4,)), '<i4', (4,)), (4096,)),
        ("(4,) <i4 other strides", lambda: (Dev((4,), '<i4', (8,)), '<i4', (4,)), ValueError),
        ("(4,) <i8 where <i4 is taken", lambda: (Dev((4,), '<i8'), '<i4', (4,)), ValueError),
        ("(5,) where (4,) is taken", lambda: (Dev((5,), '<i4'), '<i4', (4,)), ValueError),
        ("(3, 4, 6, 3) <f8 strides None", lambda: (Dev((3, 4, 6, 3), '<f8'), '<f8', (3, 4, 6, 3)), (4096,)),
        ("(3, 4, 6, 3) <f8 dense", lambda: (Dev((3, 4, 6, 3), '<f8', (576, 144, 24, 8)), '<f8', (3, 4, 6, 3)), (4096,)),
        ("(3, 4, 6, 3) <f8 other strides", lambda: (Dev((3, 4, 6, 3), '<f8', (1152, 144, 24, 8)), '<f8', (3, 4, 6, 3)), ValueError),
        ("(3, 4, 6, 3) <f4 where <f8 is taken", lambda: (Dev((3, 4, 6, 3), '<f4'), '<f8', (3, 4, 6, 3)), ValueError),
        ("(3, 4, 6, 4) where (3, 4, 6, 3) is taken", lambda: (Dev((3, 4, 6, 4), '<f8'), '<f8', (3, 4, 6, 3)), ValueError),
        ("(1, 3) <f8 strides None", lambda: (Dev((1, 3), '<f8'), '<f8', (1, 3)), (4096,)),
        ("(1, 3) <f8 dense", lambda: (Dev((1, 3), '<f8', (24, 8)), '<f8', (1, 3)), (4096,)),
        ("(1, 3) <f8 other strides", lambda: (Dev((1, 3), '<f8', (7, 8)), '<f8', (1, 3)), (4096,), WAS(ValueError)),
        ("(1, 3) <f4 where <f8 is taken", lambda: (Dev((1, 3), '<f4'), '<f8', (1, 3)), ValueError),
        ("(1, 4) where (1, 3) is taken", lambda: (Dev((1, 4), '<f8'), '<f8', (1, 3)), ValueError),
        ("(1, 3) inner stride wrong", lambda: (Dev((1, 3), '<f8', (7, 16)), '<f8', (1, 3)), ValueError),
        ("(4, 1) odd stride on the unit dimension", lambda: (Dev((4, 1), '<f8', (8, 5)), '<f8', (4, 1)), (4096,), WAS(ValueError)),
        ("a dimension short", lambda: (Dev((4,), '<f8'), '<f8', (4, 2)), ValueError),
        ("(0, 4, 6, 3) strides None", lambda: (Dev((0, 4, 6, 3), '<f8'), '<f8', (0, 4, 6, 3)), (4096,)),
        ("(0, 4, 6, 3) dense", lambda: (Dev((0, 4, 6, 3), '<f8', (576, 144, 24, 8)), '<f8', (0, 4, 6, 3)), (4096,)),
        ("(0, 4, 6, 3) other strides", lambda: (Dev((0, 4, 6, 3), '<f8', (1152, 144, 24, 8)), '<f8', (0, 4, 6, 3)), ValueError),
        ("a numpy array", lambda: (np.zeros((4, 2)), '<f8', (4, 2)), ValueError),
        ("a list", lambda: ([0, 0, 0, 0], '<i4', (4,)), ValueError),
    ],
    "records": [
        ("|u1 (128,)", lambda: Dev((128,), '|u1'), (4096,)),
        ("|u1 (128,) dense", lambda: Dev((128,), '|u1', (1,)), (4096,)),
        ("<f8 (4, 4)", lambda: Dev((4, 4), '<f8'), (4096,)),
        ("<f8 (4, 4) dense", lambda: Dev((4, 4), '<f8', (32, 8)), (4096,)),
        ("|V32 (4,)", lambda: Dev((4,), '|V32'), (4096,)),
        ("(1, 128) odd outer stride", lambda: Dev((1, 128), '|u1', (77, 1)), (4096,)),
        ("(128,) every second byte", lambda: Dev((128,), '|u1', (2,)), ValueError),
        ("(4, 4) rows apart", lambda: Dev((4, 4), '<f8', (64, 8)), ValueError),
        ("one byte short", lambda: Dev((127,), '|u1'), ValueError),
        ("eight bytes long", lambda: Dev((17,), '<f8'), ValueError),
        ("a numpy array", lambda: np.zeros(128, np.uint8), ValueError),
        ("an integer", lambda: 4096, ValueError),
    ],
    "out": [
        ("None", lambda: (None, '<i8', 4, 8), (None,)),
        ("an integer", lambda: (12345, '<i8', 4, 8), (12345,)),
        ("large enough", lambda: (Dev((4,), '<i8'), '<i8', 4, 8), (4096,)),
        ("larger", lambda: (Dev((2, 4), '<i8'), '<i8', 4, 8), (4096,)),
        ("too small", lambda: (Dev((3,), '<i8'), '<i8', 4, 8), ValueError),
        ("a wrong typestr", lambda: (Dev((8,), '<i4'), '<i8', 4, 8), ValueError),
        ("records of any type", lambda: (Dev((4, 4), '<f8'), None, 4, 32), (4096,)),
        ("records too small", lambda: (Dev((4, 3), '<f8'), None, 4, 32), ValueError),
        ("non-contiguous", lambda: (Dev((4,), '<i8', (16,)), '<i8', 4, 8), ValueError),
        ("non-contiguous and of the wrong type", lambda: (Dev((4,), '<i4', (16,)), '<i8', 4, 8), ValueError),
        ("a unit dimension with an odd stride", lambda: (Dev((1, 4), '<i8', (5, 8)), '<i8', 4, 8), (4096,)),
        ("an empty array with strides, nothing asked for", lambda: (Dev((0,), '<i8', (16,)), '<i8', 0, 8), (4096,)),
        ("an empty array with strides, four asked for", lambda: (Dev((0, 4), '<i8', (999, 3)), '<i8', 4, 8), ValueError),
        ("int32 (4,)", lambda: (Dev((4,), '<i4'), '<i4', 4, 4), (4096,)),
    ],
    "source": [
        ("None", lambda: (None, 4), (None, 0)),
        ("numpy int64 (4,)", lambda: (np.arange(4), 4), ('view', 0)),
        ("numpy int32 (4,)", lambda: (np.arange(4, dtype=np.int32), 4), ('copy', 0)),
        ("numpy every second of 8", lambda: (np.arange(8)[::2], 4), ('copy', 0)),
        ("numpy of the wrong shape", lambda: (np.arange(5), 4), ValueError),
        ("numpy 2-D", lambda: (np.zeros((4, 1), np.int64), 4), ValueError),
        ("a list", lambda: ([0, 1, 2, 3], 4), ('copy', 0)),
        ("a list of the wrong length", lambda: ([0, 1, 2], 4), ValueError),
        ("a device array", lambda: (Dev((4,), '<i8'), 4), (4096, 1)),
        ("a device array, dense strides", lambda: (Dev((4,), '<i8', (8,)), 4), (4096, 1)),
        ("a wrong dtype", lambda: (Dev((4,), '<i4'), 4), ValueError),
        ("a wrong shape", lambda: (Dev((5,), '<i8'), 4), ValueError),
        ("2-D", lambda: (Dev((4, 1), '<i8'), 4), ValueError),
        ("strided", lambda: (Dev((4,), '<i8', (16,)), 4), ValueError),
        ("one robot, an odd stride", lambda: (Dev((1,), '<i8', (3,)), 1), (4096, 1), WAS(ValueError)),
        ("one robot, numpy", lambda: (np.zeros(1, np.int64), 1), ('view', 0)),
        ("one robot, a scalar", lambda: (0, 1), ('copy', 0)),
        ("no robot, a stride", lambda: (Dev((0,), '<i8', (16,)), 0), ValueError),
    ],
    "ignored": [
        ("None", lambda: None, (None,)),
        ("(1,) int64", lambda: Dev((1,), '<i8'), (4096,)),
        ("(1, 1) int64", lambda: Dev((1, 1), '<i8'), (4096,)),
        ("(1,) int64 with an odd stride", lambda: Dev((1,), '<i8', (3,)), (4096,)),
        ("() int64", lambda: Dev((), '<i8'), (4096,)),
        ("int32", lambda: Dev((1,), '<i4'), ValueError),
        ("two elements", lambda: Dev((2,), '<i8'), ValueError),
        ("no elements", lambda: Dev((0,), '<i8'), ValueError),
        ("not a device array", lambda: np.zeros(1, np.int64), ValueError),
        ("an integer", lambda: 4096, ValueError),
    ],
}


def _outcome(role, make):
    try:
        return tuple(ROLES[role](make()))
    except Exception as exc:
        return type(exc)


@pytest.mark.parametrize("role", list(CASES))
def test_every_case_of_the_table(role):
    assert len({label for label, *_ in CASES[role]}) == len(CASES[role])
    for label, make, expected, *was in CASES[role]:
        assert _outcome(role, make) == expected, f"{role}: {label}"
        assert not was or was[0].outcome != expected, f"{role}: {label} is marked and has not changed"


def _array_of(argument):
    return argument[0] if isinstance(argument, tuple) else argument


def test_only_a_unit_extent_moves_and_only_from_refused_to_the_contiguous_answer():
    marked = [(role, label, make, expected, was[0]) for role in CASES for label, make, expected, *was in CASES[role] if was]
    assert marked and {role for role, *_ in marked} <= {"rows", "rows_view", "rows_copy", "rows_device_only", "exact", "source"}
    # (the three decoders that judged one: _rows_array's device form - whatever the host mode -, _device_array and _source_map)
    for role, label, make, expected, was in marked:
        argument = make()
        cai = _array_of(argument).__cuda_array_interface__
        assert isinstance(expected, tuple), f"{role}: {label}"
        if was.outcome is not ValueError:   # (it passed, and the stride of its one row went on as it was: the only number that differs)
            assert role.startswith("rows") and was.outcome[:4] + was.outcome[5:] == expected[:4] + expected[5:], f"{role}: {label}"
        assert 1 in cai["shape"], f"{role}: {label}"
        # what it hands on is what the same array hands on with the dense value in place of the strides of its unit-extent dimensions (its other
        # strides are right) - for all but the column whose rows lie further apart that is the contiguous array of its shape
        dense, strides = int(cai["typestr"][2:]), []
        for extent, stride in zip(reversed(cai["shape"]), reversed(cai["strides"])):
            strides.insert(0, dense if extent == 1 else stride)
            dense = strides[0] * extent
        same = lambda array: (array,) + argument[1:] if isinstance(argument, tuple) else array
        assert _outcome(role, lambda: same(Dev(cai["shape"], cai["typestr"], tuple(strides)))) == expected, f"{role}: {label}"
        if dense == int(cai["typestr"][2:]) * int(np.prod(cai["shape"])):
            assert _outcome(role, lambda: same(Dev(cai["shape"], cai["typestr"]))) == expected, f"{role}: {label}"

def test_the_python_layer_reads_a_3d_view():
    """(moved here from tests/test_rollout_abi.py with the reader: every case and every number as it was)"""
    def read(a):
        d = arrays.read(a, "t", engine._CYCLES)
        return (d.pointer, d.dtype) + d.shape + (d.strides[1], engine._cycle_stride(d))
    ptr, dt, cycles, rows, columns, stride, cycle_stride = read(Dev((5, 23, 46)))
    assert (dt, cycles, rows, columns, stride, cycle_stride) == (np.dtype("float32"), 5, 23, 46, 46, 23 * 46)
    # columns [5, 51) of a (5, 25, 62) tensor, the first 23 rows of each cycle
    view = Dev((5, 23, 46), "<f8", (25 * 62 * 8, 62 * 8, 8))
    assert read(view)[2:] == (5, 23, 46, 62, 25 * 62)
    assert read(Dev((1, 1, 46)))[2:] == (1, 1, 46, 46, 0)
    with pytest.raises(TypeError, match="device arrays only"):
        read(np.zeros((5, 23, 46), dtype=np.float32))
    with pytest.raises(TypeError, match="device arrays only"):
        read([[[0.0]]])
    for bad in (Dev((23, 46)), Dev((5, 23, 46), "<f2"), Dev((5, 23, 46), "<f4", (23 * 46 * 4, 4, 23 * 4)),
                Dev((5, 23, 46), "<f4", (23 * 46 * 4, 46 * 4 + 2, 4)), Dev((5, 23, 46), "<f4", (22 * 46 * 4, 46 * 4, 4)),
                Dev((5, 23, 46), "<f4", (23 * 46 * 4, 45 * 4, 4))):
        with pytest.raises(ValueError):
            read(bad)


def test_the_array_says_what_was_read():
    d = arrays.read(Dev((4, 1, 46), "<f8", (62 * 8, 5, 8)), "t", arrays.Need(ndim=3, dense_from=2))
    assert (d.pointer.value, d.dtype, d.shape, d.strides, d.on_device, d.keep) == (4096, np.dtype("float64"), (4, 1, 46), (62, 46, 1), True, None)
    host = np.zeros((4, 62), np.float32)[:, :46]
    d = arrays.read(host, "t", engine._ROWS_VIEW)
    assert (d.pointer.value, d.strides, d.on_device) == (host.ctypes.data, (62, 1), False) and d.keep is host
    d = arrays.read(12345, "t", engine._OUT_INT64, nbytes=8)
    assert (d.pointer.value, d.dtype, d.shape, d.on_device) == (12345, None, (), True)
    for message, call in (("actions", lambda: arrays.read(Dev((4, 46), "<f4", (184, 8)), "set_actions: actions", engine._ROWS)),
                          ("(4, 46)", lambda: arrays.read(Dev((4, 46), "<f4", (184, 8)), "t", engine._ROWS)),
                          ("(184, 8)", lambda: arrays.read(Dev((4, 46), "<f4", (184, 8)), "t", engine._ROWS)),
                          ("<f2", lambda: arrays.read(Dev((4, 46), "<f2"), "t", engine._ROWS)),
                          (r"\(4, 3\)", lambda: arrays.read(Dev((4, 2), "<f8"), "t", engine._FLOAT64, (4, 3))),
                          ("list", lambda: arrays.read([1.0], "t", engine._ROWS))):
        with pytest.raises(ValueError, match=message):
            call()


# ---- the methods, around no handle at all

def handles_without_a_device():
    eng = BatchEngine.view(0, default_hexapod_params("tripod"), 4)
    fleet = MixedFleet.__new__(MixedFleet)
    fleet.L, fleet.h, fleet.n, fleet.max_legs, fleet.max_dof = engine.lib(), None, 4, 8, 5
    return eng, fleet


VELOCITY, JOINTS, FOOTHOLD = ("linear_xy", "angular"), ("q", "qd"), ("position", "defined")   # 3 columns; 2 * legs * dof; 4 * legs


def _calls(who, legs, dof):
    """{method: (call(array), the shape with a row short, whether it takes device arrays only)}"""
    calls = {
        "set_actions": (lambda a: who.set_actions(a, VELOCITY), (3, 3), isinstance(who, MixedFleet)),
        "step_k_actions": (lambda a: who.step_k_actions(a, VELOCITY), (2, 3, 3), True),
        "observations": (lambda a: who.observations(out=a, fields=JOINTS), (3, 2 * legs * dof), True),
        "set_footholds": (lambda a: who.set_footholds(a, FOOTHOLD), (3, 4 * legs), False),
        "footholds": (lambda a: who.footholds(a, FOOTHOLD), (3, 4 * legs), False),
        "step_k_observations": (lambda a: who.step_k_observations(out=a), (2, 3, 2 * legs * dof), True),
        "step_k_kinematics": (lambda a: who.step_k_kinematics(out=a), (2, 3, 2 * legs * dof + 3 * legs), True),
        "probe_reach": (lambda a: who.probe_reach(a, 16), (3, 2, legs, 3), True),
    }
    if isinstance(who, BatchEngine):
        calls["resident_post_actions"] = (lambda a: who.resident_post_actions(a, VELOCITY), (3, 3), True)
        calls["resident_observations"] = (lambda a: who.resident_observations(0, out=a), (3, 2 * legs * dof), True)
    return calls


NO_HOST_FORM = {"step_k_actions", "step_k_observations", "step_k_kinematics", "probe_reach", "resident_post_actions", "resident_observations"}   # TypeError


def test_a_row_short_and_a_host_array_are_refused_before_the_library_sees_a_handle():
    for who, legs, dof in zip(handles_without_a_device(), (6, 8), (3, 5)):
        for name, (call, short, device_only) in _calls(who, legs, dof).items():
            whole = (4,) + short[1:] if len(short) in (2, 4) else short[:1] + (4,) + short[2:]
            if name == "probe_reach":
                with pytest.raises(ValueError):
                    who.probe_reach(Dev(whole), 16, out=Dev((3, 2, 2 * legs)))             # out a robot short
            with pytest.raises(ValueError):
                call(Dev(short))
            if device_only:
                with pytest.raises(TypeError if name in NO_HOST_FORM else ValueError, match="device arrays only" if name in NO_HOST_FORM else None):
                    call(np.zeros(whole, dtype=np.float32))
            else:
                with pytest.raises(ValueError):
                    call(np.zeros(short, dtype=np.float32))                                # a host array a row short


def test_a_view_has_no_device_and_a_fleet_the_same_attributes():
    eng, fleet = handles_without_a_device()
    assert eng.device is None and (eng.legs, eng.dof) == (6, 3) and (fleet.legs, fleet.dof) == (8, 5)
    assert isinstance(MixedFleet.device, property)   # (asked only when a tensor is made: it goes to the first part's device)


def test_the_fleets_exact_shapes_and_the_outputs_are_refused_before_the_library_sees_a_handle():
    eng, fleet = handles_without_a_device()
    for call in (lambda: fleet.set_inputs(angular=Dev((3,), "<f8")), lambda: fleet.set_inputs(angular=Dev((4,), "<f4")),
                 lambda: fleet.set_inputs(angular=np.zeros(4)), lambda: fleet.set_inputs(linear_xy=Dev((4, 2), "<f8", (8, 32))),
                 lambda: fleet.step_k(3, tip_force=Dev((3, 4, 6, 3), "<f8")), lambda: fleet.step_k_joints(q=Dev((3, 4, 8, 4), "<f8")),
                 lambda: fleet.step_k_joints(0, 3, qd=Dev((2, 4, 8, 5), "<f8")), lambda: fleet.outputs(q=Dev((4, 6, 3), "<f8")),
                 lambda: fleet.outputs(walk_state=Dev((4,), "<i8")), lambda: fleet.outputs(health=Dev((4 * 32 - 1,), "|u1")),
                 lambda: fleet.restore(None, Dev((4,), "<i8", (16,))), lambda: eng.restore(None, [0, 1, 2]),
                 lambda: eng.scan_health(out_health=Dev((3, 4), "<f8")), lambda: eng.scan_health(out_restore_map=Dev((4,), "<i4")),
                 lambda: eng.step_k_health(count=2, health=Dev((1, 4, 4), "<f8"), first_hit=Dev((4,), "<i4")), lambda: fleet.step_k_health(first_hit=Dev((4,), "<i4")),
                 lambda: eng.set_footholds(Dev((4, 24)), FOOTHOLD, ignored=Dev((2,), "<i8")),
                 lambda: fleet.set_footholds(Dev((4, 32)), FOOTHOLD, ignored=np.zeros(1, np.int64))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError, match="device arrays only"):
        eng.step_k_health(count=2, health=np.zeros((2, 4, 4)))
    with pytest.raises(TypeError, match="unknown input"):
        fleet.set_inputs(velocity=Dev((4,), "<f8"))
