"""The one reader of array arguments: every tensor-shaped argument of BatchEngine / MixedFleet - a device array (an object with the CUDA array
interface, e.g. a torch tensor or a view of one), or a numpy array or an integer device pointer where the call takes one - goes through
``read`` and comes back as one ``Array``.  What a call takes is a ``Need``, stated once next to the call.  Pure Python: the library is never
loaded here.

The layout rule, one for every call: walking from the last dimension to the first, a dimension at or behind ``dense_from`` must lie exactly
on the ones behind it; a dimension before ``dense_from`` may lie further apart - a whole number of elements, and at least the span of the
ones behind it.  A dimension of extent 1 is never judged, anywhere: its stride addresses nothing, and the dense value stands in for it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

_CAI = "__cuda_array_interface__"
FLOATS = ("<f4", "<f8")
# what an array without elements is held to (``Need.empty``): its strides as any other's; not the strides of a zero-extent dimension; or none
JUDGED, DIMENSION, NOTHING = 0, 1, 2


class Array(NamedTuple):
    """What ``read`` makes of an argument: strides in ELEMENTS, the dense value standing in for every dimension of extent 1; ``keep`` owns
    the memory behind a host pointer.  An integer pointer that passed through has no dtype and the shape ()."""
    pointer: C.c_void_p
    dtype: Optional[np.dtype]
    shape: tuple
    strides: tuple
    on_device: bool
    keep: object


class Need(NamedTuple):
    """What a call takes.  types: the typestrs allowed (None: any); ndim: how many dimensions (None: any; an exact shape is given to ``read``);
    dense_from: the first dimension that must be dense; exact: whether ``read``'s nbytes means exactly that many bytes, or at least;
    host: None (device arrays only), "view" (a numpy array as it is), "copy" (a contiguous copy of one that is not) or "cast" (whatever numpy
    makes a contiguous array of types[0] from - a list included); integer: an object that is no array passes through as a device pointer;
    not_device / wrong_type: what an object that is no (device) array / an element type not allowed raises; empty: see JUDGED."""
    types: Optional[tuple] = FLOATS
    ndim: Optional[int] = None
    dense_from: int = 0
    exact: bool = True
    host: Optional[str] = None
    integer: bool = False
    not_device: type = ValueError
    wrong_type: type = ValueError
    empty: int = JUDGED


_TYPES = {}


def _type(typestr: str):
    """(numpy dtype, bytes per element) of a typestr; the bytes are the typestr's own count (float64 4x4 records and |V32 alike)."""
    got = _TYPES[typestr] = (np.dtype(typestr), int(typestr[2:]))
    return got


def read(a, what: str, need: Need, shape=None, nbytes=None) -> Array:
    """``a`` as an Array, or the exception of the first thing about it that ``need`` does not allow: ``what`` names the argument.  shape: the
    exact shape (None in it: any extent); nbytes: the bytes it must hold (``need.exact``: exactly, else at least)."""
    types, ndim, dense_from, exact, host, integer, not_device, wrong_type, empty = need
    cai, keep = getattr(a, _CAI, None), None
    if cai is not None:
        typestr, got, strides = cai["typestr"], tuple(map(int, cai["shape"])), cai.get("strides")
    elif host == "cast" or (host and isinstance(a, np.ndarray)):
        keep = np.ascontiguousarray(a, dtype=types[0]) if host == "cast" else a
        typestr, got, strides, empty = keep.dtype.str, keep.shape, keep.strides, DIMENSION
    elif integer:
        return Array(C.c_void_p(int(a)), None, (), (), True, None)
    else:
        raise not_device(f"{what}: device arrays only (an object with {_CAI}, e.g. a torch tensor) - got {type(a).__name__}")
    if types is not None and typestr not in types:
        raise wrong_type(f"{what}: {' or '.join(_NAMES.get(t, t) for t in types)} is expected, got {typestr} {got}")
    if (ndim is not None and len(got) != ndim) or (shape is not None and got != shape and not _fits(got, shape)):
        raise ValueError(f"{what}: {f'{ndim} dimensions are' if shape is None else f'the shape {tuple(shape)} is'} expected, got {typestr} {got}")
    if host == "copy" and keep is not None:
        keep = np.ascontiguousarray(keep)
        strides = keep.strides
    dtype, size = _TYPES.get(typestr) or _type(typestr)
    elements, below, total = [0] * len(got), 1, size
    judged = bool(strides) and not (empty == NOTHING and 0 in got)
    for i in range(len(got) - 1, -1, -1):
        extent = got[i]
        if judged and extent != 1 and (extent or empty != DIMENSION):
            stride = strides[i]
            if (stride != below * size) if i >= dense_from else (stride % size or stride < below * size):
                raise ValueError(f"{what}: from dimension {dense_from} on the elements must be contiguous, the dimensions before it a whole number of "
                                 f"elements and at least what they hold apart (shape {got}, strides {tuple(strides)} in bytes of {typestr})")
            below = stride // size
        elements[i] = below
        below *= extent
        total *= extent
    if nbytes is not None and (total != nbytes if exact else total < nbytes):
        raise ValueError(f"{what}: {'' if exact else 'at least '}{nbytes} bytes are expected, got shape {got} of {typestr} ({total} bytes)")
    if keep is not None:
        return Array(keep.ctypes.data_as(C.c_void_p), dtype, got, tuple(elements), False, keep)
    return Array(C.c_void_p(cai["data"][0]), dtype, got, tuple(elements), True, None)


_NAMES = {"<f4": "float32", "<f8": "float64", "<i4": "int32", "<i8": "int64"}


def _fits(got: tuple, shape) -> bool:
    """got is ``shape`` but for the extents ``shape`` leaves open (None)"""
    return len(got) == len(shape) and all(want is None or want == extent for want, extent in zip(shape, got))
