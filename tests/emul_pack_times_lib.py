"""Test helper: build + bind tests/emul/libtsfa_emul_pack_times.so, the single-thread g++ build of the times packer's kernel
body (tsfresh_amd/csrc/pack_times.h), next to emul_pack_dense_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack_times.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack_times.so")
_lib = None

GUARD = 64          # sentinel cells on either side of hours_out
SENTINEL = -7.25e300
TICKS_PER_SECOND = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_pack_times_chunk.argtypes, lib.tsfa_emul_pack_times_chunk.restype = [], ctypes.c_int
    lib.tsfa_emul_pack_times.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_int64] * 5 + [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    lib.tsfa_emul_pack_times.restype = ctypes.c_int
    _lib = lib
    return lib


def row_chunk():
    """Stamps of one work item."""
    return int(load().tsfa_emul_pack_times_chunk())


def raw(t_ptr, t_type, ticks_per_second, n_batch, n_time, sb, st, offsets_ptr, hours_ptr, flags_ptr, grid=3):
    """The emulated call on raw addresses (ints, 0 for NULL) -> its status."""
    return int(load().tsfa_emul_pack_times(t_ptr or None, t_type, ticks_per_second, n_batch, n_time, sb, st, offsets_ptr or None,
                                           hours_ptr or None, flags_ptr or None, grid))


class EmulTimes:
    """One emulated tsfa_pack_times call on the strided numpy view `t` of logical shape (B, n): int64 ticks (`unit` one of
    "s", "ms", "us", "ns"), datetime64 of those units (viewed as int64, the unit taken from the dtype) or float64 seconds, any
    strides numpy can express without a negative one, stride 0 included.  `offsets`: int64[B + 1], as the dense packer wrote
    them.  `hours`: float64[T], `flags`, `status`; `guards_intact`: the sentinel cells before offsets[0] and from
    offsets[B] on, and the words around the flag word, are untouched."""

    def __init__(self, t, offsets, unit="ns", grid=3, flags=0):
        assert t.ndim == 2
        if t.dtype.kind == "M":
            unit = np.datetime_data(t.dtype)[0]
            t = t.view(np.int64)
        B, n = t.shape
        assert all(s % 8 == 0 and s >= 0 for s in t.strides)
        sb, st = (s // 8 for s in t.strides)
        t_type = {np.dtype(np.int64): _native.TSFA_I64, np.dtype(np.float64): _native.TSFA_F64}[t.dtype]
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        assert offsets.shape == (B + 1,) and offsets[0] == 0
        T = int(offsets[-1])
        out = np.full(T + 2 * GUARD, SENTINEL, dtype=np.float64)
        word = np.array([0, flags, 0], dtype=np.int32)
        self.status = raw(t.ctypes.data, t_type, TICKS_PER_SECOND[unit], B, n, sb, st, offsets.ctypes.data,
                          out[GUARD:].ctypes.data, word[1:].ctypes.data, grid)
        self.flags = int(word[1])
        if self.status != _native.TSFA_OK:
            return
        self.hours = out[GUARD:GUARD + T].copy()
        self.guards_intact = bool((out[:GUARD] == SENTINEL).all() and (out[GUARD + T:] == SENTINEL).all()
                                  and word[0] == 0 and word[2] == 0)

    @property
    def bad_time(self):
        return bool(self.flags & _native.TSFA_DENSE_BAD_TIME)
