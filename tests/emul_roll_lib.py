"""Test helper: build + bind tests/emul/libtsfa_emul_roll.so, the single-thread g++ build of the window builder's kernel
bodies (tsfresh_amd/csrc/roll_device.h), next to emul_pack_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_roll.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_roll.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_roll.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64,
                                   ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.tsfa_emul_roll.restype = ctypes.c_int64
    _lib = lib
    return lib


def roll(lengths, rolling_direction, max_timeshift, min_timeshift, steps, sort=None):
    """The emulated tsfa_roll_windows on series of the given lengths packed back to back, first row at 0.
    -> (series, frm, until, ts) as roll_views returns them (+ the shift values when `sort`, the packed sort column, is given),
    or the negative tsfa_status the builder refuses the arguments with."""
    lib = load()
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    cap = max(int(offsets[-1]), 1)
    starts, ends, series, shifts = (np.full(cap, -7, dtype=np.int64) for _ in range(4))
    sort_ptr, sort_type, sv = None, 0, None
    if sort is not None:
        sort, sort_type = _native.pack_column(np.asarray(sort))
        sv = np.zeros(cap, dtype=sort.dtype)
        sort_ptr = sort.ctypes.data
    n = lib.tsfa_emul_roll(offsets.ctypes.data, len(lengths), int(rolling_direction), int(max_timeshift or 0),
                           int(min_timeshift), int(steps), starts.ctypes.data, ends.ctypes.data, series.ctypes.data,
                           shifts.ctypes.data, sort_ptr, sort_type, None if sv is None else sv.ctypes.data)
    if n < 0:
        return int(n)
    assert n <= cap and np.all(starts[n:] == -7) and np.all(ends[n:] == -7)   # nothing is written past the last window
    base = offsets[series[:n]]
    out = (series[:n].copy(), starts[:n] - base, ends[:n] - base, shifts[:n].copy())
    return out if sv is None else out + (sv[:n],)


class EmulWindows:
    """Stands in for tsfresh_amd._native.DeviceWindows over an EmulPack / EmulKindPack: the same arguments in, the same
    attributes out, the g++ build of the kernel bodies behind it."""

    def __init__(self, pack, rolling_direction=1, max_timeshift=None, min_timeshift=0, steps=None):
        offsets = np.asarray(pack.offsets, dtype=np.int64)
        lengths = np.diff(offsets)
        if steps is None:
            steps = int(lengths.max())
        sort = getattr(pack, "sort", None)
        got = roll(lengths, rolling_direction, max_timeshift, min_timeshift, steps, sort=sort)
        if isinstance(got, int):
            raise _native.NativeError(got, "the emulated window builder refuses these arguments")
        self.series, frm, until, self.timeshifts = got[:4]
        self.starts, self.ends = offsets[self.series] + frm, offsets[self.series] + until
        self._shift_values = got[4].view(sort.dtype) if sort is not None else None
        self.n_windows, self.device, self.rolling_direction = len(self.series), 0, int(rolling_direction)

    def shift_values(self):
        if self._shift_values is None:
            raise ValueError("the pack holds no sort column")
        return self._shift_values

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
