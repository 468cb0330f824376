"""Test helper: build + bind tests/emul/libtsfa_emul_roll_dense.so, the g++ build of tsfa_roll_count / tsfa_roll_fill's host
checks and kernel bodies (tsfresh_amd/csrc/roll_device.h), next to emul_roll_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_roll_dense.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_roll_dense.so")
_lib = None

SENTINEL = -7
GUARD = 16          # sentinel cells after the last window of every output array


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_roll_count.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                         ctypes.c_int64]
    lib.tsfa_emul_roll_count.restype = ctypes.c_int
    lib.tsfa_emul_roll_fill.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [
                                            ctypes.c_int64]
    lib.tsfa_emul_roll_fill.restype = ctypes.c_int
    _lib = lib
    return lib


def count(offsets, n_series, rolling_direction, max_timeshift, min_timeshift, steps, scanned=None, series_len=0, grid=3):
    """The emulated tsfa_roll_count -> (status, n_windows).  offsets: int64 array or None; scanned: uint32 array of n_series
    (the ragged route: it receives the exclusive scan of the counts) or None (the uniform route)."""
    total = ctypes.c_int64(-1)
    rc = load().tsfa_emul_roll_count(None if offsets is None else offsets.ctypes.data, int(n_series), int(series_len),
                                     int(rolling_direction), int(max_timeshift or 0), int(min_timeshift), int(steps),
                                     None if scanned is None else scanned.ctypes.data, ctypes.byref(total), grid)
    return int(rc), int(total.value)


def fill(offsets, n_series, n_windows, out, rolling_direction, max_timeshift, min_timeshift, steps, scanned=None, series_len=0,
         grid=3):
    """The emulated tsfa_roll_fill into the rows of `out` (int64 [4, >= n_windows]: starts, ends, series, timeshifts) ->
    status."""
    return int(load().tsfa_emul_roll_fill(
        None if offsets is None else offsets.ctypes.data, int(n_series), None if scanned is None else scanned.ctypes.data,
        int(series_len), int(n_windows), int(rolling_direction), int(max_timeshift or 0), int(min_timeshift), int(steps),
        out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, grid))


def windows(lengths, rolling_direction, max_timeshift, min_timeshift, steps, uniform=False, base=0, grid=3):
    """Both calls on series of the given lengths packed back to back from row `base` on -> (starts, ends, series,
    timeshifts) of n_windows entries each, or the negative tsfa_status of the call that refused.  uniform: take the
    closed-form route (the lengths must be equal).  The GUARD cells after the last window of every array must keep their
    sentinel."""
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.full(len(lengths) + 1, base, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    offsets[1:] += base
    scanned, series_len = None, 0
    if uniform:
        assert len(set(lengths.tolist())) == 1
        series_len = int(lengths[0])
    else:
        scanned = np.zeros(len(lengths), dtype=np.uint32)
    kw = dict(scanned=scanned, series_len=series_len, grid=grid)
    rc, n = count(offsets, len(lengths), rolling_direction, max_timeshift, min_timeshift, steps, **kw)
    if rc:
        return rc
    out = np.full((4, n + GUARD), SENTINEL, dtype=np.int64)
    rc = fill(offsets, len(lengths), n, out, rolling_direction, max_timeshift, min_timeshift, steps, **kw)
    if rc:
        return rc
    assert (out[:, n:] == SENTINEL).all(), "a cell after the last window was written"
    return tuple(out[k, :n].copy() for k in range(4))
