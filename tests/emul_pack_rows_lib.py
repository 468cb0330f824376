"""Test helper: build + bind tests/emul/libtsfa_emul_pack_rows.so, the single-thread g++ build of the row packer's kernel
bodies (tsfresh_amd/csrc/pack_rows.h), next to emul_pack_set_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack_rows.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack_rows.so")
_lib = None

GUARD = 16   # sentinel elements on either side of every output


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.tsfa_emul_pack_rows_geometry.argtypes = [i64] + [ctypes.POINTER(i32)] * 5
    lib.tsfa_emul_pack_rows_geometry.restype = None
    lib.tsfa_emul_pack_rows.argtypes = [vp, i32, vp, i64, i64, i64, i64, vp, vp, i64]
    lib.tsfa_emul_pack_rows.restype = ctypes.c_int
    lib.tsfa_emul_pack_hours.argtypes = [vp, i32, i64, i64, vp, vp, i64, i64, vp, vp, i64]
    lib.tsfa_emul_pack_hours.restype = ctypes.c_int
    _lib = lib
    return lib


def geometry(n_cols=1):
    """-> dict(tile_c, tile_t: the tiles route's tile for n_cols columns; rows_max_grid, hours_tile, hours_max_grid)."""
    out = [ctypes.c_int32() for _ in range(5)]
    load().tsfa_emul_pack_rows_geometry(int(n_cols), *[ctypes.byref(o) for o in out])
    return dict(zip(("tile_c", "tile_t", "rows_max_grid", "hours_tile", "hours_max_grid"), (int(o.value) for o in out)))


def sort_order(ids, sort=None, kinds=None):
    """What a pack set keeps for these key columns, computed with numpy's stable sorts: -> (perm uint32: sorted position ->
    input row, offsets int64 of the (kind, id) groups over the whole sorted frame)."""
    keys = [np.asarray(ids)]
    if sort is not None:
        keys.insert(0, np.asarray(sort))
    if kinds is not None:
        keys.append(np.asarray(kinds))
    perm = np.lexsort(tuple(keys)) if len(keys) > 1 else np.argsort(keys[0], kind="stable")
    sid = np.asarray(ids)[perm]
    head = np.ones(len(perm), dtype=bool)
    head[1:] = sid[1:] != sid[:-1]
    if kinds is not None:
        sk = np.asarray(kinds)[perm]
        head[1:] |= sk[1:] != sk[:-1]
    offsets = np.concatenate([np.nonzero(head)[0], [len(perm)]]).astype(np.int64)
    return perm.astype(np.uint32), offsets


def _guarded(n, dtype, fill):
    buf = np.full(n + 2 * GUARD, fill, dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, fill):
    head, tail = buf[:GUARD], buf[GUARD + n:]
    same = (lambda a: bool(np.all(np.isnan(a)))) if isinstance(fill, float) and fill != fill else (lambda a: bool(np.all(a == fill)))
    return same(head) and same(tail)


class EmulRows:
    """tsfa_pack_set_rows on host arrays.  values: any 1-D or 2-D view (its own strides reach the driver); perm: uint32.
    -> .status (the route, or a negative status), .columns [C, N] of the output dtype, .nan (C bools), .guards_intact."""

    def __init__(self, values, perm, n_workgroups=0):
        lib = load()
        v = values if values.ndim == 2 else values[:, None]
        n, c = v.shape
        assert all(s % v.itemsize == 0 and s >= 0 for s in v.strides)
        sr, sc = (s // v.itemsize for s in v.strides)
        vtype = _native._DEVICE_PACK_TYPES[v.dtype]
        odt = np.float32 if v.dtype == np.float32 else np.float64
        perm = np.ascontiguousarray(perm, dtype=np.uint32)
        obuf, out = _guarded(n * c, odt, -7.25)
        fbuf, flags = _guarded(c, np.uint32, 0xabcdef01)
        flags[:] = 0
        self.status = lib.tsfa_emul_pack_rows(v.ctypes.data, vtype, perm.ctypes.data, n, c, sr, sc, out.ctypes.data,
                                              flags.ctypes.data, int(n_workgroups))
        self.columns = out.reshape(c, n).copy()
        self.nan = flags != 0
        self.guards_intact = _intact(obuf, n * c, -7.25) and _intact(fbuf, c, 0xabcdef01)


class EmulHours:
    """tsfa_pack_set_hours on host arrays.  t: int64 ticks or float64 seconds, any 1-D view; perm / offsets: `sort_order`'s.
    -> .status, .hours float64 [N], .flags, .guards_intact."""

    def __init__(self, t, ticks_per_second, perm, offsets, n_workgroups=0):
        lib = load()
        n = len(perm)
        assert t.ndim == 1 and len(t) == n and t.strides[0] % 8 == 0 and t.strides[0] >= 0
        ttype = _native.TSFA_I64 if t.dtype == np.int64 else _native.TSFA_F64
        perm = np.ascontiguousarray(perm, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        obuf, out = _guarded(n, np.float64, -7.25)
        fbuf, flag = _guarded(1, np.uint32, 0xabcdef01)
        flag[:] = 0
        self.status = lib.tsfa_emul_pack_hours(t.ctypes.data, ttype, int(ticks_per_second), t.strides[0] // 8, perm.ctypes.data,
                                               offsets.ctypes.data, n, len(offsets) - 1, out.ctypes.data, flag.ctypes.data,
                                               int(n_workgroups))
        self.hours = out.copy()
        self.flags = int(flag[0])
        self.guards_intact = _intact(obuf, n, -7.25) and _intact(fbuf, 1, 0xabcdef01)
