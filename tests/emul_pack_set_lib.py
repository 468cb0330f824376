"""Test helper: build + bind tests/emul/libtsfa_emul_pack_set.so, the single-thread g++ build of the pack set's kernel bodies
(tsfresh_amd/csrc/pack_device.h), next to emul_pack_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack_set.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack_set.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.tsfa_emul_pack_set_tile.restype = ctypes.c_int
    lib.tsfa_emul_pack_set_create.argtypes = [vp, i32, vp, i32, vp, i32, i64, i32]
    lib.tsfa_emul_pack_set_create.restype = vp
    lib.tsfa_emul_pack_set_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32),
                                            ctypes.POINTER(i32)]
    lib.tsfa_emul_pack_set_info.restype = None
    lib.tsfa_emul_pack_set_ranges.argtypes = [vp, vp, vp, vp]
    lib.tsfa_emul_pack_set_ranges.restype = None
    lib.tsfa_emul_pack_set_kind.argtypes = [vp, i64, vp, vp, vp]
    lib.tsfa_emul_pack_set_kind.restype = None
    lib.tsfa_emul_pack_set_values.argtypes = [vp, vp, i32, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.tsfa_emul_pack_set_values.restype = ctypes.c_int
    lib.tsfa_emul_pack_set_destroy.argtypes = [vp]
    lib.tsfa_emul_pack_set_destroy.restype = None
    _lib = lib
    return lib


def tile():
    return int(load().tsfa_emul_pack_set_tile())


class EmulKindPack:
    """Stands in for the DevicePack views a DevicePackSet hands out."""

    def __init__(self, values, offsets, ids, sort, flags, n_passes):
        self._values, self.offsets, self.ids, self.sort = values, offsets, ids, sort
        self.n_rows, self.n_series = len(values), len(ids)
        self.values_dtype = values.dtype
        self.flags, self.n_passes = flags, n_passes
        self.device = 0

    @property
    def value_nan(self):
        return bool(self.flags & _native.TSFA_PACK_VALUE_NAN)

    @property
    def was_in_order(self):
        return bool(self.flags & _native.TSFA_PACK_IN_ORDER)

    def values_host(self):
        return self._values

    def close(self):
        pass


class EmulPackSet:
    """Stands in for tsfresh_amd._native.DevicePackSet: the same columns in (what `_native.pack_column` returns), the same
    attributes out, the g++ build of the kernel bodies behind it."""

    def __init__(self, ids, sort, kinds, device=0, keep_sort=False):
        lib = load()
        ids_a, ids_t = ids
        sort_a, sort_t = sort if sort is not None else (None, 0)
        kind_a, kind_t = kinds if kinds is not None else (None, 0)
        self._lib, self.device, self.n_rows = lib, device, len(ids_a)
        self._h = lib.tsfa_emul_pack_set_create(ids_a.ctypes.data, ids_t, None if sort_a is None else sort_a.ctypes.data,
                                                sort_t, None if kind_a is None else kind_a.ctypes.data, kind_t,
                                                len(ids_a), 1 if keep_sort else 0)
        if not self._h:
            raise ValueError("the emulated pack set refuses these columns")
        groups, kinds_n, flags, passes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        lib.tsfa_emul_pack_set_info(self._h, ctypes.byref(groups), ctypes.byref(kinds_n), ctypes.byref(flags),
                                    ctypes.byref(passes))
        self.n_groups, self.n_kinds = int(groups.value), int(kinds_n.value)
        self.flags, self.n_passes = int(flags.value), int(passes.value)
        self._rows = np.empty(self.n_kinds + 1, dtype=np.int64)
        self._groups = np.empty(self.n_kinds + 1, dtype=np.int64)
        self.kinds = None if kind_a is None else np.empty(self.n_kinds, dtype=kind_a.dtype)
        lib.tsfa_emul_pack_set_ranges(self._h, self._rows.ctypes.data, self._groups.ctypes.data,
                                      None if self.kinds is None else self.kinds.ctypes.data)
        self._ids_dtype = ids_a.dtype
        self._sort_dtype = None if sort_a is None or not keep_sort else sort_a.dtype

    @property
    def was_in_order(self):
        return bool(self.flags & _native.TSFA_PACK_IN_ORDER)

    def values(self, column):
        val_a, val_t = column
        assert len(val_a) == self.n_rows
        out = np.empty(self.n_rows, dtype=np.float64)   # float32 results use the first half
        out_type, nan = ctypes.c_int32(), ctypes.c_int32()
        rc = self._lib.tsfa_emul_pack_set_values(self._h, val_a.ctypes.data, val_t, out.ctypes.data, ctypes.byref(out_type),
                                                 ctypes.byref(nan))
        if rc != 0:
            raise ValueError("the emulated pack set refuses this value column")
        dtype = np.dtype(np.float32 if out_type.value == _native.TSFA_F32 else np.float64)
        gathered = out.view(dtype)[:self.n_rows].copy()
        flags = self.flags | (_native.TSFA_PACK_VALUE_NAN if nan.value else 0)
        packs = []
        for k in range(self.n_kinds):
            r0, r1, g0, g1 = self._rows[k], self._rows[k + 1], self._groups[k], self._groups[k + 1]
            offsets = np.empty(g1 - g0 + 1, dtype=np.int64)
            ids = np.empty(g1 - g0, dtype=self._ids_dtype)
            sort = None if self._sort_dtype is None else np.empty(r1 - r0, dtype=self._sort_dtype)
            self._lib.tsfa_emul_pack_set_kind(self._h, k, offsets.ctypes.data, ids.ctypes.data,
                                              None if sort is None else sort.ctypes.data)
            packs.append(EmulKindPack(gathered[r0:r1], offsets, ids, sort, flags, self.n_passes))
        return packs

    def close(self):
        if self._h:
            self._lib.tsfa_emul_pack_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()
