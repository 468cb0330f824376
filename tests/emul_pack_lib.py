"""Test helper: build + bind tests/emul/libtsfa_emul_pack.so, the single-thread g++ build of the device packer's kernel
bodies (tsfresh_amd/csrc/pack_device.h), next to emul_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_pack_tile.restype = ctypes.c_int
    lib.tsfa_emul_pack.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                   ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    lib.tsfa_emul_pack.restype = ctypes.c_int
    _lib = lib
    return lib


def tile():
    return int(load().tsfa_emul_pack_tile())


class EmulPack:
    """Stands in for tsfresh_amd._native.DevicePack: the same columns in (what `_native.pack_column` returns), the same
    attributes out, the g++ build of the kernel bodies behind it."""

    def __init__(self, ids, sort, values, device=0, keep_sort=True):
        lib = load()
        (ids_a, ids_t), (val_a, val_t) = ids, values
        sort_a, sort_t = sort if sort is not None else (None, 0)
        n = len(ids_a)
        out_values = np.empty(n, dtype=np.float64)   # float32 results use the first half
        offsets = np.empty(n + 1, dtype=np.int64)
        uniq = np.empty(n, dtype=ids_a.dtype)
        out_sort = None if sort_a is None else np.empty(n, dtype=sort_a.dtype)
        out_type, flags, passes, groups = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        rc = lib.tsfa_emul_pack(ids_a.ctypes.data, ids_t, None if sort_a is None else sort_a.ctypes.data, sort_t,
                                val_a.ctypes.data, val_t, n, out_values.ctypes.data, ctypes.byref(out_type),
                                offsets.ctypes.data, uniq.ctypes.data, None if out_sort is None else out_sort.ctypes.data,
                                ctypes.byref(groups), ctypes.byref(flags), ctypes.byref(passes))
        if rc != 0:
            raise ValueError("the emulated packer refuses these columns")
        self.n_rows, self.n_series = n, int(groups.value)
        self.flags, self.n_passes = int(flags.value), int(passes.value)
        self.values_dtype = np.dtype(np.float32 if out_type.value == _native.TSFA_F32 else np.float64)
        self._values = out_values.view(self.values_dtype)[:n].copy()
        self.ids = uniq[:self.n_series].copy()
        self.offsets = offsets[:self.n_series + 1].copy()
        self.sort = out_sort

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
