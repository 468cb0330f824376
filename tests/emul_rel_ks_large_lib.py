"""Test helper: build + bind tests/emul/libtsfa_emul_rel_ks_large.so, the g++ build of the Kolmogorov-Smirnov tail beyond
10 000 rows (tsfresh_amd/csrc/rel_ks_large.h), next to emul_rel_ks_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_rel_ks_large.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_rel_ks_large.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    i64, i32, ptr = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    lib.tsfa_emul_ksl_run.argtypes, lib.tsfa_emul_ksl_run.restype = [], i32
    lib.tsfa_emul_ks_large_tails.argtypes, lib.tsfa_emul_ks_large_tails.restype = [ptr, ptr, ptr, i64, ptr, ptr], i64
    _lib = lib
    return lib


def run_length():
    return int(load().tsfa_emul_ksl_run())


def ks_large_tails(n1, n2, d):
    """The emulated tsfa_ks_large_tails -> (p, route, cells left to the host)."""
    n1 = np.ascontiguousarray(n1, dtype=np.int64)
    n2 = np.ascontiguousarray(n2, dtype=np.int64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    k = n1.shape[0]
    p = np.full(k, -1.0)
    route = np.full(k, 255, dtype=np.uint8)
    left = load().tsfa_emul_ks_large_tails(n1.ctypes.data, n2.ctypes.data, d.ctypes.data, k, p.ctypes.data, route.ctypes.data)
    return p, route, int(left)
