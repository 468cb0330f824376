"""Test helper: build + bind tests/emul/libtsfa_emul_rel_mwu.so, the g++ build of the exact Mann-Whitney tail
(tsfresh_amd/csrc/rel_mwu.h), next to emul_rel_ks_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_rel_mwu.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_rel_mwu.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    i64, i32, ptr = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    lib.tsfa_emul_mwu_lds_elems.argtypes, lib.tsfa_emul_mwu_lds_elems.restype = [], i32
    lib.tsfa_emul_mwu_served.argtypes, lib.tsfa_emul_mwu_served.restype = [i64, i64], i32
    lib.tsfa_emul_mwu_stage.argtypes, lib.tsfa_emul_mwu_stage.restype = [ptr, ptr, i32, ptr, ptr, ptr, i64, i64, ptr, ptr], i64
    _lib = lib
    return lib


def lds_elems():
    return int(load().tsfa_emul_mwu_lds_elems())


def served(n1, n2):
    return bool(load().tsfa_emul_mwu_served(int(n1), int(n2)))


def mwu_tails(n1, n2, table, u, p, route):
    """The emulated tsfa_mwu_tails on the caller's p (float64) and route (uint8), changed in place -> the cells served."""
    n1 = np.ascontiguousarray(n1, dtype=np.int64)
    n2 = np.ascontiguousarray(n2, dtype=np.int64)
    table = np.ascontiguousarray(table, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64)
    assert p.flags.c_contiguous and route.flags.c_contiguous and p.shape == route.shape == u.shape == table.shape
    return int(load().tsfa_emul_mwu_stage(n1.ctypes.data, n2.ctypes.data, n1.shape[0], table.ctypes.data, u.ctypes.data, None, 0,
                                          p.size, p.ctypes.data, route.ctypes.data))


def mwu_stage_classes(class_n, rank_sums, p, route):
    """The Mann-Whitney stage on class tables whose route bytes rel_tails.h wrote (p, route, rank_sums: [m, C]; p and route
    changed in place) -> the cells served."""
    class_n = np.ascontiguousarray(class_n, dtype=np.int64)
    rest = np.ascontiguousarray(class_n.sum() - class_n)
    rank_sums = np.ascontiguousarray(rank_sums, dtype=np.float64)
    assert p.flags.c_contiguous and route.flags.c_contiguous and p.shape == route.shape == rank_sums.shape
    return int(load().tsfa_emul_mwu_stage(class_n.ctypes.data, rest.ctypes.data, class_n.shape[0], None, None, rank_sums.ctypes.data,
                                          int(class_n.sum()), p.size, p.ctypes.data, route.ctypes.data))
