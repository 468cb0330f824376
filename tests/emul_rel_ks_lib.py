"""Test helper: build + bind tests/emul/libtsfa_emul_rel_ks.so, the g++ build of the exact Kolmogorov-Smirnov tail
(tsfresh_amd/csrc/rel_ks.h), next to emul_rel_tails_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd._native import _REAL_COL_DTYPE as REAL_COL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_rel_ks.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_rel_ks.so")
_lib = None

HOST_KS, KS_EXACT = 5, 6
ANY, LDS, SCRATCH = 0, 1, 2   # the ring of tsfa_emul_ks_lattice: the driver's choice, the LDS slice, the scratch slice


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    i64, f64, i32, ptr = ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p
    lib.tsfa_emul_ks_ring_chunks.argtypes, lib.tsfa_emul_ks_ring_chunks.restype = [i64] * 4, i64
    lib.tsfa_emul_ks_lds_chunks.argtypes, lib.tsfa_emul_ks_lds_chunks.restype = [], i32
    lib.tsfa_emul_ks_lattice.argtypes, lib.tsfa_emul_ks_lattice.restype = [i64, i64, i64, i64, i32], f64
    lib.tsfa_emul_ks_stage.argtypes = [ptr, ptr, ptr, ptr, i64, i32, ptr, i64, ptr, ptr]
    lib.tsfa_emul_ks_stage.restype = i64
    lib.tsfa_emul_ks_tails.argtypes, lib.tsfa_emul_ks_tails.restype = [ptr, ptr, ptr, i64, ptr, ptr], i64
    _lib = lib
    return lib


def ring_chunks(m, n, g, h):
    return int(load().tsfa_emul_ks_ring_chunks(int(m), int(n), int(g), int(h)))


def lds_chunks():
    return int(load().tsfa_emul_ks_lds_chunks())


def lattice(m, n, g, h, storage=ANY):
    """rk_ks_lattice(m, n, g, h) on a ring that starts out as NaN; -1.0 when the ring asked for is too small."""
    return float(load().tsfa_emul_ks_lattice(int(m), int(n), int(g), int(h), int(storage)))


def ks_tails(n1, n2, d):
    """The emulated tsfa_ks_tails -> (p, route, cells left to the host)."""
    n1 = np.ascontiguousarray(n1, dtype=np.int64)
    n2 = np.ascontiguousarray(n2, dtype=np.int64)
    d = np.ascontiguousarray(d, dtype=np.float64)
    k = n1.shape[0]
    p = np.full(k, -1.0)
    route = np.full(k, 255, dtype=np.uint8)
    left = load().tsfa_emul_ks_tails(n1.ctypes.data, n2.ctypes.data, d.ctypes.data, k, p.ctypes.data, route.ctypes.data)
    return p, route, int(left)


def ks_stage_classes(class_n, ks_d, p, route):
    """The Kolmogorov-Smirnov stage on class tables whose route bytes rel_tails.h wrote (p, route: [m, C], changed in place)
    -> the cells served."""
    class_n = np.ascontiguousarray(class_n, dtype=np.int64)
    ks_d = np.ascontiguousarray(ks_d, dtype=np.float64)
    assert p.flags.c_contiguous and route.flags.c_contiguous and p.shape == route.shape == ks_d.shape
    return int(load().tsfa_emul_ks_stage(None, None, ks_d.ctypes.data, class_n.ctypes.data, int(class_n.sum()), class_n.shape[0], None,
                                         p.size, p.ctypes.data, route.ctypes.data))


def ks_stage_real(cols, n_rows, p, route):
    """The same on the table of a real target (cols: the records of tsfa_relevance_real; p, route: [m])."""
    cols = np.ascontiguousarray(cols, dtype=REAL_COL_DTYPE)
    assert p.flags.c_contiguous and route.flags.c_contiguous and p.shape == route.shape == cols.shape
    return int(load().tsfa_emul_ks_stage(None, None, None, None, int(n_rows), 0, cols.ctypes.data, p.size, p.ctypes.data,
                                         route.ctypes.data))
