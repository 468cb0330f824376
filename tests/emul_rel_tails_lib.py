"""Test helper: build + bind tests/emul/libtsfa_emul_rel_tails.so, the g++ build of the p-value tails, the FDR step-up and the
mask compaction (tsfresh_amd/csrc/rel_tails.h), next to emul_roll_dense_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd._native import _CLASS_COL_DTYPE as COL_DTYPE, _REAL_COL_DTYPE as REAL_COL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_rel_tails.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_rel_tails.so")
_lib = None

NONE, MWU_NORMAL, FISHER, KENDALL, HOST_MWU_EXACT, HOST_KS = range(6)
SENTINEL = -7
GUARD = 16          # sentinel cells after the last index


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    i64, f64, i32, ptr = ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p
    lib.tsfa_emul_mwu_normal.argtypes, lib.tsfa_emul_mwu_normal.restype = [f64, i64, i64, f64], f64
    lib.tsfa_emul_kendall.argtypes, lib.tsfa_emul_kendall.restype = [i64, i64, i64, i64, f64, f64, i64, f64, f64], f64
    lib.tsfa_emul_fisher.argtypes, lib.tsfa_emul_fisher.restype = [i64] * 4, f64
    lib.tsfa_emul_tails_classes.argtypes = [ptr, ptr, ptr, ptr, i64, i64, i32, i32, ptr, ptr, ptr]
    lib.tsfa_emul_tails_classes.restype = i64
    lib.tsfa_emul_tails_real.argtypes = [ptr, i64, i64, i64, f64, f64, ptr, ptr, ptr]
    lib.tsfa_emul_tails_real.restype = i64
    lib.tsfa_emul_fdr.argtypes = [ptr, ptr, i64, i32, f64, f64, i32, i32, ptr, ptr, ptr, ptr]
    lib.tsfa_emul_fdr.restype = ctypes.c_int
    lib.tsfa_emul_compact_mask.argtypes, lib.tsfa_emul_compact_mask.restype = [ptr, i64, ptr, i32], i64
    _lib = lib
    return lib


def mwu_normal(rank_sum_1, n1, n2, tie_term):
    return float(load().tsfa_emul_mwu_normal(float(rank_sum_1), int(n1), int(n2), float(tie_term)))


def kendall(n, dis, xtie, ntie, x0, x1, ytie, y0, y1):
    return float(load().tsfa_emul_kendall(int(n), int(dis), int(xtie), int(ntie), float(x0), float(x1), int(ytie), float(y0),
                                          float(y1)))


def fisher(a, b, c, d):
    return float(load().tsfa_emul_fisher(int(a), int(b), int(c), int(d)))


def tails_classes(n_unique, tie_term, rank_sums, hi_counts, class_n, with_ks=False):
    """The class tables from the sweep's statistics -> (p [m, C], route [m, C], type [m], host cells)."""
    m, C = rank_sums.shape
    cols = np.zeros(m, dtype=COL_DTYPE)
    cols["n_unique"], cols["tie_term"] = n_unique, tie_term
    rank_sums = np.ascontiguousarray(rank_sums, dtype=np.float64)
    hi_counts = np.ascontiguousarray(hi_counts, dtype=np.int64)
    class_n = np.ascontiguousarray(class_n, dtype=np.int64)
    p = np.full((m, C), -1.0)
    route = np.full((m, C), 255, dtype=np.uint8)
    typ = np.full(m, 255, dtype=np.uint8)
    n_host = load().tsfa_emul_tails_classes(cols.ctypes.data, rank_sums.ctypes.data, hi_counts.ctypes.data, class_n.ctypes.data,
                                            int(class_n.sum()), m, C, int(with_ks), p.ctypes.data, route.ctypes.data,
                                            typ.ctypes.data)
    return p, route, typ, int(n_host)


def tails_real(cols, n_rows, ytie, y0, y1):
    """The table of a real target from the records of tsfa_relevance_real -> (p [m], route [m], type [m], host cells)."""
    cols = np.ascontiguousarray(cols, dtype=REAL_COL_DTYPE)
    m = cols.shape[0]
    p = np.full(m, -1.0)
    route = np.full(m, 255, dtype=np.uint8)
    typ = np.full(m, 255, dtype=np.uint8)
    n_host = load().tsfa_emul_tails_real(cols.ctypes.data, int(n_rows), m, int(ytie), float(y0), float(y1), p.ctypes.data,
                                         route.ctypes.data, typ.ctypes.data)
    return p, route, typ, int(n_host)


def fdr(p, types, alpha, c_m, n_significant=1, multiclass=False):
    """The emulated tsfa_relevance_fdr on p [m, T] -> (relevant_per_table [m, T], relevant [m], n_significant [m], p_min [m])."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    if p.ndim == 1:
        p = p.reshape(-1, 1)
    m, T = p.shape
    types = np.ascontiguousarray(types, dtype=np.uint8)
    rel_t = np.full((m, T), 255, dtype=np.uint8)
    rel = np.full(m, 255, dtype=np.uint8)
    nsig = np.full(m, -1, dtype=np.int32)
    pmin = np.full(m, -1.0)
    rc = load().tsfa_emul_fdr(p.ctypes.data, types.ctypes.data, m, T, float(alpha), float(c_m), int(n_significant),
                              int(multiclass), rel_t.ctypes.data, rel.ctypes.data, nsig.ctypes.data, pmin.ctypes.data)
    assert rc == 0, rc
    return rel_t.astype(bool), rel.astype(bool), nsig, pmin


def compact(mask, nt=1024):
    """The emulated tsfa_compact_mask -> the ascending indices; the GUARD cells after the last index must keep their sentinel."""
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    n = mask.shape[0]
    out = np.full(int(mask.astype(bool).sum()) + GUARD, SENTINEL, dtype=np.int32)
    count = int(load().tsfa_emul_compact_mask(mask.ctypes.data, n, out.ctypes.data, int(nt)))
    assert (out[count:] == SENTINEL).all(), "a cell after the last index was written"
    return out[:count].copy()
