"""Test helper: build + bind tests/emul/libtsfa_emul_cwt_links.so, the single-thread g++ build of number_cwt_peaks' two
ridge-line linkers (tsfresh_amd/csrc/fam_cwt.h) fed a relative-maximum mask through the device's LDS layout, next to
emul_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_cwt_links.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_cwt_links.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_cwt_links.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.tsfa_emul_cwt_links.restype = ctypes.c_int
    _lib = lib
    return lib


def links(mask, W, route, derive_w1=False):
    """mask: (W, n) booleans, mask[r, c] = column c is a relative maximum of CWT row r.  route 1: the column linker, 0: the
    general linker.  -> (sorted list of (end column, end row), columns marked as row-0 lines (derive_w1), overflow flag)."""
    lib = load()
    mask = np.asarray(mask, dtype=bool)
    assert mask.shape[0] == W
    n = mask.shape[1]
    bits = np.zeros(n, dtype=np.uint16)
    for r in range(W):
        bits |= (mask[r].astype(np.uint16) << r)
    cap = 3 * n
    col = np.empty(cap, dtype=np.int32)
    row = np.empty(cap, dtype=np.int32)
    out = np.empty(n, dtype=np.uint16)
    ovf = ctypes.c_int(0)
    cnt = lib.tsfa_emul_cwt_links(bits.ctypes.data, n, W, 1 if derive_w1 else 0, route, col.ctypes.data, row.ctypes.data, cap,
                                  out.ctypes.data, ctypes.byref(ovf))
    if cnt < 0:
        raise RuntimeError("emul_cwt_links: n = %d, W = %d, route = %d is not served" % (n, W, route))
    assert np.array_equal(out & np.uint16((1 << W) - 1), bits), "a linker changed the maxima"
    assert not np.any(out & np.uint16(~((1 << W) - 1 | 1 << (W + 1)) & 0xFFFF)), "a linker set a bit that is no mark"
    marks = sorted(int(c) for c in np.nonzero(out & np.uint16(1 << (W + 1)))[0])
    return sorted(zip(col[:cnt].tolist(), row[:cnt].tolist())), marks, bool(ovf.value)
