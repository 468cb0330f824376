"""Test helper: build + bind tests/emul/libtsfa_emul_mprofile.so, the single-thread g++ build of k_mprofile's body
(tsfresh_amd/csrc/fam_mprofile.h), next to emul_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_mprofile.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_mprofile.so")
_lib = None

FEATURE_CODE = {"min": 0, "max": 1, "mean": 2, "median": 3, "25": 4, "75": 5}


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_mprofile.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_void_p]
    lib.tsfa_emul_mprofile.restype = ctypes.c_int
    lib.tsfa_emul_mprofile_restart.restype = ctypes.c_int
    lib.tsfa_emul_mprofile_lds_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.tsfa_emul_mprofile_lds_bytes.restype = ctypes.c_longlong
    lib.tsfa_emul_mprofile_lds_limit.restype = ctypes.c_longlong
    _lib = lib
    return lib


def restart_stride():
    return int(load().tsfa_emul_mprofile_restart())


def longest_in_lds(xs_bytes):
    """The longest series whose working set (tsfa_layout.h: MpLds) fits a workgroup's LDS; longer ones take HBM scratch."""
    lib = load()
    n = 1
    while lib.tsfa_emul_mprofile_lds_bytes(n + 1, xs_bytes) <= lib.tsfa_emul_mprofile_lds_limit():
        n += 1
    return n


def emul_mprofile(columns, values, offsets):
    """columns: [(windows, feature name)]; values: float32 or float64 samples of the ragged batch -> [n_series x len(columns)]."""
    lib = load()
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.float32, np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    params = np.array([[w, FEATURE_CODE[f]] for w, f in columns], dtype=np.float64).reshape(-1)
    out = np.full((len(offsets) - 1, len(columns)), -12345.0)
    rc = lib.tsfa_emul_mprofile(params.ctypes.data, len(columns), values.ctypes.data, 0 if values.dtype == np.float32 else 1,
                                offsets.ctypes.data, len(offsets) - 1, out.ctypes.data)
    if rc != 0:
        raise ValueError("the emulated kernel refuses these columns")
    return out
