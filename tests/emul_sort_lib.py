"""Test helper: build + bind tests/emul/libtsfa_emul_sort.so, the single-thread g++ build of the SORT family's kernel body
(tsfresh_amd/csrc/fam_sort.h) run through the device's one-wavefront LDS layout (tsfa_layout.h: SortLds), next to emul_lib.py
and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from emul_lib import _Spec

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_sort.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_sort.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_sort_calc_id.argtypes = [ctypes.c_char_p]
    lib.tsfa_emul_sort_calc_id.restype = ctypes.c_int
    lib.tsfa_emul_sort_lds_bytes.argtypes = [ctypes.c_int] * 5
    lib.tsfa_emul_sort_lds_bytes.restype = ctypes.c_longlong
    lib.tsfa_emul_sort_extract.argtypes = [ctypes.POINTER(_Spec), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_char_p, ctypes.c_int]
    lib.tsfa_emul_sort_extract.restype = ctypes.c_int
    _lib = lib
    return lib


def lds_bytes(maxn, xs_bytes, w_doubles, mode, with_np):
    """Bytes of LDS a one-wavefront k_sort launch carves (mode 1: sorted copy, 2: 16-bit order)."""
    return int(load().tsfa_emul_sort_lds_bytes(maxn, xs_bytes, w_doubles, mode, 1 if with_np else 0))


def emul_sort(fc_parameters, values, offsets, mode, own_launch=False, kind="value"):
    """SORT-family columns of a ragged batch (float32 or float64 samples, series of at most 2048) -> (names, matrix)."""
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    lib = load()
    plan = compile_fc_parameters(fc_parameters)
    specs = plan.native_specs(lambda name: lib.tsfa_emul_sort_calc_id(name.encode()))
    arr = (_Spec * max(len(specs), 1))()
    for i, (cid, p) in enumerate(specs):
        arr[i].calc = cid
        for k in range(4):
            arr[i].p[k] = p[k]
    values = np.ascontiguousarray(values)
    assert values.dtype in (np.float32, np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    out = np.empty((n, len(specs)))
    err = ctypes.create_string_buffer(512)
    rc = lib.tsfa_emul_sort_extract(arr, len(specs), values.ctypes.data, 0 if values.dtype == np.float32 else 1,
                                    offsets.ctypes.data, n, mode, 1 if own_launch else 0, out.ctypes.data, len(specs), err, 512)
    if rc != 0:
        raise RuntimeError("emul_sort: %d %s" % (rc, err.value.decode()))
    return [kind + "__" + nm for nm in plan.names], out
