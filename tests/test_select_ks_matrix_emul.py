"""ks_tail="device_matrix" without a GPU: the option's code and constants, and the g++ build of the kernel bodies of
csrc/rel_ks_matrix.h (tests/emul/emul_rel_ks_matrix.cpp: lanes looped) on the table of tests/ks_matrix_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import emul_build
import ks_matrix_cases as cases
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_matrix_is_a_value_of_ks_tail_with_the_headers_codes():
    assert _native._tail_code("ks_tail", "device_matrix") == 3
    with pytest.raises(ValueError, match="mwu_tail"):
        _native._tail_code("mwu_tail", "device_matrix")
    assert (_native.TSFA_KS_TAIL_DEVICE_MATRIX, _native.TSFA_ROUTE_KS_MATRIX) == (3, 9)   # include/tsfresh_amd.h
    assert _native.PROTOTYPES["tsfa_ks_matrix_tails"] == _native.PROTOTYPES["tsfa_ks_large_tails"]


def test_emulated_matrix_tails_meet_the_bar_on_triples():
    lib_path = os.path.join(HERE, "emul", "libtsfa_emul_rel_ks_matrix.so")
    emul_build.build(os.path.join(HERE, "emul", "emul_rel_ks_matrix.cpp"), lib_path)
    run = ctypes.CDLL(lib_path).tsfa_emul_ks_matrix_tails
    run.argtypes, run.restype = [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 2, ctypes.c_int64
    k = len(cases.CASES)
    p, route = np.full(k, -1.0), np.full(k, 255, dtype=np.uint8)
    left = run(cases.N1.ctypes.data, cases.N2.ctypes.data, cases.D.ctypes.data, k, p.ctypes.data, route.ctypes.data)
    assert left == int((route == cases.HOST_KS).sum())
    cases.check(p, route, skip=lambda case: case[0][0] * case[0][1] / sum(case[0]) > 140.5)   # n >= 141: the MFMA kernel, no emulation
