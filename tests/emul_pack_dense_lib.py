"""Test helper: build + bind tests/emul/libtsfa_emul_pack_dense.so, the single-thread g++ build of the dense packer's kernel
bodies (tsfresh_amd/csrc/pack_dense.h), next to emul_pack_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack_dense.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack_dense.so")
_lib = None

ROUTE_ROWS_UNIT, ROUTE_TRANSPOSE, ROUTE_ROWS = 0, 1, 2
GUARD = 64          # sentinel cells on either side of the output buffers
_OUT_SENTINEL = 0x5A


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_pack_dense_tile.argtypes, lib.tsfa_emul_pack_dense_tile.restype = [ctypes.c_int, ctypes.c_int64], ctypes.c_int
    for name in ("tsfa_emul_f16_to_f32_bits", "tsfa_emul_bf16_to_f32_bits"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [ctypes.c_uint32], ctypes.c_uint32
    lib.tsfa_emul_pack_dense.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_int64] * 6 + [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int32)]
    lib.tsfa_emul_pack_dense.restype = ctypes.c_int
    _lib = lib
    return lib


def tile_t(n_channels):
    """Time steps of one LDS tile of the transpose route for an array of n_channels (the tile holds a fixed number of
    samples: fewer channels, more time steps)."""
    return int(load().tsfa_emul_pack_dense_tile(0, n_channels))


def tile_c():
    """Most channels of one LDS tile."""
    return int(load().tsfa_emul_pack_dense_tile(1, 0))


def row_chunk():
    """Samples of one work item of the rows routes."""
    return int(load().tsfa_emul_pack_dense_tile(2, 0))


def vec():
    """Most samples a lane moves in one step of the aligned unit-stride copy (the half types'; half of it for the others)."""
    return int(load().tsfa_emul_pack_dense_tile(3, 0))


def n_grid(n_channels):
    """The smallest series lengths that straddle the edges: of a lane's step in the aligned copy (either width), and of the
    LDS tile for n_channels."""
    tt = tile_t(n_channels)
    v = vec()
    return sorted({1, v // 2 - 1, v // 2, v // 2 + 1, v - 1, v, v + 1, tt - 1, tt, tt + 1, 2 * tt + 3})


def x_type_of(a, bf16=False):
    """tsfa_dtype of a numpy array; bfloat16 travels as uint16 bit patterns with bf16=True."""
    if bf16:
        assert a.dtype == np.uint16
        return _native.TSFA_BF16
    return {np.dtype(np.float64): _native.TSFA_F64, np.dtype(np.float32): _native.TSFA_F32,
            np.dtype(np.float16): _native.TSFA_F16}[a.dtype]


class EmulDense:
    """One emulated tsfa_pack_dense call on the strided numpy view `x` of logical shape (B, C, n) (any strides numpy can
    express, stride 0 included).  `values`: [C, T] in the output dtype, `offsets`: int64[B + 1], `flags`, `route`,
    `status`; `guards_intact`: the sentinel cells around the value buffer, between T and the channel stride inside it, and
    around the offsets are untouched."""

    def __init__(self, x, lengths=None, bf16=False, grid=3, channel_stride_out=None):
        lib = load()
        assert x.ndim == 3
        B, C, n = x.shape
        isz = x.dtype.itemsize
        assert all(s % isz == 0 and s >= 0 for s in x.strides)
        sb, sc, st = (s // isz for s in x.strides)
        x_type = x_type_of(x, bf16)
        out_dtype = np.dtype(np.float64 if x_type == _native.TSFA_F64 else np.float32)
        cso = B * n if channel_stride_out is None else int(channel_stride_out)
        raw = np.full((C * max(cso, 0) + 2 * GUARD) * out_dtype.itemsize, _OUT_SENTINEL, dtype=np.uint8)
        out = raw.view(out_dtype)
        offs = np.full(B + 1 + 2 * GUARD, -12345, dtype=np.int64)
        flags = np.zeros(3, dtype=np.int32)
        route = ctypes.c_int32(-1)
        lptr, ltype = None, 0
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths)
            ltype = {np.dtype(np.int32): _native.TSFA_I32, np.dtype(np.int64): _native.TSFA_I64}[lengths.dtype]
            lptr = lengths.ctypes.data
        self.status = lib.tsfa_emul_pack_dense(
            x.ctypes.data, x_type, B, C, n, sb, sc, st, lptr, ltype, out[GUARD:].ctypes.data, cso, offs[GUARD:].ctypes.data,
            flags[1:].ctypes.data, grid, ctypes.byref(route))
        self.route, self.flags = int(route.value), int(flags[1])
        self.out_dtype = out_dtype
        if self.status != _native.TSFA_OK:
            return
        self.offsets = offs[GUARD:GUARD + B + 1].copy()
        T = int(self.offsets[-1])
        body = out[GUARD:GUARD + C * cso].reshape(C, cso)
        self.values = body[:, :T].copy()
        sent = np.full(1, _OUT_SENTINEL, dtype=np.uint8).repeat(out_dtype.itemsize).view(out_dtype)[0]
        as_bits = np.dtype("u%d" % out_dtype.itemsize)
        self.guards_intact = bool(
            (out[:GUARD].view(as_bits) == sent.view(as_bits)).all() and (out[GUARD + C * cso:].view(as_bits) == sent.view(as_bits)).all()
            and (body[:, T:].view(as_bits) == sent.view(as_bits)).all()
            and (offs[:GUARD] == -12345).all() and (offs[GUARD + B + 1:] == -12345).all()
            and flags[0] == 0 and flags[2] == 0)

    @property
    def value_nan(self):
        return bool(self.flags & _native.TSFA_PACK_VALUE_NAN)

    @property
    def bad_length(self):
        return bool(self.flags & _native.TSFA_DENSE_BAD_LENGTH)
