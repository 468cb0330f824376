"""Test helper: build + bind tests/emul/libtsfa_emul_pack_valid.so, the g++ build of the valid-step packer's kernel bodies
(tsfresh_amd/csrc/pack_valid.h) with the 64 lanes of a wavefront looped, next to emul_pack_times_lib.py and with its recipe.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import ctypes
import os

import numpy as np

import emul_build
import emul_pack_dense_lib as epd
import emul_pack_times_lib as ept
from tsfresh_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "emul_pack_valid.cpp")
LIB = os.path.join(HERE, "emul", "libtsfa_emul_pack_valid.so")
_lib = None

GUARD = 64                 # sentinel cells on either side of every output
OUT_SENTINEL = 0xA5        # every byte of the value buffer before the call
STEP_SENTINEL = -77
STAMP_SENTINEL = -5555555555
OFFSET_SENTINEL = -12345


def load():
    global _lib
    if _lib is not None:
        return _lib
    emul_build.build(SRC, LIB)
    lib = ctypes.CDLL(LIB)
    lib.tsfa_emul_pack_valid_const.argtypes, lib.tsfa_emul_pack_valid_const.restype = [ctypes.c_int], ctypes.c_int
    lib.tsfa_emul_pack_valid.argtypes = (
        [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_int64] * 6 + [ctypes.c_void_p, ctypes.c_int32]
        + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
        + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
           ctypes.c_void_p, ctypes.c_int64])
    lib.tsfa_emul_pack_valid.restype = ctypes.c_int
    _lib = lib
    return lib


def row_chunk():
    """Steps of one work item."""
    return int(load().tsfa_emul_pack_valid_const(0))


def scratch_bytes(n_batch, n_time):
    """What the call needs of scratch: 200 bytes per work item."""
    return int(load().tsfa_emul_pack_valid_const(2)) * n_batch * (-(-n_time // row_chunk()))


def raw(x_ptr, x_type, shape, strides, lengths_ptr, lengths_type, t_ptr, t_type, t_strides, values_ptr, cso, offsets_ptr, steps_ptr,
        stamps_ptr, scratch_ptr, scratch_nbytes, flags_ptr, grid=3):
    """The emulated call on raw addresses (ints, 0 for NULL) -> its status."""
    (B, C, n), (sb, sc, st), (tsb, tst) = shape, strides, t_strides
    return int(load().tsfa_emul_pack_valid(x_ptr or None, x_type, B, C, n, sb, sc, st, lengths_ptr or None, lengths_type,
                                           t_ptr or None, t_type, tsb, tst, values_ptr or None, cso, offsets_ptr or None,
                                           steps_ptr or None, stamps_ptr or None, scratch_ptr or None, scratch_nbytes,
                                           flags_ptr or None, grid))


class EmulValid:
    """One emulated tsfa_pack_dense_valid call on the strided numpy view `x` of logical shape (B, C, n) (any strides numpy
    can express without a negative one, stride 0 included; bfloat16 travels as uint16 bit patterns with bf16=True), with
    optional `lengths` and optional stamps `t`: a strided (B, n) view of int64 ticks (`unit`), datetime64 or float64 seconds.
    `values`: [C, T] in the output dtype, `offsets`: int64[B + 1], `steps`: int32[T], `stamps`: the right-padded (B, n)
    stamps of the kept steps (cells beyond a kept count hold STAMP_SENTINEL's bits), `hours`: float64[T] by the emulated
    tsfa_pack_times on (stamps, offsets) -- its flag bit lands in `flags` as well --, `flags`, `status`; `guards_intact`:
    the sentinel cells around every output, between T and the channel stride, and around the flag word are untouched."""

    def __init__(self, x, lengths=None, t=None, unit="ns", bf16=False, grid=3, flags=0):
        assert x.ndim == 3
        B, C, n = x.shape
        isz = x.dtype.itemsize
        assert all(s % isz == 0 and s >= 0 for s in x.strides)
        x_type = epd.x_type_of(x, bf16)
        out_dtype = np.dtype(np.float64 if x_type == _native.TSFA_F64 else np.float32)
        cso = B * n
        out = np.full((C * cso + 2 * GUARD) * out_dtype.itemsize, OUT_SENTINEL, dtype=np.uint8).view(out_dtype)
        offs = np.full(B + 1 + 2 * GUARD, OFFSET_SENTINEL, dtype=np.int64)
        steps = np.full(cso + 2 * GUARD, STEP_SENTINEL, dtype=np.int32)
        word = np.array([0, flags, 0], dtype=np.int32)
        scratch = np.zeros(scratch_bytes(B, n) // 8, dtype=np.uint64)
        lptr, ltype = 0, 0
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths)
            ltype = {np.dtype(np.int32): _native.TSFA_I32, np.dtype(np.int64): _native.TSFA_I64}[lengths.dtype]
            lptr = lengths.ctypes.data
        tptr, t_type, t_strides, stamps, sptr = 0, 0, (0, 0), None, 0
        if t is not None:
            assert t.shape == (B, n)
            if t.dtype.kind == "M":
                unit = np.datetime_data(t.dtype)[0]
                t = t.view(np.int64)
            assert all(s % 8 == 0 and s >= 0 for s in t.strides)
            t_type = {np.dtype(np.int64): _native.TSFA_I64, np.dtype(np.float64): _native.TSFA_F64}[t.dtype]
            t_strides = tuple(s // 8 for s in t.strides)
            stamps = np.full(B * n + 2 * GUARD, STAMP_SENTINEL, dtype=np.int64)
            tptr, sptr = t.ctypes.data, stamps[GUARD:].ctypes.data
        self.status = raw(x.ctypes.data, x_type, (B, C, n), tuple(s // isz for s in x.strides), lptr, ltype, tptr, t_type, t_strides,
                          out[GUARD:].ctypes.data, cso, offs[GUARD:].ctypes.data, steps[GUARD:].ctypes.data, sptr,
                          scratch.ctypes.data, scratch.nbytes, word[1:].ctypes.data, grid)
        self.flags = int(word[1])
        self.out_dtype = out_dtype
        if self.status != _native.TSFA_OK:
            return
        self.offsets = offs[GUARD:GUARD + B + 1].copy()
        T = int(self.offsets[-1])
        body = out[GUARD:GUARD + C * cso].reshape(C, cso)
        self.values = body[:, :T].copy()
        self.steps = steps[GUARD:GUARD + T].copy()
        as_bits = np.dtype("u%d" % out_dtype.itemsize)
        sent = np.full(out_dtype.itemsize, OUT_SENTINEL, dtype=np.uint8).view(as_bits)[0]
        ok = ((out[:GUARD].view(as_bits) == sent).all() and (out[GUARD + C * cso:].view(as_bits) == sent).all()
              and (body[:, T:].view(as_bits) == sent).all()
              and (offs[:GUARD] == OFFSET_SENTINEL).all() and (offs[GUARD + B + 1:] == OFFSET_SENTINEL).all()
              and (steps[:GUARD] == STEP_SENTINEL).all() and (steps[GUARD + T:] == STEP_SENTINEL).all()
              and word[0] == 0 and word[2] == 0)
        self.stamps = self.hours = None
        if stamps is not None:
            kept = np.diff(self.offsets)
            self.stamps = stamps[GUARD:GUARD + B * n].reshape(B, n).copy()
            beyond = np.arange(n)[None, :] >= kept[:, None]
            ok = ok and (stamps[:GUARD] == STAMP_SENTINEL).all() and (stamps[GUARD + B * n:] == STAMP_SENTINEL).all() \
                and (self.stamps[beyond] == STAMP_SENTINEL).all()
            view = self.stamps if t_type == _native.TSFA_I64 else self.stamps.view(np.float64)
            hours = ept.EmulTimes(view, self.offsets, unit=unit, grid=grid, flags=self.flags)
            assert hours.status == 0
            ok = ok and hours.guards_intact
            self.hours, self.flags = hours.hours, hours.flags
        self.guards_intact = bool(ok)

    @property
    def bad_length(self):
        return bool(self.flags & _native.TSFA_DENSE_BAD_LENGTH)

    @property
    def empty_series(self):
        return bool(self.flags & _native.TSFA_DENSE_EMPTY_SERIES)
