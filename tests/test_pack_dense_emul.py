"""The dense packer's kernel bodies (tsfresh_amd/csrc/pack_dense.h), g++ build, one thread per workgroup, against numpy indexing:
the two half-precision conversions over every bit pattern, the three routes over the smallest shapes that straddle the tile
edges, every layout / element type / form of `lengths`, and the clamping of bad lengths with guard cells around the buffers.
No GPU needed."""
import numpy as np
import pytest

import emul_pack_dense_lib as epd
from tsfresh_amd import _native

TC = epd.tile_c()
TT = epd.tile_t(TC)   # (of a full channel tile; fewer channels: epd.tile_t(C), longer)
B_GRID = (1, 3)
C_GRID = (1, 2, 5, TC - 1, TC, TC + 1)
DTYPES = ("float64", "float32", "float16", "bfloat16")
LAYOUTS = ("bcn", "bnc", "slice", "expand")


def _bf16_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _as_out(x, dtype):
    """What the packer must produce for the strided view x (bfloat16: uint16 bit patterns)."""
    if dtype == "bfloat16":
        return _bf16_to_f32(np.ascontiguousarray(x))
    return np.ascontiguousarray(x).astype(np.float32) if dtype == "float16" else np.ascontiguousarray(x)


def _storage(rng, shape, dtype, fill_nan):
    """A C-contiguous array of `shape`: finite random samples, or NaN everywhere (the gaps and borders of a sliced view:
    a kernel that loaded one of them would raise TSFA_PACK_VALUE_NAN)."""
    if dtype == "bfloat16":
        if fill_nan:
            return np.full(shape, 0x7fc1, dtype=np.uint16)
        return (rng.integers(0, 0x7f80, size=shape) | (rng.integers(0, 2, size=shape) << 15)).astype(np.uint16)
    if fill_nan:
        return np.full(shape, np.nan, dtype=dtype)
    return (rng.standard_normal(shape) * 37.0).astype(dtype)


def _view(rng, layout, B, C, n, dtype):
    """A (B, C, n) view in the named layout."""
    if layout == "bcn":
        return _storage(rng, (B, C, n), dtype, False)
    if layout == "bnc":
        return _storage(rng, (B, n, C), dtype, False).transpose(0, 2, 1)
    if layout == "expand":
        return np.broadcast_to(_storage(rng, (1, C, n), dtype, False), (B, C, n))
    big = _storage(rng, (2 * B + 1, C + 2, 3 * n + 2), dtype, True)
    view = big[1::2, 1:C + 1, 2:2 + 3 * n:3]
    assert view.shape == (B, C, n)
    view[...] = _storage(rng, (B, C, n), dtype, False)
    return view


def _expected(x, dtype, lens):
    return np.concatenate([_as_out(x[b, :, :lens[b]], dtype) for b in range(x.shape[0])], axis=1)


def _same_bits(a, b):
    u = np.dtype("u%d" % a.dtype.itemsize)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def _route_of(x, layout):
    """The issue's rule on the view's element strides (numpy is free in the stride it gives an axis of one entry); for
    shapes with more than one channel and time step the layout alone names the route."""
    _, sc, st = (s // x.dtype.itemsize for s in x.strides)
    C, n = x.shape[1:]
    route = epd.ROUTE_ROWS_UNIT if st == 1 else (epd.ROUTE_TRANSPOSE if sc == 1 and C > 1 else epd.ROUTE_ROWS)
    if C > 1 and n > 1:
        assert route == {"bcn": epd.ROUTE_ROWS_UNIT, "expand": epd.ROUTE_ROWS_UNIT, "bnc": epd.ROUTE_TRANSPOSE,
                         "slice": epd.ROUTE_ROWS}[layout]
    return route


def test_tiles_are_exported():
    assert TT >= 2 and TC >= 2 and TT % 32 == 0 and epd.row_chunk() >= TT and epd.vec() >= 1
    # a tile holds the same number of samples whatever the channel count; its time steps stay a multiple of the 32 banks
    for C in (1, 2, 3, 5, 8, 16, 17, TC, TC + 1, 1000):
        tc = min(TC, max(2, 1 << (C - 1).bit_length()))
        assert epd.tile_t(C) * tc == TT * TC and epd.tile_t(C) % 32 == 0


@pytest.mark.parametrize("kind", ("float16", "bfloat16"))
def test_every_half_bit_pattern(kind):
    lib = epd.load()
    bits = np.arange(65536, dtype=np.uint16)
    if kind == "float16":
        want, conv, x_all = bits.view(np.float16).astype(np.float32), lib.tsfa_emul_f16_to_f32_bits, bits.view(np.float16)
    else:
        want, conv, x_all = _bf16_to_f32(bits), lib.tsfa_emul_bf16_to_f32_bits, bits
    bf16 = kind == "bfloat16"
    nan = np.isnan(want)
    assert nan.sum() == (2046 if kind == "float16" else 254)
    # the conversion function itself, pattern by pattern
    got = np.array([conv(int(h)) for h in bits], dtype=np.uint32)
    assert np.array_equal(got[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got.view(np.float32)[nan]).all()
    # through the packer: all patterns in one row (rows route), and as one batch of one-sample series over 3 channels-last
    # channels (transpose route)
    res = epd.EmulDense(x_all.reshape(1, 1, -1), bf16=bf16)
    assert res.status == 0 and res.value_nan and res.guards_intact
    assert np.array_equal(res.values[0].view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(res.values[0][nan]).all()
    clean = np.ascontiguousarray(x_all[~nan])
    res = epd.EmulDense(clean.reshape(1, 1, -1), bf16=bf16)
    assert not res.value_nan and _same_bits(res.values[0], want[~nan])
    n = len(clean) // 240
    res = epd.EmulDense(clean[:240 * n].reshape(80, n, 3).transpose(0, 2, 1), bf16=bf16)
    assert res.route == epd.ROUTE_TRANSPOSE and not res.value_nan
    assert _same_bits(res.values, want[~nan][:240 * n].reshape(80, n, 3).transpose(2, 0, 1).reshape(3, -1))
    # every NaN pattern on its own raises the flag
    for h in bits[nan]:
        one = np.array([h], dtype=np.uint16)
        res = epd.EmulDense((one if bf16 else one.view(np.float16)).reshape(1, 1, 1), bf16=bf16)
        assert res.value_nan, hex(int(h))


def test_nan_flag_of_the_wide_types():
    for dtype in (np.float32, np.float64):
        x = np.ones((2, 3, 5), dtype=dtype)
        assert not epd.EmulDense(x).value_nan
        x[1, 2, 4] = np.nan
        assert epd.EmulDense(x).value_nan and epd.EmulDense(x.transpose(0, 2, 1).copy().transpose(0, 2, 1)).value_nan
        # a NaN beyond a series' length is never read
        assert not epd.EmulDense(x, lengths=np.array([5, 4], dtype=np.int32)).value_nan
        x[1, 2, 4] = -np.inf
        assert not epd.EmulDense(x).value_nan


def _length_forms(rng, B, n):
    ragged = rng.integers(1, n + 1, size=B)
    ragged[0] = 1
    ragged[-1] = n
    forms = [None]
    for dt in (np.int32, np.int64):
        forms += [np.full(B, n, dtype=dt), ragged.astype(dt)]
    return forms


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shape_grid(dtype, layout):
    rng = np.random.default_rng(11)
    for B in B_GRID:
        for C in C_GRID:
            for n in epd.n_grid(C):
                x = _view(rng, layout, B, C, n, dtype)
                for lengths in _length_forms(rng, B, n):
                    lens = np.full(B, n) if lengths is None else lengths
                    res = epd.EmulDense(x, lengths=lengths, bf16=dtype == "bfloat16")
                    where = (dtype, layout, B, C, n, None if lengths is None else (lengths.dtype.name, lengths.tolist()))
                    assert res.status == 0 and res.flags == 0, where
                    assert res.route == _route_of(x, layout), where
                    assert np.array_equal(res.offsets, np.concatenate([[0], np.cumsum(lens)])), where
                    assert _same_bits(res.values, _expected(x, dtype, lens)), where
                    assert res.guards_intact, where


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_longer_than_one_work_item_and_many_workgroups(dtype):
    rng = np.random.default_rng(5)
    n = 2 * epd.row_chunk() + 5
    for layout in ("bcn", "slice", "bnc"):
        x = _view(rng, layout, 2, 2, n, dtype)
        lengths = np.array([epd.row_chunk() + 1, n], dtype=np.int64)
        for grid in (1, 2, 1000):
            res = epd.EmulDense(x, lengths=lengths, bf16=dtype == "bfloat16", grid=grid)
            assert res.flags == 0 and res.guards_intact
            assert _same_bits(res.values, _expected(x, dtype, lengths))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_lengths_are_flagged_clamped_and_stay_inside_the_buffers(dtype, layout):
    rng = np.random.default_rng(2)
    for C, n in ((1, TT + 1), (5, TT - 1), (TC + 1, 2 * TT + 3)):
        x = _view(rng, layout, 3, C, n, dtype)
        for ltype in (np.int32, np.int64):
            for bad in (0, -1, n + 1, -2 ** 31, 2 ** 31 - 1):
                for pos in range(3):
                    lengths = np.array([n, 1, n // 2 + 1], dtype=ltype)
                    lengths[pos] = bad
                    res = epd.EmulDense(x, lengths=lengths, bf16=dtype == "bfloat16")
                    assert res.status == 0 and res.bad_length
                    # nothing outside x was loaded (the gaps of the sliced view hold NaN), nothing outside T written
                    assert not res.value_nan and res.guards_intact
                    lens = np.clip(lengths.astype(np.int64), 0, n)
                    assert np.array_equal(res.offsets, np.concatenate([[0], np.cumsum(lens)]))
                    assert _same_bits(res.values, _expected(x, dtype, lens))
    huge = np.array([2 ** 62, -2 ** 62, 3], dtype=np.int64)
    res = epd.EmulDense(_view(rng, layout, 3, 2, 7, dtype), lengths=huge, bf16=dtype == "bfloat16")
    assert res.bad_length and res.guards_intact and res.offsets.tolist() == [0, 7, 7, 10]


def test_arguments_tsfa_pack_dense_refuses():
    x = np.ones((2, 3, 4), dtype=np.float32)
    assert epd.EmulDense(x, channel_stride_out=7).status == _native.TSFA_ERR_INVALID
    assert epd.EmulDense(x, channel_stride_out=8).status == 0
    lib = epd.load()
    out, offs, flags = np.zeros(64, dtype=np.float64), np.zeros(8, dtype=np.int64), np.zeros(1, dtype=np.int32)

    def call(x_type=_native.TSFA_F32, shape=(2, 3, 4), strides=(12, 4, 1), ltype=0, lengths=None, cso=8):
        return lib.tsfa_emul_pack_dense(x.ctypes.data, x_type, *shape, *strides, lengths, ltype, out.ctypes.data, cso,
                                        offs.ctypes.data, flags.ctypes.data, 1, None)
    assert call() == 0
    for bad_type in (_native.TSFA_I32, _native.TSFA_I64, _native.TSFA_BOOL, 13, -1):
        assert call(x_type=bad_type) == _native.TSFA_ERR_INVALID
    for k in range(3):
        strides = [12, 4, 1]
        strides[k] = -1
        assert call(strides=tuple(strides)) == _native.TSFA_ERR_INVALID
        shape = [2, 3, 4]
        shape[k] = 0
        assert call(shape=tuple(shape)) == _native.TSFA_ERR_INVALID
    lens = np.array([4, 4], dtype=np.int16)
    assert call(lengths=lens.ctypes.data, ltype=_native.TSFA_I16) == _native.TSFA_ERR_INVALID
    # 33 554 432 samples per series: refused before anything is touched (the buffers here are far too small for it)
    assert call(shape=(1, 1, 33554432), strides=(0, 0, 0), cso=33554432) == _native.TSFA_ERR_TOO_LONG
