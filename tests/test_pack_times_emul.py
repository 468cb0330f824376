"""The times packer's kernel body (tsfresh_amd/csrc/pack_times.h), g++ build, one thread per workgroup, against the pandas
arithmetic it replaces (`data._hours_since_first` on a DatetimeIndex): bit equality in every unit, on spans whose int64 ->
float64 conversion rounds, on stamps that do not ascend, through every stride form; NaT / NaN, the cells beyond a length,
the guards around the output and every status code.  No GPU needed; what only the device can show (its own division and
conversion sequences) is in test_tensor_times_gpu.py."""
import numpy as np
import pandas as pd
import pytest

import emul_pack_dense_lib as epd
import emul_pack_times_lib as ept
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction.data import _hours_since_first

B = 5
CHUNK = ept.row_chunk()
NAT = np.iinfo(np.int64).min
UNITS = ("ns", "us", "ms", "s")


def _lengths(n):
    """Ragged lengths of B series of at most n samples that include 1, 2 (where n allows) and n."""
    return np.array([min(n, v) for v in (1, 2, n, max(1, n // 2 + 1), max(1, n - 1))], dtype=np.int64)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _ticks(n, unit, seed, b=B):
    """(b, n) ascending int64 stamps around 2020 in `unit`, irregular steps of up to ~3 hours."""
    rng = np.random.default_rng(seed)
    tps = ept.TICKS_PER_SECOND[unit]
    steps = rng.integers(1, 10_000 * tps + 1, size=(b, n))
    return 1_600_000_000 * tps + rng.integers(0, 86_400 * tps, size=(b, 1)) + np.cumsum(steps, axis=1)


def _pandas_hours(t, lengths, unit):
    """`_hours_since_first` on the DatetimeIndex of the ragged batch: the expression the kernel must equal bit for bit."""
    flat = np.concatenate([t[b, :lengths[b]] for b in range(t.shape[0])])
    index = pd.DatetimeIndex(flat.view("datetime64[%s]" % unit))
    assert index.unit == unit
    return _hours_since_first(index, slice(None), _offsets(lengths))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_offsets_of_the_dense_packer_are_the_layout():
    """The offsets the times packer consumes are the ones the dense packer writes for the same lengths."""
    lengths = _lengths(7)
    dense = epd.EmulDense(np.zeros((B, 1, 7), dtype=np.float32), lengths=lengths)
    assert dense.status == 0 and np.array_equal(dense.offsets, _offsets(lengths))
    t = _ticks(7, "ns", 1)
    res = ept.EmulTimes(t, dense.offsets)
    assert res.status == 0 and res.guards_intact and not res.bad_time
    assert _same(res.hours, _pandas_hours(t, lengths, "ns"))


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("n", (1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5))
def test_bit_equal_to_pandas(unit, n):
    t = _ticks(n, unit, seed=n)
    for lengths in (np.full(B, n, dtype=np.int64), _lengths(n)):
        for grid in (1, 3, 10 ** 6):
            res = ept.EmulTimes(t, _offsets(lengths), unit=unit, grid=grid)
            assert res.status == 0 and res.guards_intact and res.flags == 0
            assert _same(res.hours, _pandas_hours(t, lengths, unit))
    # datetime64 of the unit is the same array
    res = ept.EmulTimes(t.view("datetime64[%s]" % unit), _offsets(_lengths(n)), unit="ns")
    assert _same(res.hours, _pandas_hours(t, _lengths(n), unit))


def test_spans_beyond_2_pow_53_round_in_the_conversion():
    rng = np.random.default_rng(3)
    n = 40
    year = 365 * 86_400 * 10 ** 9
    t = (np.arange(n)[None, :] * year + rng.integers(0, 10 ** 9, size=(B, n)) + 10 ** 18 // 2).astype(np.int64)
    t[:, 0] = rng.integers(0, 10 ** 9, size=B)
    diff = t - t[:, :1]
    assert (np.abs(diff[:, 1:]) > 2 ** 53).all() and (diff.astype(np.float64).astype(np.int64) != diff).any()   # inexact
    lengths = _lengths(n)
    res = ept.EmulTimes(t, _offsets(lengths))
    assert res.status == 0 and res.guards_intact and res.flags == 0
    assert _same(res.hours, _pandas_hours(t, lengths, "ns"))
    # a reciprocal multiply, or one division by the product, does not give these bits
    want = _pandas_hours(t, np.full(B, n), "ns")
    assert not _same(diff.reshape(-1) * 1e-9 / 3600.0, want) or not _same(diff.reshape(-1) / 3.6e12, want)


def test_stamps_that_do_not_ascend_give_negative_hours():
    rng = np.random.default_rng(4)
    t = rng.permuted(_ticks(33, "us", 5), axis=1)
    lengths = _lengths(33)
    res = ept.EmulTimes(t, _offsets(lengths), unit="us")
    assert res.status == 0 and res.guards_intact and (res.hours < 0).any()
    assert _same(res.hours, _pandas_hours(t, lengths, "us"))


@pytest.mark.parametrize("n", (1, 2, 9, CHUNK + 3))
def test_strides(n):
    lengths = _lengths(n)
    t = _ticks(n, "ns", seed=7 + n)
    want = _pandas_hours(t, lengths, "ns")
    views = {
        "contiguous": t,
        "transposed": np.ascontiguousarray(t.T).T,                       # stride_time = B
        "step2": np.repeat(t, 2, axis=1)[:, ::2],                         # a step-2 slice
        "offset": np.concatenate([t[:, :1] - 1, t], axis=1)[:, 1:],       # (an odd first element: the pair path's alignment test)
    }
    for name, v in views.items():
        assert np.array_equal(v, t)
        res = ept.EmulTimes(v, _offsets(lengths))
        assert res.status == 0 and res.guards_intact, name
        assert _same(res.hours, want), name
    if n > 1:
        assert views["transposed"].strides == (8, 8 * B) and views["step2"].strides[1] == 16
    # one clock for the batch: stride_batch 0
    shared = np.broadcast_to(t[2], (B, n))
    assert shared.strides[0] == 0
    res = ept.EmulTimes(shared, _offsets(lengths))
    assert res.status == 0 and res.guards_intact
    assert _same(res.hours, _pandas_hours(np.ascontiguousarray(shared), lengths, "ns"))


@pytest.mark.parametrize("n", (1, 2, 11, CHUNK + 1))
def test_float_seconds(n):
    rng = np.random.default_rng(n)
    t = 1.6e9 + np.cumsum(rng.uniform(0.001, 5000.0, size=(B, n)), axis=1)
    lengths = _lengths(n)
    want = np.concatenate([(t[b, :lengths[b]] - t[b, 0]) / 3600.0 for b in range(B)])
    for v in (t, np.ascontiguousarray(t.T).T, np.repeat(t, 2, axis=1)[:, ::2]):
        res = ept.EmulTimes(v, _offsets(lengths), unit="s")   # (the unit is ignored for seconds)
        assert res.status == 0 and res.guards_intact and res.flags == 0
        assert _same(res.hours, want)
    # ... also with a ticks_per_second that ticks would refuse
    out = np.zeros(int(lengths.sum()))
    flags = np.zeros(1, dtype=np.int32)
    off = _offsets(lengths)
    assert ept.raw(t.ctypes.data, _native.TSFA_F64, 12345, B, n, n, 1, off.ctypes.data, out.ctypes.data, flags.ctypes.data) == 0
    assert _same(out, want)


@pytest.mark.parametrize("kind", ("ticks", "seconds"))
def test_missing_stamps(kind):
    n = 9
    lengths = np.array([9, 4, 9, 1, 6], dtype=np.int64)
    off = _offsets(lengths)
    ticks = _ticks(n, "ns", 11)
    base = ticks if kind == "ticks" else ticks.astype(np.float64) / 1e9
    missing = NAT if kind == "ticks" else np.nan

    def want_of(t):
        if kind == "ticks":
            return _pandas_hours(t, lengths, "ns")
        return np.concatenate([(t[b, :lengths[b]] - t[b, 0]) / 3600.0 for b in range(B)])

    # one inside a length: the bit, NaN hours for that sample only
    t = base.copy()
    t[2, 5] = missing
    res = ept.EmulTimes(t, off)
    assert res.status == 0 and res.guards_intact and res.flags == _native.TSFA_DENSE_BAD_TIME
    assert np.flatnonzero(np.isnan(res.hours)).tolist() == [int(off[2]) + 5]
    assert np.array_equal(res.hours, want_of(t), equal_nan=True)
    # the bit is ORed into what the word held
    assert ept.EmulTimes(t, off, flags=_native.TSFA_PACK_VALUE_NAN).flags == _native.TSFA_PACK_VALUE_NAN | _native.TSFA_DENSE_BAD_TIME
    # beyond a length: never read
    t = base.copy()
    t[1, 4:] = missing
    t[3, 1:] = missing
    res = ept.EmulTimes(t, off)
    assert res.status == 0 and res.guards_intact and res.flags == 0 and not np.isnan(res.hours).any()
    assert _same(res.hours, want_of(base))
    # a missing first stamp: the whole series
    t = base.copy()
    t[4, 0] = missing
    res = ept.EmulTimes(t, off)
    assert res.status == 0 and res.guards_intact and res.bad_time
    assert np.flatnonzero(np.isnan(res.hours)).tolist() == list(range(int(off[4]), int(off[5])))
    assert np.array_equal(res.hours, want_of(t), equal_nan=True)


def test_a_length_of_zero_reads_and_writes_nothing():
    """Offsets of a batch whose bad lengths the dense packer clamped to 0: such a series has no cell, and its first stamp --
    which lies at its length -- is not read."""
    t = _ticks(5, "ns", 2)
    t[1, :] = NAT
    off = np.array([0, 5, 5, 10, 15, 20], dtype=np.int64)
    res = ept.EmulTimes(t, off)
    assert res.status == 0 and res.guards_intact and res.flags == 0
    assert _same(res.hours, _pandas_hours(t[[0, 2, 3, 4]], np.full(4, 5), "ns"))
    # a difference of offsets beyond n_time is clamped: nothing outside t is read (the cells it leaves are not written)
    off = np.array([0, 9, 10, 15, 20, 25], dtype=np.int64)
    res = ept.EmulTimes(_ticks(5, "ns", 2), off)
    assert res.status == 0 and res.guards_intact
    assert (res.hours[5:9] == ept.SENTINEL).all() and _same(res.hours[:5], _pandas_hours(_ticks(5, "ns", 2)[:1], np.array([5]), "ns"))


def test_status_codes():
    t = _ticks(4, "ns", 1)
    off = _offsets(np.full(B, 4))
    out = np.zeros(B * 4)
    flags = np.zeros(1, dtype=np.int32)
    p = dict(t=t.ctypes.data, ty=_native.TSFA_I64, tps=10 ** 9, B=B, n=4, sb=4, st=1, off=off.ctypes.data, out=out.ctypes.data,
             fl=flags.ctypes.data)

    def call(**kw):
        a = dict(p, **kw)
        return ept.raw(a["t"], a["ty"], a["tps"], a["B"], a["n"], a["sb"], a["st"], a["off"], a["out"], a["fl"])

    assert call() == _native.TSFA_OK
    for name in ("t", "off", "out", "fl"):
        assert call(**{name: 0}) == _native.TSFA_ERR_INVALID, name
    for ty in (_native.TSFA_F32, _native.TSFA_I32, _native.TSFA_U64, _native.TSFA_F16, 99):
        assert call(ty=ty) == _native.TSFA_ERR_INVALID
    for tps in (0, -1, 2, 60, 10 ** 12):
        assert call(tps=tps) == _native.TSFA_ERR_INVALID
    for tps in (1, 10 ** 3, 10 ** 6, 10 ** 9):
        assert call(tps=tps) == _native.TSFA_OK
    assert call(sb=-1) == _native.TSFA_ERR_INVALID and call(st=-1) == _native.TSFA_ERR_INVALID
    assert call(B=0) == _native.TSFA_ERR_INVALID and call(n=0) == _native.TSFA_ERR_INVALID and call(B=-3) == _native.TSFA_ERR_INVALID
    assert call(n=33_554_432) == _native.TSFA_ERR_TOO_LONG
    assert call(B=2 ** 40, n=2 ** 24) == _native.TSFA_ERR_INVALID       # more than 2^62 stamps
    assert call(sb=2 ** 60) == _native.TSFA_ERR_INVALID                  # a stride that reaches beyond 2^60 elements
    assert (out == _pandas_hours(t, np.full(B, 4), "ns")).all()           # (the refused calls wrote nothing)


def test_the_flag_bit_is_a_new_one():
    bits = (_native.TSFA_PACK_UNSORTED, _native.TSFA_PACK_VALUE_NAN, _native.TSFA_PACK_IN_ORDER, _native.TSFA_DENSE_BAD_LENGTH,
            _native.TSFA_DENSE_BAD_TIME)
    assert bits == (1, 2, 4, 8, 16)
