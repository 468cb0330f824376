"""The valid-step packer's kernel bodies (tsfresh_amd/csrc/pack_valid.h), g++ build with the 64 lanes of a wavefront looped,
against a numpy statement of `dropna()` on the wide frame of the batch (pack_valid_cases.dropna_reference): values, offsets,
original step indices and kept stamps exactly, the hours bit for bit against `data._hours_since_first` on the DatetimeIndex of
the kept rows; every validity pattern at every series length, layout and element type, the scan's carry, more work items than
workgroups, the two flags with the clamping, the guards around every output and the status codes.  No GPU needed; what only
the device can show (the hardware ballot, the rounds split over four wavefronts, the barriers, the 1024-thread scan) is in
test_pack_valid_gpu.py, which runs the same grid against this emulation."""
import numpy as np
import pandas as pd
import pytest

import emul_pack_valid_lib as epv
import pack_valid_cases as pvc
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction.data import _hours_since_first

NAT = pvc.NAT


def _run(case, unit="ns", grid=3):
    return epv.EmulValid(case.x_view(), lengths=case.lengths, t=case.t_view(), unit=unit, bf16=case.dtype == "bfloat16", grid=grid)


def _pandas_hours(kept_stamps, offsets, unit):
    index = pd.DatetimeIndex(kept_stamps.view("datetime64[%s]" % unit))
    assert index.unit == unit
    return _hours_since_first(index, slice(None), offsets)


def _check(case, unit="ns", grid=3):
    res = _run(case, unit, grid)
    values, offsets, steps, stamps = pvc.dropna_reference(case)
    assert res.status == 0 and res.guards_intact, case.name
    assert res.flags == 0, case.name
    assert np.array_equal(res.offsets, offsets), case.name
    assert pvc.same_bits(res.values, values), case.name
    assert res.steps.dtype == np.int32 and np.array_equal(res.steps, steps), case.name
    if stamps is not None:
        kept = np.diff(offsets)
        got = np.concatenate([res.stamps[b, :kept[b]] for b in range(len(kept))])
        assert np.array_equal(got, stamps), case.name
        assert pvc.same_bits(res.hours, _pandas_hours(stamps, offsets, unit)), case.name
    return res


def test_the_grid_constants_are_the_kernels():
    assert epv.row_chunk() == pvc.CHUNK
    assert epv.scratch_bytes(3, 1025) == _native.pack_dense_valid_scratch_bytes(3, 1025) == 200 * 3 * 2


@pytest.mark.parametrize("layout", pvc.LAYOUTS)
@pytest.mark.parametrize("dtype", pvc.DTYPES)
def test_every_pattern_at_every_length(dtype, layout):
    for n in pvc.N_GRID:
        _check(pvc.make_case(dtype, layout, n, with_stamps=False))
        res = _check(pvc.make_case(dtype, layout, n, with_stamps=True))
        if n >= 63 and layout != "expanded":
            kept = np.diff(res.offsets)
            # the patterns did what their names say
            assert kept[0] == n and kept[1] == (n + 1) // 2 and kept[2] == 1 and kept[3] == 1
            assert kept[4] == n - max(0, min(n, pvc.CHUNK + 34) - (pvc.CHUNK - 30)) and 1 <= kept[5] < n
            assert kept[6] == n - n // 3 and 1 <= kept[7] < n
            assert res.steps[res.offsets[3]] == n - 1 and res.steps[res.offsets[2]] == 0


@pytest.mark.parametrize("unit", pvc.UNITS)
def test_hours_equal_pandas_in_every_unit(unit):
    for n in (65, 1025):
        for layout in ("bcn", "stepped", "expanded"):
            _check(pvc.make_case("float32", layout, n, with_stamps=True, unit=unit), unit=unit)


def test_float_seconds_and_a_nan_second():
    case = pvc.make_case("float64", "bcn", 65, with_stamps=True, unit="s")
    ticks = case.stamps()
    seconds = np.where(ticks == NAT, np.nan, ticks.astype(np.float64))
    res = epv.EmulValid(case.x_view(), lengths=case.lengths, t=seconds)
    values, offsets, steps, stamps = pvc.dropna_reference(case)
    assert res.status == 0 and res.guards_intact and res.flags == 0
    assert np.array_equal(res.offsets, offsets) and np.array_equal(res.steps, steps) and pvc.same_bits(res.values, values)
    first = np.repeat(stamps[offsets[:-1]], np.diff(offsets))
    assert pvc.same_bits(res.hours, (stamps.astype(np.float64) - first.astype(np.float64)) / 3600.0)


def test_the_grid_size_does_not_matter():
    case = pvc.make_case("float32", "cl3", 2049, with_stamps=True)
    want = _run(case, grid=1)
    for grid in (2, 5, 10 ** 6):
        res = _run(case, grid=grid)
        assert res.guards_intact and np.array_equal(res.offsets, want.offsets) and np.array_equal(res.steps, want.steps)
        assert pvc.same_bits(res.values, want.values) and pvc.same_bits(res.hours, want.hours)


@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_many_series_carry_the_scan_and_stride_the_grid(dtype):
    case = pvc.many_series_case(dtype)
    assert case.shape[0] > 65536
    _check(case)


def test_lengths_of_either_width_and_none():
    case = pvc.make_case("float32", "bcn", 65, with_stamps=False)
    want = pvc.dropna_reference(case)
    res = epv.EmulValid(case.x_view(), lengths=case.lengths.astype(np.int32))
    assert res.flags == 0 and res.guards_intact and np.array_equal(res.offsets, want[1]) and pvc.same_bits(res.values, want[0])
    # without lengths the padding of series 6 is read: it is NaN, so the same steps stay
    res = epv.EmulValid(case.x_view())
    assert res.flags == 0 and res.guards_intact and np.array_equal(res.offsets, want[1]) and pvc.same_bits(res.values, want[0])


def test_infinities_are_values():
    x = np.array([[[1.0, np.inf, -np.inf, np.nan, 5.0]]], dtype=np.float32)
    res = epv.EmulValid(x)
    assert res.flags == 0 and res.steps.tolist() == [0, 1, 2, 4]
    assert pvc.same_bits(res.values, np.array([[1.0, np.inf, -np.inf, 5.0]], dtype=np.float32))


def test_every_half_nan_is_dropped_and_nothing_else():
    bits = np.arange(65536, dtype=np.uint16)
    for dtype in ("float16", "bfloat16"):
        x = bits.reshape(1, 1, -1) if dtype == "bfloat16" else bits.view(np.float16).reshape(1, 1, -1)
        res = epv.EmulValid(x, bf16=dtype == "bfloat16")
        as_float = pvc.from_bits(bits, dtype)
        keep = ~np.isnan(as_float)
        assert res.flags == 0 and res.guards_intact and np.array_equal(res.steps, np.flatnonzero(keep).astype(np.int32))
        assert pvc.same_bits(res.values[0], as_float[keep])


def test_an_empty_series_raises_its_flag():
    case = pvc.make_case("float64", "bcn", 65, with_stamps=True)
    x = case.x_view().copy()
    x[3, 1, :] = np.nan                                  # every step of series 3
    res = epv.EmulValid(x, lengths=case.lengths, t=case.t_view())
    assert res.status == 0 and res.guards_intact and res.flags == _native.TSFA_DENSE_EMPTY_SERIES and res.empty_series
    assert res.offsets[3] == res.offsets[4] and np.flatnonzero(np.diff(res.offsets) == 0).tolist() == [3]
    # by the stamps alone, in the last series (its successor is offsets[B])
    t = case.stamps().copy()
    t[7, :] = NAT
    res = epv.EmulValid(case.x_view(), lengths=case.lengths, t=t)
    assert res.flags == _native.TSFA_DENSE_EMPTY_SERIES and np.flatnonzero(np.diff(res.offsets) == 0).tolist() == [7]
    # the bit is ORed into what the word held
    assert epv.EmulValid(x, flags=_native.TSFA_PACK_IN_ORDER).flags == _native.TSFA_PACK_IN_ORDER | _native.TSFA_DENSE_EMPTY_SERIES


@pytest.mark.parametrize("layout", ("bcn", "cl3", "stepped"))
def test_bad_lengths_are_clamped_and_flagged(layout):
    """The views are exactly as large as the batch (numpy owns nothing beyond), the cells between the stepped view's samples
    are NaN: a length beyond n that was not clamped would read them or run off the end."""
    for n in (5, 1025):
        case = pvc.make_case("float32", layout, n, with_stamps=True)
        good = case.lengths.copy()
        for bad in (0, -3, n + 1, 2 ** 40):
            for pos in (0, 4, 7):
                case.lengths = good.copy()
                case.lengths[pos] = bad
                values, offsets, steps, stamps = pvc.dropna_reference(case)   # (it clamps the lengths into [0, n])
                res = _run(case)
                assert res.status == 0 and res.guards_intact
                assert res.flags == _native.TSFA_DENSE_BAD_LENGTH | (_native.TSFA_DENSE_EMPTY_SERIES if bad <= 0 else 0)
                assert np.array_equal(res.offsets, offsets) and np.array_equal(res.steps, steps) and pvc.same_bits(res.values, values)


def test_status_codes():
    x = np.zeros((2, 3, 4), dtype=np.float32)
    t = np.zeros((2, 4), dtype=np.int64)
    out = np.zeros(3 * 8, dtype=np.float32)
    offs = np.zeros(3, dtype=np.int64)
    steps = np.zeros(8, dtype=np.int32)
    stamps = np.zeros(8, dtype=np.int64)
    scratch = np.zeros(2 * 25 + 1, dtype=np.uint64)
    flags = np.zeros(1, dtype=np.int32)
    p = dict(x=x.ctypes.data, ty=_native.TSFA_F32, shape=(2, 3, 4), strides=(12, 4, 1), l=0, lt=0, t=t.ctypes.data, tt=_native.TSFA_I64,
             ts=(4, 1), out=out.ctypes.data, cso=8, off=offs.ctypes.data, steps=steps.ctypes.data, stamps=stamps.ctypes.data,
             scr=scratch.ctypes.data, nscr=2 * 200, fl=flags.ctypes.data)

    def call(**kw):
        a = dict(p, **kw)
        return epv.raw(a["x"], a["ty"], a["shape"], a["strides"], a["l"], a["lt"], a["t"], a["tt"], a["ts"], a["out"], a["cso"], a["off"],
                       a["steps"], a["stamps"], a["scr"], a["nscr"], a["fl"])

    assert call() == _native.TSFA_OK and steps.tolist() == [0, 1, 2, 3] * 2 and offs.tolist() == [0, 4, 8]
    assert call(t=0, stamps=0) == _native.TSFA_OK
    for name in ("x", "out", "off", "steps", "scr", "fl"):
        assert call(**{name: 0}) == _native.TSFA_ERR_INVALID, name
    assert call(stamps=0) == _native.TSFA_ERR_INVALID                    # stamps in, nowhere to put them
    for ty in (_native.TSFA_I32, _native.TSFA_I64, 99):
        assert call(ty=ty) == _native.TSFA_ERR_INVALID
    for tt in (_native.TSFA_F32, _native.TSFA_I32, 99):
        assert call(tt=tt) == _native.TSFA_ERR_INVALID
    assert call(tt=_native.TSFA_F64) == _native.TSFA_OK
    assert call(strides=(12, -4, 1)) == _native.TSFA_ERR_INVALID and call(ts=(-4, 1)) == _native.TSFA_ERR_INVALID
    assert call(ts=(4, 2 ** 60)) == _native.TSFA_ERR_INVALID
    assert call(shape=(2, 0, 4)) == _native.TSFA_ERR_INVALID and call(cso=7) == _native.TSFA_ERR_INVALID
    assert call(nscr=2 * 200 - 1) == _native.TSFA_ERR_INVALID and call(scr=scratch.ctypes.data + 4) == _native.TSFA_ERR_INVALID
    assert call(l=x.ctypes.data, lt=_native.TSFA_F32) == _native.TSFA_ERR_INVALID
    assert call(shape=(1, 1, 33_554_432), strides=(0, 0, 0), cso=33_554_432, nscr=2 ** 40) == _native.TSFA_ERR_TOO_LONG


def test_the_flag_bit_is_a_new_one():
    bits = (_native.TSFA_PACK_UNSORTED, _native.TSFA_PACK_VALUE_NAN, _native.TSFA_PACK_IN_ORDER, _native.TSFA_DENSE_BAD_LENGTH,
            _native.TSFA_DENSE_BAD_TIME, _native.TSFA_DENSE_EMPTY_SERIES)
    assert bits == (1, 2, 4, 8, 16, 32)
