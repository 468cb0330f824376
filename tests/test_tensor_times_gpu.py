"""`times=` on the device.  The times packer alone: `tsfa_pack_times` equals the pandas / numpy expression bit for bit in every
unit, for float seconds, through unit and non-unit strides and for one shared clock -- which is what shows that the device's
int64 -> float64 conversion and its float64 division are the correctly rounded IEEE ones.  The three tensor entries with
`times=`: bit-equal to the frame entries on the wide frame that carries the same stamps as its DatetimeIndex (host packer),
the timewise columns also within the oracle's tolerances; a composite plan; the rolled windows; the selection; NaT.

B = 6, C = 2, n = 37, ragged lengths that include 1 and 2 (the packer alone also at a row of more than one work item)."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import conftest
from engines import oracle_engine
from parity import compare
from tsfresh_amd import (MinimalFCParameters, _native, extract_features, extract_features_tensor,
                         extract_relevant_features_tensor, extract_rolled_features, extract_rolled_features_tensor,
                         impute_tensor, select_features_tensor)
from tsfresh_amd.feature_extraction.data import _hours_since_first

pytestmark = pytest.mark.gpu

B, C, N = 6, 2, 37
KINDS = ["p", "q"]
LENGTHS = np.array([37, 1, 2, 20, 37, 11], dtype=np.int64)
TPS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
NAT = np.iinfo(np.int64).min
ATTRS = ("pvalue", "rvalue", "intercept", "slope", "stderr")
TIMEWISE = {"linear_trend_timewise": [{"attr": a} for a in ATTRS]}
MINIMAL_TIMED = dict(MinimalFCParameters(), **TIMEWISE)
ADF_TIMED = dict({"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"}, {"attr": "pvalue", "autolag": "BIC"}],
                  "maximum": None}, **TIMEWISE)
SETTINGS = {"minimal": MINIMAL_TIMED, "adf": ADF_TIMED}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _stamps(unit="ns", b=B, n=N):
    """(b, n) ascending int64 ticks of `unit`, irregular steps of up to ~2 hours."""
    rng = np.random.default_rng(31 + n)
    tps = TPS[unit]
    return 1_600_000_000 * tps + np.cumsum(rng.integers(1, 7_000 * tps + 1, size=(b, n)), axis=1)


@functools.lru_cache(maxsize=None)
def _samples():
    """(B, C, N) float32: a trend in the hours of each series plus noise."""
    rng = np.random.default_rng(17)
    hours = (_stamps() - _stamps()[:, :1]) / 3.6e12
    x = np.stack([(b + 1) * 0.5 * hours[b] + rng.standard_normal(N) for b in range(B)])
    return np.stack([x, -2.0 * x + rng.standard_normal((B, N))], axis=1).astype(np.float32)


def _pandas_hours(t, lengths, unit):
    flat = np.concatenate([t[b, :lengths[b]] for b in range(t.shape[0])])
    return _hours_since_first(pd.DatetimeIndex(flat.view("datetime64[%s]" % unit)), slice(None), _offsets(lengths))


def _frame(x, t, lengths, unit="ns"):
    cols = {"id": np.repeat(np.arange(B), lengths)}
    for c, kind in enumerate(KINDS):
        cols[kind] = np.concatenate([x[b, c, :lengths[b]] for b in range(B)])
    flat = np.concatenate([t[b, :lengths[b]] for b in range(B)])
    return pd.DataFrame(cols, index=pd.DatetimeIndex(flat.view("datetime64[%s]" % unit)))


@functools.lru_cache(maxsize=None)
def _frame_features(which, ragged):
    """The frame entry on the DatetimeIndex frame, host packer: computed once and left unchanged."""
    lengths = LENGTHS if ragged else np.full(B, N)
    return extract_features(_frame(_samples(), _stamps(), lengths), column_id="id", default_fc_parameters=SETTINGS[which],
                            pack="host", device=0)


def _device_hours(t, t_type, tps, lengths, n):
    """`_native.pack_times` on the offsets `_native.pack_dense` writes for `lengths` -> (hours[:T], flag word, cells beyond T)."""
    dev = "cuda:0"
    b = t.shape[0]
    x = torch.zeros((b, 1, n), dtype=torch.float32, device=dev)
    values = torch.empty((1, b * n), dtype=torch.float32, device=dev)
    offsets = torch.empty(b + 1, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ld = torch.from_numpy(lengths).to(dev)
    hours = torch.full((b * n + 8,), -7.25, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    _native.pack_dense(x.data_ptr(), _native.TSFA_F32, (b, 1, n), x.stride(), values.data_ptr(), b * n, offsets.data_ptr(),
                       flag.data_ptr(), device=0, lengths_ptr=ld.data_ptr(), lengths_type=_native.TSFA_I64)
    assert offsets.cpu().numpy().tolist() == _offsets(lengths).tolist() and int(flag.item()) == 0
    _native.pack_times(t.data_ptr(), t_type, tps, tuple(t.shape), t.stride(), offsets.data_ptr(), hours.data_ptr(), flag.data_ptr(),
                       device=0)
    T = int(lengths.sum())
    out = hours.cpu().numpy()
    return out[:T], int(flag.item()), out[T:]


@pytest.mark.parametrize("unit", ("ns", "us", "ms", "s"))
def test_packer_int64_ticks_equal_pandas_bit_for_bit(gpu, unit):
    t = _stamps(unit)
    want = _pandas_hours(t, LENGTHS, unit)
    views = {
        "contiguous": torch.from_numpy(t).cuda(),
        "transposed": torch.from_numpy(np.ascontiguousarray(t.T)).cuda().T,
        "step2": torch.from_numpy(np.repeat(t, 2, axis=1)).cuda()[:, ::2],
    }
    assert views["transposed"].stride() == (1, B) and views["step2"].stride() == (2 * N, 2)
    for name, v in views.items():
        got, flags, beyond = _device_hours(v, _native.TSFA_I64, TPS[unit], LENGTHS, N)
        assert flags == 0 and (beyond == -7.25).all(), name
        assert _same_bits(got, want), name
    shared = torch.from_numpy(t[3]).cuda().unsqueeze(0).expand(B, N)
    got, flags, beyond = _device_hours(shared, _native.TSFA_I64, TPS[unit], LENGTHS, N)
    assert flags == 0 and (beyond == -7.25).all()
    assert _same_bits(got, _pandas_hours(np.broadcast_to(t[3], (B, N)), LENGTHS, unit))


def test_packer_conversion_rounds_as_numpy_on_spans_beyond_2_pow_53(gpu):
    rng = np.random.default_rng(5)
    year = 365 * 86_400 * 10 ** 9
    t = (np.arange(N)[None, :] * year + rng.integers(0, 10 ** 9, size=(B, N)) + 10 ** 18 // 2).astype(np.int64)
    t[:, 0] = rng.integers(0, 10 ** 9, size=B)
    t[4] = rng.permutation(t[4])   # (stamps that do not ascend: negative hours)
    diff = t - t[:, :1]
    assert (diff.astype(np.float64).astype(np.int64) != diff).any()   # the conversion is inexact for some
    got, flags, _ = _device_hours(torch.from_numpy(t).cuda(), _native.TSFA_I64, 10 ** 9, LENGTHS, N)
    assert flags == 0 and (got < 0).any()
    assert _same_bits(got, _pandas_hours(t, LENGTHS, "ns"))


def test_packer_rows_of_more_than_one_work_item(gpu):
    n = 2 * 1024 + 5
    lengths = np.array([n, 1, 1025, 2], dtype=np.int64)
    t = _stamps("ns", b=4, n=n)
    want = _pandas_hours(t, lengths, "ns")
    for v in (torch.from_numpy(t).cuda(), torch.from_numpy(np.ascontiguousarray(t.T)).cuda().T):
        got, flags, beyond = _device_hours(v, _native.TSFA_I64, 10 ** 9, lengths, n)
        assert flags == 0 and (beyond == -7.25).all()
        assert _same_bits(got, want)


def test_packer_float_seconds_and_missing_stamps(gpu):
    rng = np.random.default_rng(9)
    t = 1.6e9 + np.cumsum(rng.uniform(0.001, 5000.0, size=(B, N)), axis=1)
    want = np.concatenate([(t[b, :LENGTHS[b]] - t[b, 0]) / 3600.0 for b in range(B)])
    for v in (torch.from_numpy(t).cuda(), torch.from_numpy(np.ascontiguousarray(t.T)).cuda().T):
        got, flags, beyond = _device_hours(v, _native.TSFA_F64, 1, LENGTHS, N)
        assert flags == 0 and (beyond == -7.25).all()
        assert _same_bits(got, want)
    off = _offsets(LENGTHS)
    # NaN / NaT beyond a length is padding; inside it is the bit and a NaN; a missing first stamp takes the series
    for stamps, t_type, missing in ((t, _native.TSFA_F64, np.nan), (_stamps(), _native.TSFA_I64, NAT)):
        bad = stamps.copy()
        bad[1, 1:] = missing
        bad[3, 20:] = missing
        got, flags, _ = _device_hours(torch.from_numpy(bad).cuda(), t_type, 10 ** 9, LENGTHS, N)
        assert flags == 0 and not np.isnan(got).any()
        bad[0, 7] = missing
        bad[5, 0] = missing
        got, flags, beyond = _device_hours(torch.from_numpy(bad).cuda(), t_type, 10 ** 9, LENGTHS, N)
        assert flags == _native.TSFA_DENSE_BAD_TIME and (beyond == -7.25).all()
        assert np.flatnonzero(np.isnan(got)).tolist() == [7] + list(range(int(off[5]), int(off[6])))


def test_packer_refuses_what_the_header_lists(gpu):
    buf = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    p = buf.data_ptr()
    for kw, code in ((dict(t_type=_native.TSFA_F32), _native.TSFA_ERR_INVALID), (dict(tps=7), _native.TSFA_ERR_INVALID),
                     (dict(strides=(-1, 1)), _native.TSFA_ERR_INVALID), (dict(shape=(0, 4)), _native.TSFA_ERR_INVALID),
                     (dict(t_ptr=0), _native.TSFA_ERR_INVALID), (dict(shape=(1, 33_554_432)), _native.TSFA_ERR_TOO_LONG)):
        a = dict(dict(t_ptr=p, t_type=_native.TSFA_I64, tps=10 ** 9, shape=(2, 4), strides=(4, 1)), **kw)
        with pytest.raises(_native.NativeError) as ei:
            _native.pack_times(a["t_ptr"], a["t_type"], a["tps"], a["shape"], a["strides"], p, p, p, device=0)
        assert ei.value.code == code, kw


def _check_frame(feats, cols, frame):
    got = feats.cpu().numpy()
    assert feats.is_cuda and feats.dtype == torch.float64 and not (got == conftest.SENTINEL).any()
    assert cols == list(frame.columns)
    pd.testing.assert_frame_equal(pd.DataFrame(got, index=frame.index, columns=cols), frame, check_exact=True)
    return got


@pytest.mark.parametrize("ragged", (False, True), ids=("dense", "ragged"))
@pytest.mark.parametrize("which", ("minimal", "adf"))
def test_plain_entry_equals_the_datetime_frame_and_the_oracle(gpu, which, ragged):
    x, t = _samples(), _stamps()
    lengths = LENGTHS if ragged else np.full(B, N)
    frame = _frame_features(which, ragged)
    assert sum("linear_trend_timewise" in c for c in frame.columns) == 5 * C
    forms = [dict(times=torch.from_numpy(t).cuda()), dict(times=t.view("datetime64[ns]")),
             dict(times=torch.from_numpy(np.ascontiguousarray(t.T)).cuda().T)]
    for kw in forms:
        feats, cols = extract_features_tensor(torch.from_numpy(x).cuda(), lengths=torch.from_numpy(lengths).cuda() if ragged else None,
                                              kinds=KINDS, default_fc_parameters=SETTINGS[which], **kw)
        got = _check_frame(feats, cols, frame)
    # the timewise columns against the oracle, within the tolerances of tests/parity.py
    hours = _pandas_hours(t, lengths, "ns")
    off = _offsets(lengths)
    for c, kind in enumerate(KINDS):
        values = np.concatenate([x[b, c, :lengths[b]] for b in range(B)]).astype(np.float64)
        names, want = oracle_engine(TIMEWISE, values, off, kind=kind, times=hours)
        assert len(names) == 5
        bad = compare(names, got[:, [cols.index(nm) for nm in names]], want, [values[off[i]:off[i + 1]] for i in range(B)])
        assert not bad, bad[:10]


def test_other_units_and_float_seconds_reach_the_same_features(gpu):
    x = torch.from_numpy(_samples()).cuda()
    for unit in ("us", "ms", "s"):
        t = _stamps(unit)
        frame = extract_features(_frame(_samples(), t, LENGTHS, unit), column_id="id", default_fc_parameters=MINIMAL_TIMED, pack="host",
                                 device=0)
        for kw in (dict(times=torch.from_numpy(t).cuda(), time_unit=unit), dict(times=t.view("datetime64[%s]" % unit))):
            feats, cols = extract_features_tensor(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, **kw)
            _check_frame(feats, cols, frame)
    # whole seconds as float64: the same hours, so the same frame
    feats, cols = extract_features_tensor(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED,
                                          times=_stamps("s").astype(np.float64))
    _check_frame(feats, cols, frame)
    # one clock for the batch
    shared = np.broadcast_to(_stamps()[2], (B, N))
    frame = extract_features(_frame(_samples(), shared, LENGTHS), column_id="id", default_fc_parameters=MINIMAL_TIMED, pack="host", device=0)
    feats, cols = extract_features_tensor(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED,
                                          times=torch.from_numpy(_stamps()[2].copy()).cuda())
    _check_frame(feats, cols, frame)


def test_comprehensive_has_788_columns_per_kind(gpu):
    x, t = torch.from_numpy(_samples()).cuda(), torch.from_numpy(_stamps()).cuda()
    feats, cols = extract_features_tensor(x, kinds=KINDS, times=t)
    plain, cols0 = extract_features_tensor(x, kinds=KINDS)
    assert tuple(feats.shape) == (B, 2 * 788) and tuple(plain.shape) == (B, 2 * 783)
    keep = [j for j, c in enumerate(cols) if "linear_trend_timewise" not in c]
    assert [cols[j] for j in keep] == cols0
    assert _same_bits(feats[:, keep].cpu().numpy(), plain.cpu().numpy())   # the other 783 do not move
    assert not (feats.cpu().numpy() == conftest.SENTINEL).any()


@pytest.mark.parametrize("direction", (1, -1))
@pytest.mark.parametrize("ragged", (False, True), ids=("dense", "ragged"))
def test_rolled_entry_equals_the_datetime_frame(gpu, direction, ragged):
    x, t = _samples(), _stamps()
    lengths = LENGTHS if ragged else np.full(B, N)
    roll = dict(rolling_direction=direction, max_timeshift=4)
    frame = extract_rolled_features(_frame(x, t, lengths), column_id="id", default_fc_parameters=ADF_TIMED, pack="host", device=0, **roll)
    feats, cols, series, positions = extract_rolled_features_tensor(
        torch.from_numpy(x).cuda(), lengths=lengths if ragged else None, kinds=KINDS, default_fc_parameters=ADF_TIMED,
        times=torch.from_numpy(t).cuda(), **roll)
    assert list(zip(series.tolist(), positions.tolist())) == list(frame.index)
    assert sum("linear_trend_timewise" in c for c in cols) == 5 * C
    _check_frame(feats, cols, frame)


@pytest.mark.filterwarnings("ignore:.*Constant features")
def test_relevant_entry_selects_on_the_timed_matrix(gpu):
    x, t = torch.from_numpy(_samples()).cuda(), torch.from_numpy(_stamps()).cuda()
    y = np.arange(B, dtype=np.float64)   # the trend of series b grows with b: the timewise slope is relevant
    for params, sel in ((None, dict(fdr_level=0.5)), (MINIMAL_TIMED, dict(fdr_level=0.5, hypotheses_independent=True))):
        feats, cols = extract_features_tensor(x, kinds=KINDS, default_fc_parameters=params, times=t)
        assert len(cols) == 2 * (788 if params is None else len(MINIMAL_TIMED) + 4)
        impute_tensor(feats)
        want, want_names, _ = select_features_tensor(feats, y, columns=cols, **sel)
        got, names = extract_relevant_features_tensor(x, y, kinds=KINDS, default_fc_parameters=params, times=t, **sel)
        assert names == want_names and _same_bits(got.cpu().numpy(), want.cpu().numpy())
    assert any("linear_trend_timewise" in nm for nm in names), names
    # the unit travels with the clock
    tu = torch.from_numpy(_stamps("us")).cuda()
    got_us, names_us = extract_relevant_features_tensor(x, y, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, times=tu, time_unit="us", **sel)
    feats_us, cols_us = extract_features_tensor(x, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, times=tu, time_unit="us")
    assert _same_bits(got_us.cpu().numpy(), feats_us[:, [cols_us.index(nm) for nm in names_us]].cpu().numpy())


def test_nat_raises_under_check_nan_and_is_nan_cells_without(gpu):
    x = torch.from_numpy(_samples()).cuda()
    t = _stamps().copy()
    t[1, 1:] = NAT   # beyond the lengths: padding
    t[3, 30] = NAT
    clean, cols = extract_features_tensor(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, times=t)
    _check_frame(clean, cols, _frame_features("minimal", True))
    t[4, 9] = NAT
    for entry, kw in ((extract_features_tensor, {}), (extract_rolled_features_tensor, dict(max_timeshift=4))):
        with pytest.raises(ValueError, match="times must not contain NaT / NaN"):
            entry(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, times=t, **kw)
    feats, _ = extract_features_tensor(x, lengths=LENGTHS, kinds=KINDS, default_fc_parameters=MINIMAL_TIMED, times=t, check_nan=False)
    got, want = feats.cpu().numpy(), clean.cpu().numpy()
    timewise = np.array(["linear_trend_timewise" in c for c in cols])
    assert np.isnan(got[4][timewise]).all()
    rest = np.ones_like(got, dtype=bool)
    rest[4, timewise] = False
    assert np.array_equal(got[rest].view(np.uint64), want[rest].view(np.uint64))   # every other cell is unchanged
