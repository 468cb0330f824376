"""`nan_policy="drop"` on the device: the three tensor entries equal the frame entries on the wide frame after `dropna()` (host
packer), cell for cell and bit for bit -- both sides run the same kernels on the same packed samples, so equality is the
expectation, not a tolerance.

37 series x 3 kinds x 130 steps, about 10 % NaN placed per kind (so about 27 % of the steps go), ragged lengths, one series
with a single kept step, NaN beyond the lengths; with stamps also a NaT on steps whose values are fine.  The rolled entry runs
on the batch cut to 40 steps."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import conftest
from tsfresh_amd import (EfficientFCParameters, MinimalFCParameters, extract_features, extract_features_tensor,
                         extract_relevant_features, extract_relevant_features_tensor, extract_rolled_features,
                         extract_rolled_features_tensor)

pytestmark = pytest.mark.gpu

B, C, N = 37, 3, 130
KINDS = ["p", "q", "r"]
NAT = np.iinfo(np.int64).min
TIMEWISE = {"linear_trend_timewise": [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]}
EFFICIENT_TIMED = dict(EfficientFCParameters(), **TIMEWISE)
ROLL_PARAMS = dict(MinimalFCParameters(), **{"augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"}],
                                             "abs_energy": None, "autocorrelation": [{"lag": 2}]})
SINGLE = 5           # the series with one kept step


@functools.lru_cache(maxsize=None)
def _batch(n=N):
    """(x float32 (B, C, n), lengths, stamps int64 (B, n), y): x[b] rises with y[b]."""
    rng = np.random.default_rng(41)
    y = (np.arange(B) % 2).astype(np.int64)
    x = (rng.standard_normal((B, C, n)) + 1.5 * y[:, None, None]).astype(np.float32)
    x[rng.random((B, C, n)) < 0.10] = np.nan
    lengths = rng.integers(n // 2, n + 1, size=B).astype(np.int64)
    lengths[0], lengths[1] = n, n // 2
    x[SINGLE, 1, :] = np.nan
    x[SINGLE, :, 17] = [0.5, -1.25, 2.0]
    for b in range(B):
        x[b, :, lengths[b]:] = np.nan                    # padding: never read
    t = 1_600_000_000 * 10 ** 9 + np.cumsum(rng.integers(1, 7_000 * 10 ** 9, size=(B, n)), axis=1)
    nat = rng.random((B, n)) < 0.03
    nat[SINGLE, 17] = False
    t[nat] = NAT
    return x, lengths, t, y   # (shared by the tests: they hand copies to torch and leave these unchanged)


def _dropped_frame(n=N, timed=False):
    """The wide frame of the batch after dropna(): id, t (the step index), the kinds; timed: the stamps are its DatetimeIndex
    (a row with a NaT stamp goes as well)."""
    x, lengths, t, _ = _batch(n)
    cols = {"id": np.repeat(np.arange(B), lengths), "t": np.concatenate([np.arange(k) for k in lengths])}
    for c, kind in enumerate(KINDS):
        cols[kind] = np.concatenate([x[b, c, :lengths[b]] for b in range(B)])
    if timed:
        cols["stamp"] = np.concatenate([t[b, :lengths[b]] for b in range(B)]).view("datetime64[ns]")
    frame = pd.DataFrame(cols).dropna()
    if timed:
        frame = frame.set_index(pd.DatetimeIndex(frame.pop("stamp")))
    assert (frame["id"] == SINGLE).sum() == 1 and 0.55 < len(frame) / lengths.sum() < 0.85
    return frame


@functools.lru_cache(maxsize=None)
def _frame_features(timed):
    """The frame entry on the dropped frame, host packer: computed once and left unchanged."""
    return extract_features(_dropped_frame(timed=timed).drop(columns="t"), column_id="id", default_fc_parameters=EFFICIENT_TIMED,
                            pack="host", device=0)


def _check(feats, cols, frame):
    assert feats.is_cuda and feats.dtype == torch.float64
    assert cols == list(frame.columns)
    want = torch.from_numpy(frame.to_numpy())
    got = feats.cpu()
    assert not (got == conftest.SENTINEL).any()
    assert got.shape == want.shape
    # every cell, none skipped: equal, or NaN on both sides
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=0.0).view(torch.int64), torch.nan_to_num(want, nan=0.0).view(torch.int64))


@pytest.mark.parametrize("timed", (False, True), ids=("plain", "times"))
def test_plain_entry_equals_the_frame_after_dropna(gpu, timed):
    x, lengths, t, _ = _batch()
    frame = _frame_features(timed)
    assert sum("linear_trend_timewise" in c for c in frame.columns) == (5 * C if timed else 0)
    kw = dict(times=torch.from_numpy(t.copy()).cuda()) if timed else {}
    feats, cols = extract_features_tensor(torch.from_numpy(x.copy()).cuda(), lengths=torch.from_numpy(lengths.copy()).cuda(), kinds=KINDS,
                                          default_fc_parameters=EFFICIENT_TIMED, nan_policy="drop", **kw)
    _check(feats, cols, frame)
    # channels-last and from the host: the same batch through another layout
    feats, cols = extract_features_tensor(np.ascontiguousarray(x.transpose(0, 2, 1)), lengths=lengths, kinds=KINDS, channels_last=True,
                                          default_fc_parameters=EFFICIENT_TIMED, nan_policy="drop", check_nan=False,
                                          **({"times": t.view("datetime64[ns]")} if timed else {}))
    _check(feats, cols, frame)


def test_default_policy_still_raises(gpu):
    x, lengths, t, _ = _batch()
    with pytest.raises(ValueError, match="Column must not contain NaN values: p$"):
        extract_features_tensor(torch.from_numpy(x.copy()).cuda(), lengths=lengths, kinds=KINDS, default_fc_parameters=MinimalFCParameters())
    xe = x.copy()
    xe[9, 2, :] = np.nan
    with pytest.raises(ValueError, match="series 9 has no step left"):
        extract_features_tensor(torch.from_numpy(xe).cuda(), lengths=lengths, kinds=KINDS, default_fc_parameters=MinimalFCParameters(),
                                nan_policy="drop")


@pytest.mark.parametrize("direction", (1, -1, 2, -2))
def test_rolled_entry_equals_the_frame_after_dropna(gpu, direction):
    n = 40
    x, lengths, _, _ = _batch(n)
    roll = dict(rolling_direction=direction, max_timeshift=7)
    frame = extract_rolled_features(_dropped_frame(n), column_id="id", column_sort="t", default_fc_parameters=ROLL_PARAMS, pack="host",
                                    device=0, **roll)
    feats, cols, series, positions = extract_rolled_features_tensor(torch.from_numpy(x.copy()).cuda(), lengths=lengths, kinds=KINDS,
                                                                    default_fc_parameters=ROLL_PARAMS, nan_policy="drop", **roll)
    assert series.is_cuda and positions.is_cuda and positions.dtype == torch.int64
    assert list(zip(series.tolist(), positions.tolist())) == list(frame.index)   # (id, ORIGINAL step index)
    _check(feats, cols, frame)


@pytest.mark.filterwarnings("ignore:.*Constant features")
def test_relevant_entry_selects_what_the_frame_chain_selects(gpu):
    x, lengths, _, y = _batch()
    want = extract_relevant_features(_dropped_frame().drop(columns="t"), pd.Series(y, index=np.arange(B)), column_id="id",
                                     default_fc_parameters=MinimalFCParameters(), pack="host", device=0)
    got, names = extract_relevant_features_tensor(torch.from_numpy(x.copy()).cuda(), y, lengths=lengths, kinds=KINDS,
                                                  default_fc_parameters=MinimalFCParameters(), nan_policy="drop")
    assert len(names) >= C and sorted(names) == sorted(want.columns)
    assert np.array_equal(got.cpu().numpy(), want[names].to_numpy())
