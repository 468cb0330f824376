"""`nan_policy="drop_per_kind"` on the device: `extract_features_tensor` equals `extract_features` on the LONG frame of the batch
after `dropna()` (host packer), cell for cell -- both sides run the same kernels on the same kept samples, so equality is the
expectation, not a tolerance.

6 series x 3 kinds x 70 steps, about 15 % NaN placed per kind, ragged lengths, NaN beyond the lengths, one (series, kind)
pair without a kept step (NaN cells in that kind only, the row stays); with stamps also a NaT on steps whose values are fine."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tsfresh_amd import (EfficientFCParameters, MinimalFCParameters, extract_features, extract_features_tensor,
                         extract_rolled_features_tensor)

pytestmark = pytest.mark.gpu

B, C, N = 6, 3, 70
KINDS = ["p", "q", "r"]
NAT = np.iinfo(np.int64).min
TIMEWISE = {"linear_trend_timewise": [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]}
EMPTY = (2, 1)       # the (series, kind) without a kept step


@functools.lru_cache(maxsize=None)
def _batch():
    rng = np.random.default_rng(43)
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    x[rng.random((B, C, N)) < 0.15] = np.nan
    lengths = rng.integers(N // 2, N + 1, size=B).astype(np.int64)
    lengths[0] = N
    x[EMPTY[0], EMPTY[1], :] = np.nan
    for b in range(B):
        x[b, :, lengths[b]:] = np.nan                    # padding: never read
    t = 1_600_000_000 * 10 ** 9 + np.cumsum(rng.integers(1, 7_000 * 10 ** 9, size=(B, N)), axis=1)
    t[rng.random((B, N)) < 0.05] = NAT
    return x, lengths, t   # (shared by the tests: they hand copies to torch and leave these unchanged)


def _long_frame_features(timed, params):
    """The frame entry on the melted batch after dropna(): one row per (id, step, kind, value), the stamps its DatetimeIndex."""
    x, lengths, t, = _batch()
    b, c, s = (a.reshape(-1) for a in np.meshgrid(np.arange(B), np.arange(C), np.arange(N), indexing="ij"))
    inside = s < lengths[b]
    cols = {"id": b[inside], "t": s[inside], "kind": np.asarray(KINDS)[c[inside]], "value": x.reshape(-1)[inside]}
    if timed:
        cols["stamp"] = t[b, s][inside].view("datetime64[ns]")
    frame = pd.DataFrame(cols).dropna()
    if timed:
        frame = frame.set_index(pd.DatetimeIndex(frame.pop("stamp")))
    assert not ((frame["id"] == EMPTY[0]) & (frame["kind"] == KINDS[EMPTY[1]])).any() and len(frame) < 0.9 * inside.sum()
    return extract_features(frame, column_id="id", column_sort="t", column_kind="kind", column_value="value",
                            default_fc_parameters=params, pack="host", device=0)


@pytest.mark.parametrize("timed", (False, True), ids=("plain", "times"))
def test_entry_equals_the_long_frame_after_dropna(gpu, timed):
    x, lengths, t = _batch()
    params = dict(EfficientFCParameters(), **(TIMEWISE if timed else {}))
    frame = _long_frame_features(timed, params)
    want = torch.from_numpy(frame.to_numpy())
    kw = dict(times=torch.from_numpy(t.copy()).cuda()) if timed else {}
    forms = [dict(x=torch.from_numpy(x.copy()).cuda()),
             dict(x=np.ascontiguousarray(x.transpose(0, 2, 1)), channels_last=True)]
    for form in forms:
        feats, cols = extract_features_tensor(lengths=lengths, kinds=KINDS, default_fc_parameters=params,
                                              nan_policy="drop_per_kind", **form, **kw)
        got = feats.cpu()
        assert cols == list(frame.columns) and got.shape == want.shape == (B, len(cols))
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert bool((got[~torch.isnan(want)] == want[~torch.isnan(want)]).all())
        # the pair without a kept step: NaN in that kind's cells only (some calculators are NaN on their own elsewhere)
        width = len(cols) // C
        block = torch.isnan(got[EMPTY[0]]).view(C, width)
        assert block[EMPTY[1]].all() and not block[0].all() and not block[2].all()


def test_a_series_empty_in_every_kind_is_a_value_error_with_its_index(gpu):
    x, lengths, _ = _batch()
    x = x.copy()
    x[4] = np.nan
    with pytest.raises(ValueError, match="series 4 has no step left after nan_policy='drop_per_kind'"):
        extract_features_tensor(torch.from_numpy(x).cuda(), lengths=lengths, kinds=KINDS, default_fc_parameters=MinimalFCParameters(),
                                nan_policy="drop_per_kind")
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 70\]"):   # reported first
        extract_features_tensor(torch.from_numpy(x).cuda(), lengths=[70, 0, 3, 3, 3, 3], default_fc_parameters=MinimalFCParameters(),
                                nan_policy="drop_per_kind")


def test_the_rolled_entry_refuses_the_value(gpu):
    x, _, _ = _batch()
    with pytest.raises(ValueError, match="drop_per_kind.*every kind would keep its own steps"):
        extract_rolled_features_tensor(x, max_timeshift=3, default_fc_parameters=MinimalFCParameters(), nan_policy="drop_per_kind")


def test_a_multi_rate_batch_keeps_every_sensor_s_own_steps(gpu):
    """Two sensors pivoted onto one grid that never line up: the wide rule keeps nothing, the per-kind rule everything."""
    x = np.random.default_rng(3).standard_normal((4, 2, 40))
    x[:, 0, 1::2] = np.nan
    x[:, 1, 0::2] = np.nan
    with pytest.raises(ValueError, match="series 0 has no step left"):
        extract_features_tensor(x, default_fc_parameters=MinimalFCParameters(), nan_policy="drop")
    feats, cols = extract_features_tensor(x, default_fc_parameters=MinimalFCParameters(), nan_policy="drop_per_kind")
    assert feats.shape == (4, len(cols)) and not torch.isnan(feats).any()
    got = dict(zip(cols, feats.cpu().numpy().T))
    assert np.array_equal(got["0__length"], np.full(4, 20.0)) and np.array_equal(got["1__length"], np.full(4, 20.0))
    kept = x[:, 0, 0::2]   # a float64 sum of 20 terms, in any order: within 20 ulp of the sum of magnitudes
    assert (np.abs(got["0__sum_values"] - kept.sum(axis=1)) <= 20 * 2.0 ** -52 * np.abs(kept).sum(axis=1)).all()
