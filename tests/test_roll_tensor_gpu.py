"""`extract_rolled_features_tensor` on the device: values, names and window index equal those of
`extract_rolled_features(wide frame, pack="host")` bit for bit.

Why bit equality is a fair demand: a launch sizes its workgroups by the lengths of ITS batch, and the workgroup size decides
the association of the reductions.  The tensor entry extracts all windows of a kind in one launch; the host form cuts a batch
into row chunks (tsfa_extract_chunks).  Every case here stays below the window count at which that is more than one chunk --
asserted through tsfa_extract_chunks itself -- so both sides launch the same kernels on the same batch."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import conftest
from tsfresh_amd import EfficientFCParameters, _native, extract_rolled_features, extract_rolled_features_tensor
from tsfresh_amd.feature_extraction import extraction
from tsfresh_amd.feature_extraction.plan import compile_fc_parameters

pytestmark = pytest.mark.gpu

B, C, N = 6, 2, 24
KINDS = ["ax", "ay"]
PARAMS = EfficientFCParameters()
ADF_TWO_LAGS = {"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"}, {"attr": "pvalue", "autolag": "BIC"},
                                                          {"attr": "usedlag", "autolag": "AIC"}], "maximum": None}


@functools.lru_cache(maxsize=None)
def _samples():
    """(B, C, N) float32 samples on the host."""
    return (np.random.default_rng(29).standard_normal((B, C, N)) * 3.0 + 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _lengths():
    lens = np.random.default_rng(31).integers(1, N + 1, size=B)
    lens[1], lens[-1] = 1, N
    return lens


def _frame(host, lens):
    cols = {"id": np.repeat(np.arange(B), lens), "t": np.concatenate([np.arange(L) for L in lens])}
    for c, kind in enumerate(KINDS):
        cols[kind] = np.concatenate([host[b, c, :lens[b]] for b in range(B)])
    return pd.DataFrame(cols)


def _one_chunk(params, n_windows):
    """The host form extracts n_windows windows of these settings as ONE chunk (on every native plan behind them)."""
    nplan = extraction._acquire_plan(compile_fc_parameters(params, has_datetime_index=False), 0)
    lib = _native.load()
    edges = (ctypes.c_int64 * 17)()
    plans = [pl for pl, _ in nplan.parts] if isinstance(nplan, extraction._CompositePlan) else [nplan]
    return all(lib.tsfa_extract_chunks(pl._h, n_windows, edges, 17) == 1 for pl in plans)


def _check(got, host, lens, params, **roll):
    feats, cols, series, positions = got
    want = extract_rolled_features(_frame(host, lens), column_id="id", column_sort="t", default_fc_parameters=params, pack="host",
                                   device=0, **roll)
    assert len(want) > 0 and _one_chunk(params, len(want))
    assert feats.is_cuda and feats.dtype == torch.float64 and tuple(feats.shape) == want.shape
    assert series.is_cuda and positions.is_cuda and series.dtype == torch.int64 and positions.dtype == torch.int64
    assert cols == list(want.columns)
    assert list(zip(series.tolist(), positions.tolist())) == list(want.index)
    values = feats.cpu().numpy()
    assert not (values == conftest.SENTINEL).any()
    assert np.array_equal(values, want.to_numpy(), equal_nan=True)
    return want


def test_bcn_float32(gpu):
    host = _samples()
    roll = dict(rolling_direction=1, max_timeshift=7, min_timeshift=3)
    xd = torch.from_numpy(host).to("cuda:0")
    before = xd.clone()
    got = extract_rolled_features_tensor(xd, kinds=KINDS, default_fc_parameters=PARAMS, **roll)
    want = _check(got, host, np.full(B, N), PARAMS, **roll)
    assert len(want) == B * (N - 3) and got[0].shape[0] % B == 0
    dense = got[0].view(B, N - 3, -1)                      # the [B, W, F] form of a batch without lengths
    assert torch.equal(got[2].view(B, N - 3), torch.arange(B, device="cuda:0")[:, None].expand(B, N - 3))
    assert torch.equal(got[3].view(B, N - 3)[0], torch.arange(3, N, device="cuda:0")) and dense.shape[2] == len(got[1])
    assert torch.equal(xd, before)


def test_channels_last_bfloat16(gpu):
    x = torch.from_numpy(_samples()).to(torch.bfloat16)
    host = x.to(torch.float32).numpy()                      # the frame of the converted samples
    roll = dict(rolling_direction=1, max_timeshift=7, min_timeshift=3)
    got = extract_rolled_features_tensor(x.to("cuda:0").permute(0, 2, 1).contiguous(), kinds=KINDS, channels_last=True,
                                         default_fc_parameters=PARAMS, **roll)
    _check(got, host, np.full(B, N), PARAMS, **roll)


@pytest.mark.parametrize("roll", (dict(rolling_direction=2), dict(rolling_direction=-1, max_timeshift=9, min_timeshift=0)),
                         ids=("dir2", "dir-1"))
def test_lengths(gpu, roll):
    host, lens = _samples(), _lengths()
    assert lens.min() == 1 and lens.max() == N
    got = extract_rolled_features_tensor(torch.from_numpy(host).to("cuda:0"), lengths=torch.from_numpy(lens).to("cuda:0"),
                                         kinds=KINDS, default_fc_parameters=PARAMS, **roll)
    _check(got, host, lens, PARAMS, **roll)
    # a shorter batch: the longest LENGTH, not n, sizes the shifts
    short = np.minimum(lens, N - 1)
    got = extract_rolled_features_tensor(host, lengths=short, kinds=KINDS, default_fc_parameters=PARAMS, device=0, **roll)
    _check(got, host, short, PARAMS, **roll)


@pytest.mark.parametrize("ragged", (False, True), ids=("dense", "ragged"))
def test_composite_plan(gpu, ragged):
    fplan = compile_fc_parameters(ADF_TWO_LAGS, has_datetime_index=False)
    assert isinstance(extraction._acquire_plan(fplan, 0), extraction._CompositePlan)
    host = _samples()
    lens = _lengths() if ragged else np.full(B, N)
    roll = dict(max_timeshift=15, min_timeshift=11)
    got = extract_rolled_features_tensor(torch.from_numpy(host).to("cuda:0"), lengths=lens if ragged else None, kinds=KINDS,
                                         default_fc_parameters=ADF_TWO_LAGS, **roll)
    _check(got, host, lens, ADF_TWO_LAGS, **roll)


def test_plan_extract_windows_into_equals_extract_windows_host(gpu):
    rng = np.random.default_rng(37)
    values = rng.standard_normal(900).astype(np.float32)
    size = rng.integers(16, 65, size=40)
    starts = rng.integers(0, 900 - 64, size=40).astype(np.int64)
    ends = starts + size
    nplan = extraction._acquire_plan(compile_fc_parameters(PARAMS, has_datetime_index=False), 0)
    assert isinstance(nplan, _native.Plan) and _one_chunk(PARAMS, 40)
    want = np.array(nplan.extract_windows_host(values, starts, ends))
    vd, sd, ed = (torch.from_numpy(a).to("cuda:0") for a in (values, starts, ends))
    out = torch.full((40, nplan.n_cols + 3), -5.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    matrix = _native.BorrowedMatrix(out.data_ptr(), 40, nplan.n_cols + 3, 0, owner=out)
    nplan.extract_windows_into(vd.data_ptr(), _native.TSFA_F32, sd.data_ptr(), ed.data_ptr(), 40, matrix, col0=2)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 2:2 + nplan.n_cols], want, equal_nan=True) and not (got == conftest.SENTINEL).any()
    assert (got[:, :2] == -5.0).all() and (got[:, -1] == -5.0).all()          # the columns around the block are untouched
    with pytest.raises(ValueError, match="does not hold"):
        nplan.extract_windows_into(vd.data_ptr(), _native.TSFA_F32, sd.data_ptr(), ed.data_ptr(), 40, matrix, col0=4)
    with pytest.raises(ValueError, match="does not hold"):
        nplan.extract_windows_into(vd.data_ptr(), _native.TSFA_F32, sd.data_ptr(), ed.data_ptr(), 39, matrix, col0=0)
    nplan.extract_windows_into(vd.data_ptr(), _native.TSFA_F32, sd.data_ptr(), ed.data_ptr(), 0,
                               _native.BorrowedMatrix(out.data_ptr(), 0, nplan.n_cols, 0, owner=out))   # nothing to do


def test_no_window_at_all(gpu):
    xd = torch.from_numpy(_samples()).to("cuda:0")
    for kw in (dict(min_timeshift=N), dict(lengths=torch.full((B,), 5, device="cuda:0"), min_timeshift=5)):
        feats, cols, series, positions = extract_rolled_features_tensor(xd, kinds=KINDS, default_fc_parameters=PARAMS, **kw)
        assert len(cols) > 0 and tuple(feats.shape) == (0, len(cols)) and feats.is_cuda and feats.dtype == torch.float64
        assert tuple(series.shape) == (0,) and tuple(positions.shape) == (0,) and series.is_cuda and positions.is_cuda
