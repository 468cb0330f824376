"""`extract_features_tensor` on the device: for every element type and both layouts the feature tensor is bit-equal to
`extract_features(frame, pack="host")` on the wide frame of the same samples and to `Plan.extract_host` per kind (64 series:
one chunk of the host pipeline, so the launches coincide); ragged lengths; a settings object that needs a composite plan;
the ordering contract with a producer on a side stream; x stays untouched."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import conftest
from tsfresh_amd import EfficientFCParameters, extract_features, extract_features_tensor
from tsfresh_amd.feature_extraction import extraction
from tsfresh_amd.feature_extraction.plan import compile_fc_parameters

pytestmark = pytest.mark.gpu

B, C, N = 64, 3, 257
KINDS = ["ax", "ay", "az"]
DTYPES = {"float64": torch.float64, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
PARAMS = EfficientFCParameters()
ADF_TWO_LAGS = {"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"}, {"attr": "pvalue", "autolag": "BIC"},
                                                          {"attr": "usedlag", "autolag": "AIC"}], "maximum": None}


@functools.lru_cache(maxsize=None)
def _samples(dtype_name):
    """(B, C, N) CPU tensor of the named dtype and its host image in the type the packer hands the kernels."""
    base = torch.from_numpy(np.random.default_rng(17).standard_normal((B, C, N)) * 3.0 + 1.0)
    x = base.to(DTYPES[dtype_name])
    return x, x.to(torch.float64 if dtype_name == "float64" else torch.float32).numpy()


@functools.lru_cache(maxsize=None)
def _lengths():
    lens = np.random.default_rng(23).integers(1, N + 1, size=B)
    lens[0], lens[-1] = 1, N
    return lens


def _frame(host, lens):
    cols = {"id": np.repeat(np.arange(B), lens), "t": np.concatenate([np.arange(L) for L in lens])}
    for c, kind in enumerate(KINDS):
        cols[kind] = np.concatenate([host[b, c, :lens[b]] for b in range(B)])
    return pd.DataFrame(cols)


@functools.lru_cache(maxsize=None)
def _reference(dtype_name, ragged, which="efficient"):
    """The frame route and the per-kind plan route on the same samples, computed once and left unchanged."""
    _, host = _samples(dtype_name)
    lens = _lengths() if ragged else np.full(B, N)
    params = PARAMS if which == "efficient" else ADF_TWO_LAGS
    frame = extract_features(_frame(host, lens), column_id="id", column_sort="t", default_fc_parameters=params, pack="host", device=0)
    fplan = compile_fc_parameters(params, has_datetime_index=False)
    nplan = extraction._acquire_plan(fplan, 0)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    per_kind = [np.array(nplan.extract_host(np.concatenate([host[b, c, :lens[b]] for b in range(B)]), offsets)) for c in range(C)]
    return frame, np.concatenate(per_kind, axis=1)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check(feats, cols, dtype_name, ragged, which="efficient"):
    frame, per_kind = _reference(dtype_name, ragged, which)
    assert feats.is_cuda and feats.dtype == torch.float64 and tuple(feats.shape) == frame.shape
    got = feats.cpu().numpy()
    assert not (got == conftest.SENTINEL).any()
    assert cols == list(frame.columns)
    pd.testing.assert_frame_equal(pd.DataFrame(got, index=frame.index, columns=cols), frame, check_exact=True)
    assert _same_bits(got, frame.to_numpy()) and _same_bits(got, per_kind)


@pytest.mark.parametrize("ragged", (False, True), ids=("dense", "ragged"))
@pytest.mark.parametrize("layout", ("bcn", "bnc"))
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_equals_the_frame_route_and_the_plan_route(gpu, dtype_name, layout, ragged):
    x, _ = _samples(dtype_name)
    xd = x.to("cuda:0")
    if layout == "bnc":
        xd = xd.permute(0, 2, 1).contiguous()
    before = xd.clone()
    lengths = torch.from_numpy(_lengths()).to("cuda:0") if ragged else None
    feats, cols = extract_features_tensor(xd, lengths=lengths, kinds=KINDS, channels_last=layout == "bnc",
                                          default_fc_parameters=PARAMS)
    _check(feats, cols, dtype_name, ragged)
    assert torch.equal(xd, before)   # x is unchanged (no NaN among the samples: equal values are equal bits up to the sign of zero)


@pytest.mark.parametrize("dtype_name", ("float64", "bfloat16"))
def test_host_inputs_and_views(gpu, dtype_name):
    x, host = _samples(dtype_name)
    feats, cols = extract_features_tensor(x, kinds=KINDS, default_fc_parameters=PARAMS, device=0)          # a CPU tensor
    _check(feats, cols, dtype_name, False)
    if dtype_name == "float64":
        feats, cols = extract_features_tensor(host, lengths=_lengths(), kinds=KINDS, default_fc_parameters=PARAMS)   # numpy
        _check(feats, cols, dtype_name, True)
    big = torch.full((2 * B, C + 1, 2 * N + 1), float("nan"), dtype=x.dtype, device="cuda:0")
    view = big[::2, 1:, 1::2]
    view.copy_(x)
    feats, cols = extract_features_tensor(view, kinds=KINDS, default_fc_parameters=PARAMS)                 # a stepped, offset view
    _check(feats, cols, dtype_name, False)


@pytest.mark.parametrize("ragged", (False, True), ids=("dense", "ragged"))
def test_composite_plan(gpu, ragged):
    fplan = compile_fc_parameters(ADF_TWO_LAGS, has_datetime_index=False)
    assert isinstance(extraction._acquire_plan(fplan, 0), extraction._CompositePlan)
    for dtype_name in ("float64", "float16"):
        x, _ = _samples(dtype_name)
        lengths = _lengths().astype(np.int32) if ragged else None
        feats, cols = extract_features_tensor(x.to("cuda:0").permute(0, 2, 1).contiguous(), lengths=lengths, kinds=KINDS,
                                              channels_last=True, default_fc_parameters=ADF_TWO_LAGS)
        _check(feats, cols, dtype_name, ragged, "adf")


def test_x_produced_on_a_side_stream_just_before_the_call(gpu):
    x, _ = _samples("float32")
    xd = x.to("cuda:0")
    filler = torch.randn((4096, 4096), device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        for _ in range(4):
            filler = filler @ filler * 1e-3          # work ahead of the producer on the same stream
        y = (xd * 2.0 + 0.5).permute(0, 2, 1).contiguous()
        feats, cols = extract_features_tensor(y, kinds=KINDS, channels_last=True, default_fc_parameters=PARAMS)
    torch.cuda.synchronize()
    again, _ = extract_features_tensor(y, kinds=KINDS, channels_last=True, default_fc_parameters=PARAMS)
    assert torch.equal(feats.view(torch.int64), again.view(torch.int64))
    want, _ = extract_features_tensor((x * 2.0 + 0.5), kinds=KINDS, default_fc_parameters=PARAMS, device=0)
    assert torch.equal(feats.view(torch.int64), want.view(torch.int64))


def test_checks_on_the_device(gpu):
    x, _ = _samples("bfloat16")
    xd = x.to("cuda:0").clone()
    with pytest.raises(ValueError, match=r"lengths must lie in \[1, 257\]"):
        extract_features_tensor(xd, lengths=torch.full((B,), N + 1, device="cuda:0"), default_fc_parameters=PARAMS)
    xd[5, 1, 200] = float("nan")
    with pytest.raises(ValueError, match="Column must not contain NaN values: ay$"):
        extract_features_tensor(xd, kinds=KINDS, default_fc_parameters=PARAMS)
    lengths = torch.full((B,), N, device="cuda:0")
    lengths[5] = 200
    feats, _ = extract_features_tensor(xd, lengths=lengths, kinds=KINDS, default_fc_parameters={"mean": None, "length": None})
    assert not torch.isnan(feats).any() and feats[5, 1].item() == 200.0
    feats, _ = extract_features_tensor(xd, kinds=KINDS, default_fc_parameters={"mean": None}, check_nan=False)
    assert torch.isnan(feats[5, 1]).item() and int(torch.isnan(feats).sum()) == 1
