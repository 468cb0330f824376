"""`extract_features_tensor` above the kernels: shapes, dtypes, names, column order, the checks and their exceptions -- on CPU
tensors, with the g++ build of the dense packer's bodies standing in for the device and a numpy plan standing in for the
kernels (the manner of test_roll_device_routes.py).  No GPU needed."""
import ctypes
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import emul_pack_dense_lib as epd
import tsfresh_amd
from tsfresh_amd import MinimalFCParameters, _native, extract_features, tensor
from tsfresh_amd.feature_extraction import extraction
from tsfresh_amd.feature_extraction.registry import UnsupportedFeature


class _NumpyPlan:
    """Column j of a series is (j + 1) * its sum + its length, whichever way the samples arrive."""

    def __init__(self, n_cols):
        self.n_cols = n_cols

    def _rows(self, values, offsets):
        values = np.asarray(values, dtype=np.float64)
        base = np.array([[values[a:b].sum(), b - a] for a, b in zip(offsets[:-1], offsets[1:])], dtype=np.float64).reshape(-1, 2)
        return np.stack([(j + 1) * base[:, 0] + base[:, 1] for j in range(self.n_cols)], axis=1)

    def extract_host(self, values, offsets, times=None, out=None):
        return self._rows(values, offsets)

    def extract_into(self, values, offsets, matrix, col0=0, times=None, pack=None):
        assert values is None and offsets is None and isinstance(matrix, _native.BorrowedMatrix)
        assert matrix.ptr == matrix.owner.data_ptr() and matrix.ld == matrix.owner.shape[1]
        matrix.owner.numpy()[:, col0:col0 + self.n_cols] = self._rows(pack.values_host(), pack.offsets)


class _EmulChannel:
    def __init__(self, values, offsets, device):
        self._values, self.offsets, self.n_series, self.device = values, offsets, len(offsets) - 1, device

    def values_host(self):
        return self._values

    def close(self):
        pass


def _emul_dense_pack(torch_, x3, lengths, device):
    bf16 = x3.dtype == torch.bfloat16
    xnp = x3.view(torch.int16).numpy().view(np.uint16) if bf16 else x3.numpy()
    assert xnp.strides == tuple(s * xnp.itemsize for s in x3.stride())   # the view's own strides reach the packer
    res = epd.EmulDense(xnp, lengths=None if lengths is None else lengths.numpy(), bf16=bf16)
    assert res.status == 0 and res.guards_intact
    return [_EmulChannel(res.values[c], res.offsets, device) for c in range(x3.shape[1])], torch.tensor([res.flags], dtype=torch.int32)


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _NumpyPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_dense_pack", _emul_dense_pack)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)


def _wide_frame(x, kinds, lengths=None):
    """The wide frame that holds the samples of x (B, C, n)."""
    B, C, n = x.shape
    lens = np.full(B, n) if lengths is None else np.asarray(lengths)
    cols = {"id": np.repeat(np.arange(B), lens), "t": np.concatenate([np.arange(L) for L in lens])}
    for c, kind in enumerate(kinds):
        cols[kind] = np.concatenate([x[b, c, :lens[b]] for b in range(B)])
    return pd.DataFrame(cols)


def _x(B=4, C=3, n=9, seed=0, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((B, C, n)).astype(dtype)


def test_reexported_and_torch_stays_out_of_the_package_import():
    assert tsfresh_amd.extract_features_tensor is tensor.extract_features_tensor
    code = "import sys, tsfresh_amd, tsfresh_amd.tensor; assert 'torch' not in sys.modules, 'torch was imported'"
    subprocess.check_call([sys.executable, "-c", code])


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32, torch.float16, torch.bfloat16))
def test_names_order_and_values_equal_the_wide_frame(emulated, dtype):
    xt = torch.from_numpy(_x()).to(dtype)
    kinds = ["b", "a", "c"]
    params = MinimalFCParameters()
    wide = xt.to(torch.float64 if dtype == torch.float64 else torch.float32).numpy()
    want = extract_features(_wide_frame(wide, kinds), column_id="id", column_sort="t", default_fc_parameters=params, pack="host")
    for lay, arg in (("bcn", xt), ("bnc", xt.permute(0, 2, 1).contiguous())):
        feats, cols = tsfresh_amd.extract_features_tensor(arg, kinds=kinds, channels_last=lay == "bnc", default_fc_parameters=params)
        assert cols == list(want.columns)
        assert feats.dtype == torch.float64 and tuple(feats.shape) == want.shape
        assert np.array_equal(feats.numpy(), want.to_numpy())
    lengths = np.array([9, 1, 4, 7])
    want = extract_features(_wide_frame(wide, kinds, lengths), column_id="id", column_sort="t", default_fc_parameters=params,
                            pack="host")
    for lens in (lengths.astype(np.int32), torch.from_numpy(lengths), lengths.tolist()):
        feats, cols = tsfresh_amd.extract_features_tensor(xt, lengths=lens, kinds=kinds, default_fc_parameters=params)
        assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())


def test_default_kind_names_two_dimensional_input_and_numpy(emulated):
    x = _x()
    feats, cols = tsfresh_amd.extract_features_tensor(x, default_fc_parameters={"maximum": None, "length": None})
    assert cols == ["%d__%s" % (c, f) for c in range(3) for f in ("maximum", "length")]
    one, cols1 = tsfresh_amd.extract_features_tensor(x[:, 1, :], default_fc_parameters={"maximum": None, "length": None})
    assert cols1 == ["0__maximum", "0__length"] and torch.equal(one, feats[:, 2:4])
    # a strided view is taken as it is
    big = _x(B=8, C=3, n=20, seed=4)
    view = torch.from_numpy(big)[1::2, :, 2:20:2]
    a, _ = tsfresh_amd.extract_features_tensor(view, default_fc_parameters=MinimalFCParameters())
    b, _ = tsfresh_amd.extract_features_tensor(view.contiguous(), default_fc_parameters=MinimalFCParameters())
    assert torch.equal(a, b)
    ex, _ = tsfresh_amd.extract_features_tensor(torch.from_numpy(x[:1]).expand(5, 3, 9), default_fc_parameters=MinimalFCParameters())
    assert tuple(ex.shape)[0] == 5 and torch.equal(ex[0], ex[4])


def test_kind_to_fc_parameters(emulated):
    x = _x()
    feats, cols = tsfresh_amd.extract_features_tensor(
        x, kinds=["u", "v", "w"], default_fc_parameters={"maximum": None},
        kind_to_fc_parameters={"v": {"length": None, "minimum": None}, "w": {}})
    assert cols == ["u__maximum", "v__length", "v__minimum"] and tuple(feats.shape) == (4, 3)
    want = extract_features(_wide_frame(x, ["u", "v", "w"]), column_id="id", column_sort="t", default_fc_parameters={"maximum": None},
                            kind_to_fc_parameters={"v": {"length": None, "minimum": None}, "w": {}}, pack="host")
    assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())
    none, cols = tsfresh_amd.extract_features_tensor(x, kind_to_fc_parameters={"7": {"length": None}})
    assert cols == [] and tuple(none.shape) == (4, 0)


@pytest.mark.parametrize("bad", (np.zeros((2, 3), dtype=np.int64), np.zeros((2, 3), dtype=bool), np.zeros((2, 3), dtype=np.complex64),
                                 torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3), dtype=torch.bool),
                                 torch.zeros((2, 3), dtype=torch.complex64)))
def test_type_errors_name_the_dtype(emulated, bad):
    with pytest.raises(TypeError, match=str(bad.dtype).replace("torch.", "")):
        tsfresh_amd.extract_features_tensor(bad, default_fc_parameters=MinimalFCParameters())


def test_value_errors(emulated):
    params = MinimalFCParameters()
    x = _x()
    for bad in (x[0, 0], x[None]):
        with pytest.raises(ValueError, match="dimensions"):
            tsfresh_amd.extract_features_tensor(bad, default_fc_parameters=params)
    for lens in (np.array([9, 9, 9]), np.full((4, 1), 9), np.full(5, 9)):
        with pytest.raises(ValueError, match="one entry per series"):
            tsfresh_amd.extract_features_tensor(x, lengths=lens, default_fc_parameters=params)
    with pytest.raises(TypeError, match="integers"):
        tsfresh_amd.extract_features_tensor(x, lengths=np.full(4, 9.0), default_fc_parameters=params)
    for bad in (0, -1, 10):
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 9\]"):
            tsfresh_amd.extract_features_tensor(x, lengths=np.array([9, bad, 1, 2]), default_fc_parameters=params, check_nan=False)
    with pytest.raises(ValueError, match="3 kinds"):
        tsfresh_amd.extract_features_tensor(x, kinds=["a", "b"], default_fc_parameters=params)
    with pytest.raises(ValueError, match="not allowed to contain '__'"):
        tsfresh_amd.extract_features_tensor(x, kinds=["a", "b__c", "d"], default_fc_parameters=params)
    with pytest.raises(ValueError, match="not allowed to end with '_'"):
        tsfresh_amd.extract_features_tensor(x, kinds=["a", "b_", "d"], default_fc_parameters=params)


def test_nan_names_the_kind_and_check_nan_false_skips_it(emulated):
    params = MinimalFCParameters()
    x = _x()
    x[2, 1, 5] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: v$"):
        tsfresh_amd.extract_features_tensor(x, kinds=["u", "v", "w"], default_fc_parameters=params)
    with pytest.raises(ValueError, match="Column must not contain NaN values: 1$"):
        tsfresh_amd.extract_features_tensor(np.ascontiguousarray(x.transpose(0, 2, 1)), channels_last=True, default_fc_parameters=params)
    feats, _ = tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, check_nan=False)
    assert torch.isnan(feats).any()
    # beyond the series' length the NaN is padding
    feats, _ = tsfresh_amd.extract_features_tensor(x, lengths=np.array([9, 9, 5, 9]), default_fc_parameters=params)
    assert not torch.isnan(feats).any()


def test_callable_calculators_are_refused(emulated):
    def my_feature(x):
        return 0.0
    with pytest.raises(UnsupportedFeature, match="callable"):
        tsfresh_amd.extract_features_tensor(_x(), default_fc_parameters={"maximum": None, my_feature: None})


def test_without_a_device_the_real_call_is_an_error_not_a_cpu_route():
    _native.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    if _native.device_count() > 0:
        # (a HIP device is present: a null pointer is refused before anything is launched)
        with pytest.raises(_native.NativeError) as ei:
            _native.pack_dense(0, _native.TSFA_F32, (1, 1, 4), (4, 4, 1), p, 4, p, p)
        assert ei.value.code == _native.TSFA_ERR_INVALID
        return
    with pytest.raises(_native.NativeError) as ei:
        _native.pack_dense(p, _native.TSFA_F32, (1, 1, 4), (4, 4, 1), p, 4, p, p)
    assert ei.value.code == _native.TSFA_ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)
    with pytest.raises(_native.NativeError) as ei:
        tsfresh_amd.extract_features_tensor(_x(), default_fc_parameters=MinimalFCParameters())
    assert ei.value.code == _native.TSFA_ERR_NO_DEVICE


def test_half_types_stay_refused_everywhere_else():
    """TSFA_F16 / TSFA_BF16 are tsfa_pack_dense's alone: the frame packer's table does not know them."""
    assert _native.TSFA_F16 not in _native._DEVICE_PACK_TYPES.values() and _native.TSFA_BF16 not in _native._DEVICE_PACK_TYPES.values()
    assert _native.pack_column(np.zeros(3, dtype=np.float16)) is None
    lib = _native.load()
    col = np.zeros(4, dtype=np.int64)
    handle = ctypes.c_void_p()
    for half in (_native.TSFA_F16, _native.TSFA_BF16):
        rc = lib.tsfa_pack_device(col.ctypes.data_as(ctypes.c_void_p), _native.TSFA_I64, None, 0, col.ctypes.data_as(ctypes.c_void_p),
                                  half, 4, _native.TSFA_HOST, 0, 0, ctypes.byref(handle))
        assert rc == _native.TSFA_ERR_INVALID and not handle.value
        assert b"unknown element type" in lib.tsfa_last_error()
