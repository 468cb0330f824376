"""`extract_rolled_features_tensor` above the kernels: names, column order, window order, the (series, position) pair of every
window, the checks and their exceptions -- on CPU tensors, with the g++ builds of the dense packer's and the window builder's
bodies standing in for the device and a numpy plan standing in for the kernels (the manner of test_tensor_entry_routes.py).
The reference of every case is `extract_rolled_features` on the equivalent wide frame, host route, under the same stand-in
plan.  No GPU needed."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import emul_pack_dense_lib as epd
import emul_roll_dense_lib as erd
import tsfresh_amd
from tsfresh_amd import MinimalFCParameters, _native, extract_rolled_features, tensor
from tsfresh_amd.feature_extraction import extraction
from tsfresh_amd.feature_extraction.registry import UnsupportedFeature


def _at(ptr, n, ctype, dtype):
    """n elements at address `ptr` as a numpy array (the stand-in plan is handed raw pointers, like the native one)."""
    if n == 0:
        return np.empty(0, dtype=dtype)
    return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(ptr), ctypes.POINTER(ctype)), (n,))


class _NumpyPlan:
    """Column j of a window is (j + 1) * its sum + its length, whichever way the samples and the windows arrive."""

    def __init__(self, n_cols):
        self.n_cols = n_cols

    def _rows(self, values, starts, ends):
        values = np.asarray(values, dtype=np.float64)
        base = np.array([[values[a:b].sum(), b - a] for a, b in zip(starts, ends)], dtype=np.float64).reshape(-1, 2)
        return np.stack([(j + 1) * base[:, 0] + base[:, 1] for j in range(self.n_cols)], axis=1) if len(base) \
            else np.empty((0, self.n_cols))

    def extract_windows_host(self, values, starts, ends, times=None):
        return self._rows(values, starts, ends)

    def extract_windows_into(self, values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=0):
        assert isinstance(matrix, _native.BorrowedMatrix) and matrix.shape[0] == n_windows > 0
        assert matrix.ptr == matrix.owner.data_ptr() and matrix.ld == matrix.owner.shape[1]
        starts = _at(starts_ptr, n_windows, ctypes.c_int64, np.int64)
        ends = _at(ends_ptr, n_windows, ctypes.c_int64, np.int64)
        ctype, dtype = (ctypes.c_float, np.float32) if values_type == _native.TSFA_F32 else (ctypes.c_double, np.float64)
        values = _at(values_ptr, int(ends.max()), ctype, dtype)
        matrix.owner.numpy()[:, col0:col0 + self.n_cols] = self._rows(values, starts, ends)


class _EmulChannel:
    def __init__(self, values, offsets, device):
        self._values, self.offsets, self.n_series, self.device = np.ascontiguousarray(values), offsets, len(offsets) - 1, device
        self.values_ptr = self._values.ctypes.data
        self.values_type = _native.TSFA_F32 if self._values.dtype == np.float32 else _native.TSFA_F64

    def close(self):
        pass


def _emul_dense_pack(torch_, x3, lengths, device):
    bf16 = x3.dtype == torch.bfloat16
    xnp = x3.view(torch.int16).numpy().view(np.uint16) if bf16 else x3.numpy()
    res = epd.EmulDense(xnp, lengths=None if lengths is None else lengths.numpy(), bf16=bf16)
    assert res.status == 0 and res.guards_intact
    return [_EmulChannel(res.values[c], res.offsets, device) for c in range(x3.shape[1])], torch.tensor([res.flags], dtype=torch.int32)


_ROUTES = []


def _emul_roll_windows(torch_, pack, series_len, rolling_direction, max_timeshift, min_timeshift, steps):
    """`tensor._roll_windows` on the emulated builder: the same two calls on the same arguments."""
    _ROUTES.append("ragged" if series_len is None else "uniform")
    scanned = np.zeros(pack.n_series, dtype=np.uint32) if series_len is None else None
    kw = dict(scanned=scanned, series_len=series_len or 0)
    rc, n = erd.count(pack.offsets, pack.n_series, rolling_direction, max_timeshift, min_timeshift, steps, **kw)
    assert rc == 0
    out = np.full((4, n + erd.GUARD), erd.SENTINEL, dtype=np.int64)
    assert erd.fill(pack.offsets, pack.n_series, n, out, rolling_direction, max_timeshift, min_timeshift, steps, **kw) == 0
    assert (out[:, n:] == erd.SENTINEL).all()
    return tuple(torch.from_numpy(out[k, :n].copy()) for k in range(4))


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _NumpyPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_dense_pack", _emul_dense_pack)
    monkeypatch.setattr(tensor, "_roll_windows", _emul_roll_windows)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor, "_synchronize", lambda torch_, device: None)
    del _ROUTES[:]


def _wide_frame(x, kinds, lengths=None):
    """The wide frame that holds the samples of x (B, C, n), sort column 0 .. len - 1."""
    B, C, n = x.shape
    lens = np.full(B, n) if lengths is None else np.asarray(lengths)
    cols = {"id": np.repeat(np.arange(B), lens), "t": np.concatenate([np.arange(L) for L in lens])}
    for c, kind in enumerate(kinds):
        cols[kind] = np.concatenate([x[b, c, :lens[b]] for b in range(B)])
    return pd.DataFrame(cols)


def _x(B=4, C=3, n=9, seed=0, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((B, C, n)).astype(dtype)


def _check(got, wide, kinds, lengths=None, **kw):
    """got: what the tensor entry returned; the reference: the host route on the wide frame of `wide` (B, C, n)."""
    feats, cols, series, positions = got
    roll = {k: kw.pop(k) for k in ("rolling_direction", "max_timeshift", "min_timeshift") if k in kw}
    want = extract_rolled_features(_wide_frame(wide, kinds, lengths), column_id="id", column_sort="t", pack="host", **roll, **kw)
    assert cols == list(want.columns)
    assert feats.dtype == torch.float64 and tuple(feats.shape) == want.shape
    assert series.dtype == torch.int64 and positions.dtype == torch.int64
    assert tuple(series.shape) == tuple(positions.shape) == (want.shape[0],)
    assert list(zip(series.tolist(), positions.tolist())) == list(want.index)
    assert np.array_equal(feats.numpy(), want.to_numpy())
    if lengths is None:
        assert feats.shape[0] % wide.shape[0] == 0   # every series has the same windows: the dense [B, W, F] view exists
        assert tuple(feats.view(wide.shape[0], feats.shape[0] // wide.shape[0], -1).shape)[2] == len(cols)
    return want


ROLLS = (dict(), dict(max_timeshift=3, min_timeshift=1), dict(rolling_direction=-1, max_timeshift=4, min_timeshift=2),
         dict(rolling_direction=2, max_timeshift=5, min_timeshift=1))


def test_reexported():
    assert tsfresh_amd.extract_rolled_features_tensor is tensor.extract_rolled_features_tensor


@pytest.mark.parametrize("roll", ROLLS, ids=("all", "dir1", "dir-1", "dir2"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_layouts_and_types_equal_the_wide_frame(emulated, dtype, roll):
    xt = torch.from_numpy(_x()).to(dtype)
    wide = xt.to(torch.float32).numpy()
    kinds = ["b", "a", "c"]
    params = MinimalFCParameters()
    for arg, channels_last in ((xt, False), (xt.permute(0, 2, 1).contiguous(), True)):
        got = tsfresh_amd.extract_rolled_features_tensor(arg, kinds=kinds, channels_last=channels_last,
                                                         default_fc_parameters=params, **roll)
        want = _check(got, wide, kinds, default_fc_parameters=params, **roll)
        assert len(want) > 0
    # (B, n): one kind named "0"
    got = tsfresh_amd.extract_rolled_features_tensor(xt[:, 1, :], default_fc_parameters=params, **roll)
    _check(got, wide[:, 1:2, :], ["0"], default_fc_parameters=params, **roll)
    assert set(_ROUTES) == {"uniform"}


@pytest.mark.parametrize("roll", ROLLS, ids=("all", "dir1", "dir-1", "dir2"))
def test_lengths_with_a_series_of_one_sample(emulated, roll):
    x = _x(B=5, n=11, seed=3, dtype=np.float32)
    lengths = np.array([11, 1, 4, 7, 10])
    params = {"maximum": None, "length": None, "sum_values": None}
    for lens in (lengths.astype(np.int32), torch.from_numpy(lengths)):
        got = tsfresh_amd.extract_rolled_features_tensor(x, lengths=lens, kinds=["u", "v", "w"], default_fc_parameters=params, **roll)
        _check(got, x, ["u", "v", "w"], lengths, default_fc_parameters=params, **roll)
    assert set(_ROUTES) == {"ragged"}
    # the longest length, not n, sizes the shifts: with direction 2 the two differ in the congruence class
    short = np.array([10, 1, 4, 7, 10])
    got = tsfresh_amd.extract_rolled_features_tensor(x, lengths=short, default_fc_parameters=params, rolling_direction=2)
    _check(got, x, ["0", "1", "2"], short, default_fc_parameters=params, rolling_direction=2)
    assert set((got[3][got[2] == 0] % 2).tolist()) == {1}   # positions 1, 3, .. 9 of a series of 10: ts = 10 (mod 2)


def test_kind_to_fc_parameters_with_an_empty_settings_object(emulated):
    x = _x()
    kw = dict(default_fc_parameters={"maximum": None}, kind_to_fc_parameters={"v": {"length": None, "minimum": None}, "w": {}})
    got = tsfresh_amd.extract_rolled_features_tensor(x, kinds=["u", "v", "w"], max_timeshift=4, **kw)
    assert got[1] == ["u__maximum", "v__length", "v__minimum"]
    _check(got, x, ["u", "v", "w"], max_timeshift=4, **kw)
    feats, cols, series, positions = tsfresh_amd.extract_rolled_features_tensor(x, kind_to_fc_parameters={"7": {"length": None}})
    assert cols == [] and tuple(feats.shape) == (len(series), 0) and len(series) == 4 * 9


def test_no_window_at_all(emulated):
    params = MinimalFCParameters()
    n_cols = len(tsfresh_amd.extract_rolled_features_tensor(_x(), default_fc_parameters=params)[1])
    for kw in (dict(min_timeshift=9), dict(max_timeshift=3, min_timeshift=4), dict(lengths=np.array([3, 1, 2, 3]), min_timeshift=3)):
        feats, cols, series, positions = tsfresh_amd.extract_rolled_features_tensor(_x(), default_fc_parameters=params, **kw)
        assert len(cols) == n_cols > 0
        assert tuple(feats.shape) == (0, n_cols) and feats.dtype == torch.float64
        assert tuple(series.shape) == (0,) and tuple(positions.shape) == (0,)
        assert series.dtype == torch.int64 and positions.dtype == torch.int64


def test_roll_argument_errors_come_first(emulated):
    params = MinimalFCParameters()
    with pytest.raises(ValueError, match="Rolling direction of 0 is not possible"):
        tsfresh_amd.extract_rolled_features_tensor(_x(), rolling_direction=0, default_fc_parameters=params)
    with pytest.raises(ValueError, match="max_timeshift needs to be positive!"):
        tsfresh_amd.extract_rolled_features_tensor(_x(), max_timeshift=0, default_fc_parameters=params)
    with pytest.raises(ValueError, match="min_timeshift needs to be positive or zero!"):
        tsfresh_amd.extract_rolled_features_tensor(_x(), min_timeshift=-1, default_fc_parameters=params)
    # before anything else is looked at
    with pytest.raises(ValueError, match="Rolling direction of 0"):
        tsfresh_amd.extract_rolled_features_tensor(np.zeros((2, 3), dtype=np.int64), rolling_direction=0)
    assert _ROUTES == []


def test_the_tensor_entrys_errors(emulated):
    params = MinimalFCParameters()
    x = _x()

    def my_feature(s):
        return 0.0
    with pytest.raises(UnsupportedFeature, match="callable"):
        tsfresh_amd.extract_rolled_features_tensor(x, default_fc_parameters={"maximum": None, my_feature: None})
    for bad in (0, -1, 10):
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 9\]"):
            tsfresh_amd.extract_rolled_features_tensor(x, lengths=np.array([9, bad, 1, 2]), default_fc_parameters=params, check_nan=False)
    with pytest.raises(TypeError, match="int64"):
        tsfresh_amd.extract_rolled_features_tensor(np.zeros((2, 3), dtype=np.int64), default_fc_parameters=params)
    with pytest.raises(ValueError, match="one entry per series"):
        tsfresh_amd.extract_rolled_features_tensor(x, lengths=np.array([9, 9, 9]), default_fc_parameters=params)
    x[2, 1, 5] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: v$"):
        tsfresh_amd.extract_rolled_features_tensor(x, kinds=["u", "v", "w"], default_fc_parameters=params)
    feats = tsfresh_amd.extract_rolled_features_tensor(x, default_fc_parameters=params, check_nan=False, max_timeshift=2)[0]
    assert torch.isnan(feats).any()
    # beyond the series' length the NaN is padding
    feats = tsfresh_amd.extract_rolled_features_tensor(x, lengths=np.array([9, 9, 5, 9]), default_fc_parameters=params)[0]
    assert not torch.isnan(feats).any()
    assert _ROUTES == ["uniform", "ragged"]   # the refused calls never reached the window builder


def test_without_a_device_the_real_call_is_an_error_not_a_cpu_route():
    if _native.device_count() > 0:
        return   # (a HIP device is present: tests/test_roll_tensor_gpu.py runs the real call)
    with pytest.raises(_native.NativeError) as ei:
        tsfresh_amd.extract_rolled_features_tensor(_x(), default_fc_parameters=MinimalFCParameters())
    assert ei.value.code == _native.TSFA_ERR_NO_DEVICE
