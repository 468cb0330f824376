"""`times=` on the tensor entries above the kernels: the plans become those of a frame with a DatetimeIndex (names, order, count),
the hours reach every kind's plan in the packed layout, the accepted forms of `times` and the refused ones, and `times=None`
makes exactly the calls it made before -- on CPU tensors, with the g++ builds of the dense packer's, the times packer's and
the window builder's bodies standing in for the device and a numpy plan that also consumes the hours standing in for the
kernels.  The reference of every case is the frame entry on the wide frame that carries the same stamps as its
DatetimeIndex, host route, under the same stand-in plan.  No GPU needed."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import emul_pack_dense_lib as epd
import emul_pack_times_lib as ept
import emul_roll_dense_lib as erd
import tsfresh_amd
from tsfresh_amd import MinimalFCParameters, _native, extract_features, extract_rolled_features, tensor
from tsfresh_amd import tensor_selection
from tsfresh_amd.feature_extraction import extraction

TIMEWISE = {"linear_trend_timewise": [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]}
NAT = np.iinfo(np.int64).min


def _at(ptr, n, ctype, dtype):
    """n elements at address `ptr` as a numpy array (the stand-in plan is handed raw pointers, like the native one)."""
    if n == 0:
        return np.empty(0, dtype=dtype)
    return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(ptr), ctypes.POINTER(ctype)), (n,))


class _NumpyPlan:
    """Column j of a series or window is (j + 1) * its sum + its length, plus -- when hours come with it -- the sum of its
    hours rebased on its first one, whichever way the samples, the windows and the hours arrive."""

    def __init__(self, n_cols):
        self.n_cols = n_cols

    def _rows(self, values, starts, ends, times):
        values = np.asarray(values, dtype=np.float64)
        base = np.array([[values[a:b].sum(), b - a] for a, b in zip(starts, ends)], dtype=np.float64).reshape(-1, 2)
        if times is not None:
            base[:, 1] += [float((times[a:b] - times[a]).sum()) for a, b in zip(starts, ends)]
        return np.stack([(j + 1) * base[:, 0] + base[:, 1] for j in range(self.n_cols)], axis=1) if len(base) \
            else np.empty((0, self.n_cols))

    def extract_host(self, values, offsets, times=None, out=None):
        return self._rows(values, offsets[:-1], offsets[1:], times)

    def extract_windows_host(self, values, starts, ends, times=None):
        return self._rows(values, starts, ends, times)

    def extract_into(self, values, offsets, matrix, col0=0, times=None, pack=None, times_ptr=None):
        assert values is None and offsets is None and times is None and isinstance(matrix, _native.BorrowedMatrix)
        hours = None if times_ptr is None else _at(times_ptr, int(pack.offsets[-1]), ctypes.c_double, np.float64)
        matrix.owner.numpy()[:, col0:col0 + self.n_cols] = self._rows(pack.values_host(), pack.offsets[:-1], pack.offsets[1:], hours)

    def extract_windows_into(self, values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=0, times_ptr=None):
        assert isinstance(matrix, _native.BorrowedMatrix) and matrix.shape[0] == n_windows > 0
        starts = _at(starts_ptr, n_windows, ctypes.c_int64, np.int64)
        ends = _at(ends_ptr, n_windows, ctypes.c_int64, np.int64)
        ctype, dtype = (ctypes.c_float, np.float32) if values_type == _native.TSFA_F32 else (ctypes.c_double, np.float64)
        values = _at(values_ptr, int(ends.max()), ctype, dtype)
        hours = None if times_ptr is None else _at(times_ptr, int(ends.max()), ctypes.c_double, np.float64)
        matrix.owner.numpy()[:, col0:col0 + self.n_cols] = self._rows(values, starts, ends, hours)


class _UntimedPlan:
    """The plan as the entries found it before `times=` existed: a keyword it does not know is a TypeError."""

    def __init__(self, n_cols):
        self._plan = _NumpyPlan(n_cols)
        self.n_cols = n_cols

    def extract_into(self, values, offsets, matrix, col0=0, times=None, pack=None):
        CALLS.append(("extract_into", values, offsets, col0, times))
        self._plan.extract_into(values, offsets, matrix, col0=col0, times=times, pack=pack)

    def extract_windows_into(self, values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=0):
        CALLS.append(("extract_windows_into", col0))
        self._plan.extract_windows_into(values_ptr, values_type, starts_ptr, ends_ptr, n_windows, matrix, col0=col0)


class _EmulChannel:
    def __init__(self, values, offsets, device):
        self._values, self.offsets, self.n_series, self.device = np.ascontiguousarray(values), offsets, len(offsets) - 1, device
        self.values_ptr = self._values.ctypes.data
        self.values_type = _native.TSFA_F32 if self._values.dtype == np.float32 else _native.TSFA_F64

    def values_host(self):
        return self._values

    def close(self):
        pass


CALLS = []


def _emul_dense_pack(torch_, x3, lengths, device):
    CALLS.append(("_dense_pack", tuple(x3.shape), None if lengths is None else lengths.tolist(), device))
    res = epd.EmulDense(x3.numpy(), lengths=None if lengths is None else lengths.numpy())
    assert res.status == 0 and res.guards_intact
    return [_EmulChannel(res.values[c], res.offsets, device) for c in range(x3.shape[1])], torch.tensor([res.flags], dtype=torch.int32)


def _emul_times_pack(torch_, times, pack, flag, device):
    t, t_type, tps = times
    CALLS.append(("_times_pack", tuple(t.shape), tuple(t.stride()), t_type, tps))
    tnp = t.numpy()
    assert tnp.strides == tuple(8 * s for s in t.stride())   # the view's own strides reach the packer
    unit = {v: k for k, v in ept.TICKS_PER_SECOND.items()}[tps]
    res = ept.EmulTimes(tnp, pack.offsets, unit=unit, flags=int(flag[0]))
    assert res.status == 0 and res.guards_intact
    flag[0] = res.flags
    return torch.from_numpy(res.hours)


def _emul_roll_windows(torch_, pack, series_len, rolling_direction, max_timeshift, min_timeshift, steps):
    scanned = np.zeros(pack.n_series, dtype=np.uint32) if series_len is None else None
    kw = dict(scanned=scanned, series_len=series_len or 0)
    rc, n = erd.count(pack.offsets, pack.n_series, rolling_direction, max_timeshift, min_timeshift, steps, **kw)
    assert rc == 0
    out = np.full((4, n + erd.GUARD), erd.SENTINEL, dtype=np.int64)
    assert erd.fill(pack.offsets, pack.n_series, n, out, rolling_direction, max_timeshift, min_timeshift, steps, **kw) == 0
    return tuple(torch.from_numpy(out[k, :n].copy()) for k in range(4))


@pytest.fixture
def emulated(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _NumpyPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_dense_pack", _emul_dense_pack)
    monkeypatch.setattr(tensor, "_times_pack", _emul_times_pack)
    monkeypatch.setattr(tensor, "_roll_windows", _emul_roll_windows)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor, "_synchronize", lambda torch_, device: None)
    del CALLS[:]


def _x(B=4, C=2, n=9, seed=0, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal((B, C, n)).astype(dtype)


def _stamps(B=4, n=9, seed=1, unit="ns"):
    """(B, n) ascending int64 ticks of `unit`, irregular steps."""
    rng = np.random.default_rng(seed)
    tps = ept.TICKS_PER_SECOND[unit]
    return 1_600_000_000 * tps + np.cumsum(rng.integers(1, 7_000 * tps + 1, size=(B, n)), axis=1)


def _wide_frame(x, kinds, stamps, lengths=None, unit="ns"):
    """The wide frame that holds the samples of x (B, C, n) and carries the stamps (B, n) as its DatetimeIndex."""
    B, C, n = x.shape
    lens = np.full(B, n) if lengths is None else np.asarray(lengths)
    cols = {"id": np.repeat(np.arange(B), lens)}
    for c, kind in enumerate(kinds):
        cols[kind] = np.concatenate([x[b, c, :lens[b]] for b in range(B)])
    flat = np.concatenate([stamps[b, :lens[b]] for b in range(B)])
    return pd.DataFrame(cols, index=pd.DatetimeIndex(flat.view("datetime64[%s]" % unit)))


def test_comprehensive_has_the_788_columns_of_the_datetime_frame(emulated):
    x, t = _x(), _stamps()
    kinds = ["b", "a"]
    want = extract_features(_wide_frame(x, kinds, t), column_id="id", pack="host")
    feats, cols = tsfresh_amd.extract_features_tensor(x, kinds=kinds, times=t)
    assert len(cols) == 2 * 788 and cols == list(want.columns)
    assert np.array_equal(feats.numpy(), want.to_numpy())
    plain, cols0 = tsfresh_amd.extract_features_tensor(x, kinds=kinds)
    assert len(cols0) == 2 * 783 and cols0 == [c for c in cols if "linear_trend_timewise" not in c]
    assert sorted(set(cols) - set(cols0)) == sorted("%s__linear_trend_timewise__attr_\"%s\"" % (k, a) for k in kinds
                                                    for a in ("pvalue", "rvalue", "intercept", "slope", "stderr"))


@pytest.mark.parametrize("lengths", (None, [9, 1, 2, 6]), ids=("dense", "ragged"))
def test_plain_entry_equals_the_frame_in_every_form_of_times(emulated, lengths):
    x, t = _x(), _stamps()
    kinds = ["u", "v"]
    params = dict(MinimalFCParameters(), **TIMEWISE)
    want = extract_features(_wide_frame(x, kinds, t, lengths), column_id="id", default_fc_parameters=params, pack="host")
    forms = {
        "int64 array": dict(times=t),
        "int64 tensor": dict(times=torch.from_numpy(t)),
        "datetime64[ns]": dict(times=t.view("datetime64[ns]"), time_unit="s"),   # (the dtype names the unit)
        "transposed view": dict(times=torch.from_numpy(np.ascontiguousarray(t.T)).T),
        "stepped view": dict(times=torch.from_numpy(np.repeat(t, 2, axis=1))[:, ::2]),
    }
    for name, kw in forms.items():
        feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=kinds, default_fc_parameters=params, **kw)
        assert cols == list(want.columns), name
        assert np.array_equal(feats.numpy(), want.to_numpy()), name
    assert [c[2] for c in CALLS if c[0] == "_times_pack"] == [(9, 1), (9, 1), (9, 1), (1, 4), (18, 2)]   # nothing was copied first
    # the other units, as ticks and as datetime64; float64 seconds
    for unit in ("us", "ms", "s"):
        tu = _stamps(unit=unit)
        want_u = extract_features(_wide_frame(x, kinds, tu, lengths, unit), column_id="id", default_fc_parameters=params, pack="host")
        for kw in (dict(times=tu, time_unit=unit), dict(times=tu.view("datetime64[%s]" % unit))):
            feats, _ = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=kinds, default_fc_parameters=params, **kw)
            assert np.array_equal(feats.numpy(), want_u.to_numpy()), unit
    ts = _stamps(unit="s")
    want_s = extract_features(_wide_frame(x, kinds, ts, lengths, "s"), column_id="id", default_fc_parameters=params, pack="host")
    feats, _ = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=kinds, default_fc_parameters=params,
                                                   times=ts.astype(np.float64))
    assert np.array_equal(feats.numpy(), want_s.to_numpy())   # (whole seconds: the float route gives the same hours)


def test_one_clock_for_the_batch(emulated):
    x, t = _x(), _stamps(B=1)[0]
    params = dict(MinimalFCParameters(), **TIMEWISE)
    want = extract_features(_wide_frame(x, ["0", "1"], np.broadcast_to(t, (4, 9))), column_id="id", default_fc_parameters=params,
                            pack="host")
    for times in (t, torch.from_numpy(t), torch.from_numpy(t).unsqueeze(0).expand(4, 9)):
        feats, cols = tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=times)
        assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())
    assert [c[2] for c in CALLS if c[0] == "_times_pack"] == [(0, 1)] * 3


def test_timewise_only_per_kind(emulated):
    x, t = _x(), _stamps()
    lengths = [9, 1, 2, 6]
    kw = dict(default_fc_parameters={"maximum": None}, kind_to_fc_parameters={"v": TIMEWISE})
    want = extract_features(_wide_frame(x, ["u", "v"], t, lengths), column_id="id", pack="host", **kw)
    feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=["u", "v"], times=t, **kw)
    assert cols == ["u__maximum"] + ["v__linear_trend_timewise__attr_\"%s\"" % a for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]
    assert cols == list(want.columns) and np.array_equal(feats.numpy(), want.to_numpy())
    # without a clock the calculator is dropped, as before
    feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=lengths, kinds=["u", "v"], **kw)
    assert cols == ["u__maximum"] and tuple(feats.shape) == (4, 1)


@pytest.mark.parametrize("roll", (dict(max_timeshift=4), dict(rolling_direction=-1, max_timeshift=4), dict(rolling_direction=2, min_timeshift=1)),
                         ids=("dir1", "dir-1", "dir2"))
@pytest.mark.parametrize("lengths", (None, [9, 1, 2, 6]), ids=("dense", "ragged"))
def test_rolled_entry_equals_the_frame(emulated, roll, lengths):
    x, t = _x(), _stamps()
    kinds = ["b", "a"]
    params = dict(MinimalFCParameters(), **TIMEWISE)
    want = extract_rolled_features(_wide_frame(x, kinds, t, lengths), column_id="id", default_fc_parameters=params, pack="host", **roll)
    feats, cols, series, positions = tsfresh_amd.extract_rolled_features_tensor(x, lengths=lengths, kinds=kinds, default_fc_parameters=params,
                                                                                times=t, **roll)
    assert cols == list(want.columns) and len(cols) == 2 * (len(MinimalFCParameters()) + 5)
    assert list(zip(series.tolist(), positions.tolist())) == list(want.index)
    assert np.array_equal(feats.numpy(), want.to_numpy())
    # and the count under the default settings
    _, cols, _, _ = tsfresh_amd.extract_rolled_features_tensor(x, lengths=lengths, kinds=kinds, times=t, **roll)
    assert len(cols) == 2 * 788


def test_relevant_entry_passes_the_clock_through(emulated, monkeypatch):
    seen = {}

    def select(features, y, columns=None, **kw):
        seen["columns"], seen["features"] = list(columns), features.clone()
        keep = [j for j, c in enumerate(columns) if "timewise" in c or c.endswith("__maximum")]
        return features[:, keep], [columns[j] for j in keep], torch.tensor(keep, dtype=torch.int32)

    monkeypatch.setattr(tensor_selection, "impute_tensor", lambda X: X)
    monkeypatch.setattr(tensor_selection, "select_features_tensor", select)
    x = _x()
    tu = _stamps(unit="us")
    y = np.array([0, 1, 0, 1])
    got, names = tsfresh_amd.extract_relevant_features_tensor(x, y, kinds=["b", "a"], times=tu, time_unit="us")
    want = extract_features(_wide_frame(x, ["b", "a"], tu, unit="us"), column_id="id", pack="host")
    assert seen["columns"] == list(want.columns) and len(seen["columns"]) == 2 * 788
    assert np.array_equal(seen["features"].numpy(), want.to_numpy())
    assert len(names) == 2 * 6 and np.array_equal(got.numpy(), want[names].to_numpy())
    tsfresh_amd.extract_relevant_features_tensor(x, y, kinds=["b", "a"])
    assert len(seen["columns"]) == 2 * 783


@pytest.mark.parametrize("bad", (np.zeros((4, 9), dtype=np.float32), np.zeros((4, 9), dtype=np.int32), np.zeros((4, 9), dtype=np.uint64),
                                 np.zeros((4, 9), dtype="datetime64[D]"), np.zeros((4, 9), dtype="datetime64[m]"),
                                 np.zeros((4, 9), dtype="timedelta64[ns]"), torch.zeros((4, 9), dtype=torch.float32),
                                 torch.zeros((4, 9), dtype=torch.int32), torch.zeros((4, 9), dtype=torch.float16)))
def test_type_errors_name_the_dtype(emulated, bad):
    import re
    for entry in (tsfresh_amd.extract_features_tensor, tsfresh_amd.extract_rolled_features_tensor):
        with pytest.raises(TypeError, match=re.escape(str(bad.dtype).replace("torch.", ""))):
            entry(_x(), default_fc_parameters=MinimalFCParameters(), times=bad)
    assert not CALLS   # refused before anything moved


def test_value_errors(emulated):
    x, t = _x(), _stamps()
    params = dict(MinimalFCParameters(), **TIMEWISE)
    with pytest.raises(TypeError, match="list"):
        tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=t.tolist())
    for bad in (t[:, :8], t[:3], t[0, :8], t[None], t.T):
        with pytest.raises(ValueError, match=r"times must have shape \(9,\).*or \(4, 9\)"):
            tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=bad)
    with pytest.raises(ValueError, match="time_unit must be one of 'ns', 'us', 'ms', 's'"):
        tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=t, time_unit="h")
    assert not CALLS
    # a bad time_unit is not looked at where the dtype names the unit, nor for seconds
    tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=t.view("datetime64[ns]"), time_unit="h")
    tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=t / 1e9, time_unit="h")


def test_nat_raises_under_check_nan_and_passes_without(emulated):
    x, t = _x(), _stamps()
    params = dict(MinimalFCParameters(), **TIMEWISE)
    lengths = [9, 4, 9, 9]
    clean, cols = tsfresh_amd.extract_features_tensor(x, lengths=lengths, default_fc_parameters=params, times=t)
    bad = t.copy()
    bad[1, 6] = NAT   # beyond the series' length: padding
    feats, _ = tsfresh_amd.extract_features_tensor(x, lengths=lengths, default_fc_parameters=params, times=bad)
    assert torch.equal(feats, clean)
    bad[2, 3] = NAT
    for kw in (dict(times=bad), dict(times=bad.view("datetime64[ns]")), dict(times=np.where(bad == NAT, np.nan, bad / 1e9))):
        with pytest.raises(ValueError, match="times must not contain NaT / NaN"):
            tsfresh_amd.extract_features_tensor(x, lengths=lengths, default_fc_parameters=params, **kw)
        with pytest.raises(ValueError, match="times must not contain NaT / NaN"):
            tsfresh_amd.extract_rolled_features_tensor(x, lengths=lengths, default_fc_parameters=params, max_timeshift=3, **kw)
    feats, _ = tsfresh_amd.extract_features_tensor(x, lengths=lengths, default_fc_parameters=params, times=bad, check_nan=False)
    nan_rows = torch.isnan(feats).any(dim=1).tolist()
    assert nan_rows == [False, False, True, False]
    # a NaN sample is still the first thing reported
    xn = x.copy()
    xn[0, 1, 0] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: 1$"):
        tsfresh_amd.extract_features_tensor(xn, lengths=lengths, default_fc_parameters=params, times=bad)


def test_without_times_the_calls_are_the_ones_made_before(monkeypatch):
    """The names the earlier route tests stub keep their fixed signatures: `_dense_pack(torch, x3, lengths, device)`, a plan
    whose `extract_into` / `extract_windows_into` know no `times_ptr`, and no call of the times packer."""
    def no_times_pack(*a, **k):
        raise AssertionError("the times packer was called without times")

    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _UntimedPlan(len(fplan.names)))
    monkeypatch.setattr(tensor, "_dense_pack", _emul_dense_pack)
    monkeypatch.setattr(tensor, "_times_pack", no_times_pack)
    monkeypatch.setattr(tensor, "_roll_windows", _emul_roll_windows)
    monkeypatch.setattr(tensor, "_to_device", lambda t, device: t)
    monkeypatch.setattr(tensor, "_synchronize", lambda torch_, device: None)
    del CALLS[:]
    x = _x()
    params = dict(MinimalFCParameters(), **TIMEWISE)
    feats, cols = tsfresh_amd.extract_features_tensor(x, lengths=[9, 1, 2, 6], kinds=["u", "v"], default_fc_parameters=params, device=0)
    n = len(MinimalFCParameters())
    assert len(cols) == 2 * n and not any("timewise" in c for c in cols)
    assert CALLS == [("_dense_pack", (4, 2, 9), [9, 1, 2, 6], 0), ("extract_into", None, None, 0, None), ("extract_into", None, None, n, None)]
    del CALLS[:]
    _, cols, _, _ = tsfresh_amd.extract_rolled_features_tensor(x, kinds=["u", "v"], default_fc_parameters=params, max_timeshift=3, device=0)
    assert len(cols) == 2 * n
    assert CALLS == [("_dense_pack", (4, 2, 9), None, 0), ("extract_windows_into", 0), ("extract_windows_into", n)]
    # with times the same stand-in is refused: the keyword is what carries the hours
    monkeypatch.setattr(tensor, "_times_pack", _emul_times_pack)
    with pytest.raises(TypeError, match="times_ptr"):
        tsfresh_amd.extract_features_tensor(x, default_fc_parameters=params, times=_stamps())


def test_signatures_end_with_times_and_time_unit():
    import inspect
    for entry in (tensor.extract_features_tensor, tensor.extract_rolled_features_tensor, tensor_selection.extract_relevant_features_tensor):
        names = list(inspect.signature(entry).parameters)
        assert names[-2:] == ["times", "time_unit"]
        assert inspect.signature(entry).parameters["times"].default is None
        assert inspect.signature(entry).parameters["time_unit"].default == "ns"
