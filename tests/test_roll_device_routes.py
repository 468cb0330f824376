"""Which route `extract_rolled_features(pack=...)` takes, what it refuses, and -- with the g++ builds of the packer's and the
window builder's kernel bodies standing in for the device and a numpy plan standing in for the kernels -- that the device
route names and orders its windows exactly as the host route does.  No GPU needed."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

import emul_pack_lib
import emul_pack_set_lib
import emul_roll_lib
from tsfresh_amd import MinimalFCParameters, _native, extract_rolled_features
from tsfresh_amd.feature_extraction import data, extraction


def _frame(lengths=(14, 9, 20, 3), seed=3, ids=None):
    rng = np.random.default_rng(seed)
    rows = [pd.DataFrame({"id": sid if ids is None else ids[sid], "t": np.arange(L) * 10 + 5, "v": rng.standard_normal(L)})
            for sid, L in enumerate(lengths)]
    return pd.concat(rows, ignore_index=True)


def _time_order(df):
    return df.sort_values(["t", "id"], kind="stable").reset_index(drop=True)


class _NumpyPlan:
    """A plan whose columns are (j + 1) * sum of the window + its length: enough to tell every window from every other."""

    def __init__(self, n_cols):
        self.n_cols = n_cols

    def _rows(self, values, starts, ends):
        values = np.asarray(values, dtype=np.float64)
        base = np.array([[values[a:b].sum(), b - a] for a, b in zip(starts, ends)], dtype=np.float64).reshape(-1, 2)
        return np.stack([(j + 1) * base[:, 0] + base[:, 1] for j in range(self.n_cols)], axis=1) if len(base) \
            else np.empty((0, self.n_cols))

    def extract_windows_host(self, values, starts, ends, times=None):
        return self._rows(values, starts, ends)

    def extract_windows_pack(self, pack, windows):
        return self._rows(pack.values_host(), windows.starts, windows.ends)


@pytest.fixture
def numpy_plan(monkeypatch):
    monkeypatch.setattr(extraction, "_acquire_plan", lambda fplan, device, pins=None: _NumpyPlan(len(fplan.names)))


@pytest.fixture
def emulated_device(monkeypatch, numpy_plan):
    monkeypatch.setattr(_native, "DevicePack", emul_pack_lib.EmulPack)
    monkeypatch.setattr(_native, "DevicePackSet", emul_pack_set_lib.EmulPackSet)
    monkeypatch.setattr(_native, "DeviceWindows", emul_roll_lib.EmulWindows)


def _both(container, **kw):
    kw.setdefault("default_fc_parameters", MinimalFCParameters())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = extract_rolled_features(container, pack="host", **kw)
        got = extract_rolled_features(container, pack="device", **kw)
    assert list(got.index) == list(want.index) and list(got.columns) == list(want.columns)
    assert [type(i[1]) for i in got.index] == [type(i[1]) for i in want.index]
    assert np.array_equal(got.to_numpy(), want.to_numpy(), equal_nan=True)
    return got


def test_unknown_pack_mode():
    with pytest.raises(ValueError, match="pack must be one of"):
        extract_rolled_features(_frame(), column_id="id", column_sort="t", pack="gpu")


@pytest.mark.parametrize("in_packed_order", (False, True))
def test_device_route_names_why_a_frame_is_refused(in_packed_order):
    """The packer's reasons, for a frame in packed order too: pack="device" uploads such a frame, so it has to be eligible."""
    base = _frame() if in_packed_order else _time_order(_frame())
    df = base.copy()
    df.index = pd.date_range("2020-01-01", periods=len(df), freq="s")
    with pytest.raises(ValueError, match="pack='device'.*DatetimeIndex"):
        extract_rolled_features(df, column_id="id", column_sort="t", pack="device", default_fc_parameters=MinimalFCParameters())
    df = base.copy()
    df["id"] = df["id"].astype(np.float64)
    with pytest.raises(ValueError, match="pack='device'.*id column"):
        extract_rolled_features(df, column_id="id", column_sort="t", pack="device", default_fc_parameters=MinimalFCParameters())


def test_host_and_small_auto_never_touch_the_device(monkeypatch, numpy_plan):
    class Spy:
        def __init__(self, *a, **k):
            raise AssertionError("the device packer must not be used")

    for name in ("DevicePack", "DevicePackSet", "DeviceWindows"):
        monkeypatch.setattr(_native, name, Spy)
    df = _time_order(_frame())
    assert len(df) < data._DEVICE_PACK_MIN_ROWS
    params = MinimalFCParameters()
    a = extract_rolled_features(df, column_id="id", column_sort="t", pack="host", default_fc_parameters=params, max_timeshift=5)
    b = extract_rolled_features(df, column_id="id", column_sort="t", default_fc_parameters=params, max_timeshift=5)   # "auto"
    assert len(a) and a.equals(b)
    with pytest.raises(AssertionError, match="must not be used"):
        extract_rolled_features(df, column_id="id", column_sort="t", pack="device", default_fc_parameters=params)


def test_roll_windows_without_a_device_is_an_error_not_a_cpu_route():
    lib = _native.load()
    handle = ctypes.c_void_p()
    rc = lib.tsfa_roll_windows(None, 1, 0, 0, 5, ctypes.byref(handle))
    assert not handle.value
    if _native.device_count() > 0:
        assert rc == _native.TSFA_ERR_INVALID   # (a NULL pack)
        return
    assert rc == _native.TSFA_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.tsfa_last_error()


@pytest.mark.parametrize("kw", [dict(), dict(max_timeshift=6, min_timeshift=2), dict(rolling_direction=-2, max_timeshift=4),
                                dict(rolling_direction=3, min_timeshift=1), dict(max_timeshift=3, min_timeshift=5)])
def test_device_route_equals_host_route_emulated(emulated_device, kw):
    df = _time_order(_frame())
    got = _both(df, column_id="id", column_sort="t", **kw)
    assert (len(got) == 0) == (kw.get("min_timeshift", 0) > kw.get("max_timeshift", 99))
    _both(_frame(), column_id="id", column_sort="t", **kw)              # in packed order: uploaded, same result
    _both(df.drop(columns="t"), column_id="id", **kw)                   # no sort column: the shift value is ts - 1


def test_device_route_window_ids_emulated(emulated_device):
    # string ids keep the ordering step; Timestamps name the windows of a datetime sort column; duplicate stamps inside a
    # series give duplicate window ids whose order must be the host route's
    df = _time_order(_frame(ids=["s10", "s9", "b", "a"]))
    _both(df, column_id="id", column_sort="t", max_timeshift=4)
    stamped = _time_order(_frame())
    stamped["t"] = pd.Timestamp("2021-03-01") + pd.to_timedelta(stamped["t"], unit="h")
    got = _both(stamped, column_id="id", column_sort="t", rolling_direction=-1, max_timeshift=4)
    assert isinstance(got.index[0][1], pd.Timestamp)
    dup = _time_order(_frame())
    dup["t"] = dup["t"] // 20
    got = _both(dup, column_id="id", column_sort="t", max_timeshift=4)
    assert got.index.duplicated().any()
    for dtype in (np.int32, np.float32, np.float64):
        typed = _time_order(_frame())
        typed["t"] = typed["t"].astype(dtype)
        _both(typed, column_id="id", column_sort="t", max_timeshift=4, rolling_direction=2)


def test_device_route_several_kinds_emulated(emulated_device):
    """`steps` is the longest series over all kinds of a frame (kind b owns it here), and per entry for a dict."""
    rng = np.random.default_rng(8)
    rows = []
    for kind, lens in (("a", [31, 20]), ("b", [47, 40])):
        for sid, L in enumerate(lens):
            rows.append(pd.DataFrame({"id": sid, "t": np.arange(L), "kind": kind, "v": rng.standard_normal(L)}))
    long = pd.concat(rows, ignore_index=True)
    kw = dict(rolling_direction=3, max_timeshift=12, min_timeshift=2)
    a = _both(_time_order(long), column_id="id", column_sort="t", column_kind="kind", column_value="v", **kw)
    frames = {k: long[long["kind"] == k].drop(columns="kind").sample(frac=1.0, random_state=1) for k in ("a", "b")}
    b = _both(frames, column_id="id", column_sort="t", column_value="v", **kw)
    assert list(a.index) != list(b.index)   # 31 and 47 are not congruent modulo 3
    wide = _frame()
    wide["w"] = np.cumsum(wide["v"])
    _both(_time_order(wide), column_id="id", column_sort="t", max_timeshift=5)
