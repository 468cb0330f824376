"""Which frames reach the device packer, and what happens without a device -- no GPU needed."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import data
from tsfresh_amd.feature_extraction.data import pack_timeseries


def _unsorted_frame(n_ids=20, length=30):
    rng = np.random.default_rng(3)
    df = pd.DataFrame({"id": np.repeat(np.arange(n_ids), length), "t": np.tile(np.arange(length), n_ids),
                       "v": rng.standard_normal(n_ids * length).astype(np.float32)})
    return df.sort_values(["t", "id"], kind="stable").reset_index(drop=True)


def test_pack_device_without_a_device_is_an_error_not_a_cpu_route():
    ids = np.array([2, 1, 2, 1], dtype=np.int64)
    values = np.arange(4, dtype=np.float32)
    if _native.device_count() > 0:
        pack = _native.DevicePack(_native.pack_column(ids), None, _native.pack_column(values))
        assert pack.n_series == 2 and list(pack.ids) == [1, 2]
        pack.close()
        return
    lib = _native.load()
    handle = ctypes.c_void_p()
    rc = lib.tsfa_pack_device(ids.ctypes.data, _native.TSFA_I64, None, 0, values.ctypes.data, _native.TSFA_F32, 4,
                              _native.TSFA_HOST, 0, 0, ctypes.byref(handle))
    assert rc == _native.TSFA_ERR_NO_DEVICE and not handle.value
    assert b"no CPU fallback" in lib.tsfa_last_error()
    with pytest.raises(_native.NativeError) as ei:
        _native.DevicePack(_native.pack_column(ids), None, _native.pack_column(values))
    assert ei.value.code == _native.TSFA_ERR_NO_DEVICE


@pytest.mark.parametrize("column, dtype, word", [("id", np.float64, "id column"), ("v", np.float16, "value column"),
                                                  ("t", object, "sort column")])
def test_pack_device_names_why_a_frame_is_not_eligible(column, dtype, word):
    df = _unsorted_frame()
    df[column] = df[column].astype(dtype)
    with pytest.raises(ValueError, match="pack='device'.*" + word):
        pack_timeseries(df, column_id="id", column_sort="t", pack="device")


def test_pack_device_refuses_a_datetime_index():
    df = _unsorted_frame()
    df.index = pd.date_range("2020-01-01", periods=len(df), freq="s")
    with pytest.raises(ValueError, match="pack='device'.*DatetimeIndex"):
        pack_timeseries(df, column_id="id", column_sort="t", pack="device")


def test_unknown_pack_mode():
    with pytest.raises(ValueError, match="pack must be one of"):
        pack_timeseries(_unsorted_frame(), column_id="id", column_sort="t", pack="gpu")


def test_pack_host_and_small_auto_never_touch_the_device_pack(monkeypatch):
    class Spy:
        calls = 0

        def __init__(self, *a, **k):
            Spy.calls += 1
            raise AssertionError("the device packer must not be used")

    monkeypatch.setattr(_native, "DevicePack", Spy)
    df = _unsorted_frame()
    want = df.sort_values(["id", "t"], kind="stable")
    for mode in ("host", "auto"):   # (auto: the frame is far below _DEVICE_PACK_MIN_ROWS)
        packed, _, _ = pack_timeseries(df, column_id="id", column_sort="t", pack=mode)
        assert packed[0].device_pack is None
        assert np.array_equal(packed[0].values, want["v"].to_numpy())
    packed, _, _ = pack_timeseries(df, column_id="id", column_sort="t")   # the default of the packer itself is the host
    assert packed[0].device_pack is None
    assert Spy.calls == 0
    assert len(df) < data._DEVICE_PACK_MIN_ROWS
