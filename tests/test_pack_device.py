"""The device packer on the GPU: exact equality with data._pack's host route, end-to-end equality of extract_features
across pack="device" / pack="host", the pack="auto" rule, the NaN message, and that destroying a pack frees its memory."""
import numpy as np
import pandas as pd
import pytest

import conftest
import pack_cases
from tsfresh_amd import EfficientFCParameters, MinimalFCParameters, _native, extract_features, extract_relevant_features
from tsfresh_amd.feature_extraction import data

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", pack_cases.SIZES)
@pytest.mark.parametrize("name", sorted(pack_cases.CASES))
def test_device_pack_equals_host_route(gpu, name, n, monkeypatch):
    ids, sort, values = pack_cases.make_case(name, n)
    pack = pack_cases.assert_equals_host(_native.DevicePack, ids, sort, values, monkeypatch)
    assert not pack.value_nan
    if name == "in_order":
        assert pack.was_in_order and pack.n_passes == 0
    if np.asarray(ids).dtype.kind in "iu" and (sort is None or sort.dtype.kind in "iu") and not pack.was_in_order:
        assert pack.n_passes == pack_cases.expected_passes(ids, sort)


def test_device_pack_of_2_24_rows_in_time_order(gpu, monkeypatch):
    n_ids, length = 1 << 14, 1 << 10
    rng = np.random.default_rng(5)
    ids = np.tile(np.arange(n_ids, dtype=np.int64), length)          # one row per (timestamp, id), ordered by time
    sort = np.repeat(np.arange(length, dtype=np.int64), n_ids)
    values = rng.standard_normal(n_ids * length).astype(np.float32)
    pack = pack_cases.assert_equals_host(_native.DevicePack, ids, sort, values, monkeypatch)
    assert pack.n_series == n_ids and pack.n_passes == 4             # two bytes of the id, two of the stamp


def _ragged_frame(value_dtype, n_ids=2000, seed=11):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(100, 1501, n_ids)
    ids = np.repeat(np.arange(n_ids, dtype=np.int64) * 3 - 100, lengths)
    t = np.concatenate([np.arange(k, dtype=np.int64) for k in lengths])
    x = rng.standard_normal(len(ids))
    if np.dtype(value_dtype).kind == "i":
        v = np.round(x * 1000).astype(value_dtype)
    else:
        v = x.astype(value_dtype)
    return pd.DataFrame({"id": ids, "t": t, "v": v})


def _time_ordered(df, rng=None):
    if rng is not None:
        return df.iloc[rng.permutation(len(df))].reset_index(drop=True)
    return df.sort_values(["t", "id"], kind="stable").reset_index(drop=True)


def _assert_same(got, want):
    assert not (got.to_numpy() == conftest.SENTINEL).any(), "cells no kernel wrote"
    pd.testing.assert_frame_equal(got, want, check_exact=True)


@pytest.mark.parametrize("value_dtype", [np.float32, np.int16])
@pytest.mark.parametrize("layout", ["time", "shuffled"])
def test_extract_features_does_not_depend_on_the_pack_route(gpu, value_dtype, layout):
    df = _ragged_frame(value_dtype)
    other = _time_ordered(df, np.random.default_rng(1) if layout == "shuffled" else None)
    want = extract_features(df, column_id="id", column_sort="t", default_fc_parameters=EfficientFCParameters(), pack="host")
    got = extract_features(other, column_id="id", column_sort="t", default_fc_parameters=EfficientFCParameters(),
                           pack="device")
    _assert_same(got, want)
    same_rows_host = extract_features(other, column_id="id", column_sort="t", default_fc_parameters=EfficientFCParameters(),
                                      pack="host")
    _assert_same(got, same_rows_host)


def test_wide_long_and_dict_formats(gpu):
    base = _ragged_frame(np.float32, n_ids=300)
    base["w"] = np.round(base["v"] * 100).astype(np.int32)
    params = MinimalFCParameters()
    wide_t = _time_ordered(base)
    _assert_same(extract_features(wide_t, column_id="id", column_sort="t", default_fc_parameters=params, pack="device"),
                 extract_features(base, column_id="id", column_sort="t", default_fc_parameters=params, pack="host"))
    long_ = pd.concat([base[["id", "t"]].assign(kind="a", value=base["v"].astype(np.float64)),
                       base[["id", "t"]].assign(kind="b", value=base["w"].astype(np.float64))], ignore_index=True)
    long_t = _time_ordered(long_)
    kw = dict(column_id="id", column_sort="t", column_kind="kind", column_value="value", default_fc_parameters=params)
    _assert_same(extract_features(long_t, pack="device", **kw), extract_features(long_, pack="host", **kw))
    frames = {"a": base[["id", "t", "v"]].rename(columns={"v": "value"}),
              "b": base[["id", "t", "w"]].rename(columns={"w": "value"})}
    frames_t = {k: _time_ordered(f) for k, f in frames.items()}
    kw = dict(column_id="id", column_sort="t", column_value="value", default_fc_parameters=params)
    _assert_same(extract_features(frames_t, pack="device", **kw), extract_features(frames, pack="host", **kw))


def test_composite_plan_and_device_resident_chain(gpu):
    df = _ragged_frame(np.float32, n_ids=400)
    other = _time_ordered(df)
    # two autolag values of augmented_dickey_fuller: one native plan cannot hold them together (a composite plan)
    params = {"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"},
                                                        {"attr": "teststat", "autolag": "BIC"}]}
    _assert_same(extract_features(other, column_id="id", column_sort="t", default_fc_parameters=params, pack="device"),
                 extract_features(df, column_id="id", column_sort="t", default_fc_parameters=params, pack="host"))
    ids = np.unique(df["id"].to_numpy())
    means = df.groupby("id")["v"].std().reindex(ids).to_numpy()
    y = pd.Series((means > np.median(means)).astype(int), index=ids)
    kw = dict(column_id="id", column_sort="t", default_fc_parameters=MinimalFCParameters(), device_resident=True)
    got = extract_relevant_features(other, y, pack="device", **kw)
    want = extract_relevant_features(df, y, pack="host", **kw)
    assert got.shape[1] > 0
    _assert_same(got, want)


def test_pack_auto_takes_the_device_for_large_unsorted_frames_only(gpu, monkeypatch):
    made = []
    real = _native.DevicePack

    class Spy(real):
        def __init__(self, *a, **k):
            made.append(len(a[0][0]))
            super().__init__(*a, **k)

    monkeypatch.setattr(_native, "DevicePack", Spy)
    rows = data._DEVICE_PACK_MIN_ROWS
    length = 256
    n_ids = rows // length
    rng = np.random.default_rng(2)
    df = pd.DataFrame({"id": np.repeat(np.arange(n_ids), length), "t": np.tile(np.arange(length), n_ids),
                       "v": rng.standard_normal(rows).astype(np.float32)})
    kw = dict(column_id="id", column_sort="t", default_fc_parameters=MinimalFCParameters())
    want = extract_features(df, **kw)                       # id-ordered: the presorted proof, no device pack
    assert made == []
    got = extract_features(_time_ordered(df), **kw)         # unsorted, at the threshold: the device
    assert made == [rows]
    _assert_same(got, want)
    small = df[df["id"] < n_ids // 2]
    extract_features(_time_ordered(small), **kw)            # unsorted but smaller: the host
    assert made == [rows]


def test_nan_raises_the_reference_message_on_both_routes(gpu):
    df = _time_ordered(_ragged_frame(np.float32, n_ids=50))
    df.loc[1234, "v"] = np.nan
    for mode in ("host", "device"):
        with pytest.raises(ValueError, match="Column must not contain NaN values: v"):
            extract_features(df, column_id="id", column_sort="t", default_fc_parameters=MinimalFCParameters(), pack=mode)


_FREE_MEMORY_SCRIPT = r"""
import sys
import numpy as np
import torch   # first: torch ships its own HIP runtime and must be the one that opens the device in this process
torch.cuda.init()
sys.path.insert(0, %(root)r)
from tsfresh_amd import _native
n = 1 << 22
rng = np.random.default_rng(9)
ids = _native.pack_column(rng.integers(0, 4096, n))
sort = _native.pack_column(rng.integers(0, 1 << 20, n))
values = _native.pack_column(rng.standard_normal(n).astype(np.float32))
free = []
for _ in range(20):
    pack = _native.DevicePack(ids, sort, values, keep_sort=True)
    assert pack.n_series == 4096 and pack.n_passes == 5, (pack.n_series, pack.n_passes)
    pack.close()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info()[0])
print("FREE", free[1], free[19])
assert free[19] == free[1], free
print("PACK_MEMORY_OK")
"""


def test_destroying_a_pack_frees_its_device_memory(gpu):
    """20 packs of 2^22 rows, each destroyed: the free device memory after the 20th equals that after the 2nd (a fresh child
    process, torch imported first so that torch.cuda.mem_get_info and the library see one HIP runtime)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _FREE_MEMORY_SCRIPT % {"root": root}], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "PACK_MEMORY_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
