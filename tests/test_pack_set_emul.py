"""The pack set's kernel bodies (csrc/pack_device.h), emulated with one thread per workgroup (tests/emul/emul_pack_set.cpp),
against data._pack's host route on every kind's rows.  Equality is exact: a packer moves and converts."""
import numpy as np
import pandas as pd
import pytest

import emul_pack_lib
import emul_pack_set_lib
import pack_cases
import pack_set_cases
from tsfresh_amd import _native
from tsfresh_amd.feature_extraction import data

EmulPackSet = emul_pack_set_lib.EmulPackSet


def test_tile_size_matches_the_cases():
    assert emul_pack_set_lib.tile() == pack_set_cases.TILE


@pytest.mark.parametrize("n", pack_set_cases.SIZES)
@pytest.mark.parametrize("name", sorted(pack_set_cases.CASES))
def test_emulated_set_equals_host_route_per_kind(name, n, monkeypatch):
    ids, sort, kinds, values = pack_set_cases.make_case(name, n)
    pack_set, packs = pack_set_cases.assert_set_equals_host(EmulPackSet, ids, sort, kinds, values, monkeypatch)
    if n > 1 and name == "interleaved":
        # rows in (id, sort) order: ONLY the kind passes run (3 kinds: one byte), and the frame is not "in order"
        assert pack_set.n_passes == 1 and not pack_set.was_in_order
    if name == "kind_major":
        assert pack_set.n_passes == 0 and pack_set.was_in_order
    if n > 1 and name == "edge_ids":
        assert packs[0].ids.tolist() == [3, 5, 9] and packs[1].ids.tolist() == [9, 12]
        if n >= 3:
            assert packs[2].ids.tolist() == [12] and packs[2].n_rows == 1


@pytest.mark.parametrize("where", sorted(pack_set_cases.BOUNDARIES))
def test_kind_boundary_against_the_tile_grid(where, monkeypatch):
    rows = pack_set_cases.BOUNDARIES[where]
    ids, sort, kinds, values = pack_set_cases.make_boundary_case(rows)
    _, packs = pack_set_cases.assert_set_equals_host(EmulPackSet, ids, sort, kinds, values, monkeypatch)
    assert packs[0].n_rows == rows and packs[1].n_rows == len(ids) - rows


@pytest.mark.parametrize("layout", ["time_major", "random", "in_order"])
def test_constant_kind_column_adds_no_pass_and_equals_the_single_packer(layout):
    ids, sort, values = pack_cases.make_case(layout, 2 * pack_set_cases.TILE + 1)
    kinds = np.full(len(ids), -7, dtype=np.int64)
    pack_set_cases.assert_set_equals_single_packer(EmulPackSet, emul_pack_lib.EmulPack, ids, sort, kinds, [values])


@pytest.mark.parametrize("n_kinds,kind_passes", [(256, 1), (257, 2)])
def test_dense_kinds_cost_one_pass_per_byte(n_kinds, kind_passes, monkeypatch):
    ids, sort, kinds, values = pack_set_cases.dense_kinds_in_id_sort_order(n_kinds)
    pack_set, _ = pack_set_cases.assert_set_equals_host(EmulPackSet, ids, sort, kinds, values, monkeypatch)
    assert pack_set.n_passes == kind_passes and not pack_set.was_in_order   # (id, sort) order: the kind passes alone
    order = np.random.default_rng(n_kinds).permutation(len(ids))
    ids, sort, kinds = ids[order], sort[order], kinds[order]
    pack_set, _ = pack_set_cases.assert_set_equals_host(EmulPackSet, ids, sort, kinds, values, monkeypatch)
    assert pack_set.n_passes == pack_cases.expected_passes(ids, sort) + kind_passes


def test_five_interleaved_kinds_on_ragged_ids(monkeypatch):
    ids, sort, kinds, values = pack_set_cases.five_kinds_on_ragged_ids()
    pack_set_cases.assert_set_equals_host(EmulPackSet, ids, sort, kinds, values, monkeypatch)


@pytest.mark.parametrize("n", (pack_set_cases.TILE - 1, 2 * pack_set_cases.TILE + 1))
def test_wide_columns_through_one_set_equal_the_single_packer(n):
    ids, sort, columns = pack_set_cases.wide_columns(n)
    assert [c.dtype.name for c in columns] == ["float32", "int64", "bool"] and int(np.abs(columns[1]).min()) > 2 ** 53
    pack_set_cases.assert_set_equals_single_packer(EmulPackSet, emul_pack_lib.EmulPack, ids, sort, None, columns)


def test_nan_value_sets_the_flag_on_every_view():
    ids, sort, kinds, values = pack_set_cases.make_case("random", 5000)
    id_col, _, sort_col, val_col = data._device_pack_columns(ids, values, sort)[1]
    with EmulPackSet(id_col, sort_col, _native.pack_column(kinds)) as pack_set:
        assert not any(p.value_nan for p in pack_set.values(val_col))
        bad = values.copy()
        bad[4321] = np.nan
        assert all(p.value_nan for p in pack_set.values(_native.pack_column(bad)))


def _long_frame(n_ids=60, seed=4):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(3, 40, n_ids)
    ids = np.repeat(np.arange(n_ids, dtype=np.int64) * 2 + 1, lengths)
    t = np.concatenate([np.arange(k, dtype=np.int64) for k in lengths])
    parts = []
    for kind in ("acc", "gyro", "temp"):
        keep = ids % 5 != 1 if kind == "gyro" else np.ones(len(ids), dtype=bool)   # one kind misses some ids
        parts.append(pd.DataFrame({"id": ids[keep], "t": t[keep], "kind": kind, "value": rng.standard_normal(int(keep.sum()))}))
    return pd.concat(parts, ignore_index=True).sort_values(["id", "t"], kind="stable").reset_index(drop=True)


def _assert_same_packing(got, want):
    assert [pk.kind for pk in got] == [pk.kind for pk in want]
    for g, w in zip(got, want):
        assert np.asarray(g.ids).dtype == np.asarray(w.ids).dtype and np.array_equal(g.ids, w.ids)
        assert np.array_equal(g.offsets, w.offsets) and g.n_series == w.n_series
        assert g.values.dtype == w.values.dtype
        assert np.array_equal(pack_cases._bits(np.asarray(g.values)), pack_cases._bits(np.asarray(w.values)))


class _Count:
    def __init__(self, cls, made):
        self.cls, self.made = cls, made

    def __call__(self, *a, **k):
        self.made.append(len(a[0][0]))
        return self.cls(*a, **k)


def test_pack_timeseries_routes_a_long_frame_through_one_set(monkeypatch):
    df = _long_frame()
    kw = dict(column_id="id", column_kind="kind", column_value="value", column_sort="t")
    want = data.pack_timeseries(df, pack="host", **kw)[0]
    sets, packs = [], []
    monkeypatch.setattr(_native, "DevicePackSet", _Count(EmulPackSet, sets))
    monkeypatch.setattr(_native, "DevicePack", _Count(emul_pack_lib.EmulPack, packs))
    got = data.pack_timeseries(df, pack="device", **kw)[0]
    assert sets == [len(df)] and packs == []            # ONE sort of the whole frame, no per-kind pack
    assert all(pk.device_pack is not None for pk in got)
    _assert_same_packing(got, want)
    assert len(got[1].ids) < len(got[0].ids)            # "gyro" misses ids
    # string ids are factorized once for the whole frame; every kind gets its own labels back
    df_s = df.assign(id=["s%03d" % v for v in df["id"]])
    _assert_same_packing(data.pack_timeseries(df_s, pack="device", **kw)[0], data.pack_timeseries(df_s, pack="host", **kw)[0])
    # kinds in blocks: today's per-kind route (here every block is in packed order: the presorted proof, no device at all)
    sets.clear()
    blocks = df.sort_values(["kind", "id", "t"], kind="stable").reset_index(drop=True)
    _assert_same_packing(data.pack_timeseries(blocks, pack="device", **kw)[0], want)
    assert sets == [] and packs == []
    # "auto" below the threshold: the host; at the threshold (and with a device in sight): the set
    monkeypatch.setattr(_native, "device_count", lambda: 1)
    assert all(pk.device_pack is None for pk in data.pack_timeseries(df, pack="auto", **kw)[0])
    monkeypatch.setattr(data, "_DEVICE_PACK_MIN_ROWS", len(df))
    _assert_same_packing(data.pack_timeseries(df, pack="auto", **kw)[0], want)
    assert sets == [len(df)] and packs == []


def test_pack_timeseries_routes_a_wide_frame_through_one_set(monkeypatch):
    rng = np.random.default_rng(8)
    base = _long_frame()
    base = base[base["kind"] == "acc"].drop(columns="kind").rename(columns={"value": "a"})
    base["b"] = rng.integers(-2 ** 40, 2 ** 40, len(base))
    base["c"] = rng.random(len(base)) < 0.5
    base["a"] = base["a"].astype(np.float32)
    df = base.sort_values(["t", "id"], kind="stable").reset_index(drop=True)   # time order: not packed
    kw = dict(column_id="id", column_sort="t")
    want = data.pack_timeseries(df, pack="host", **kw)[0]
    sets, packs = [], []
    monkeypatch.setattr(_native, "DevicePackSet", _Count(EmulPackSet, sets))
    monkeypatch.setattr(_native, "DevicePack", _Count(emul_pack_lib.EmulPack, packs))
    got = data.pack_timeseries(df, pack="device", **kw)[0]
    assert sets == [len(df)] and packs == []
    _assert_same_packing(got, want)
    # one value column: exactly today's call
    sets.clear()
    one = data.pack_timeseries(df[["id", "t", "a"]], pack="device", **kw)[0]
    assert sets == [] and packs == [len(df)]
    _assert_same_packing(one, want[:1])
    # rows in packed order: no device at all
    packs.clear()
    _assert_same_packing(data.pack_timeseries(base, pack="device", **kw)[0], want)
    assert sets == [] and packs == []
    # a float16 column: "device" refuses as before, "auto" packs it on the host and the others through the set
    half = df.assign(h=df["a"].astype(np.float16))
    with pytest.raises(ValueError, match="pack='device': kind 'h' cannot be packed on the device"):
        data.pack_timeseries(half, pack="device", **kw)
    monkeypatch.setattr(_native, "device_count", lambda: 1)
    monkeypatch.setattr(data, "_DEVICE_PACK_MIN_ROWS", len(df))
    sets.clear()
    packs.clear()
    mixed = data.pack_timeseries(half, pack="auto", **kw)[0]
    assert sets == [len(df)] and packs == []
    assert [pk.device_pack is not None for pk in mixed] == [True, True, True, False]
    _assert_same_packing(mixed, data.pack_timeseries(half, pack="host", **kw)[0])
    # the NaN message of the host route
    bad = df.copy()
    bad.loc[17, "a"] = np.nan
    for mode in ("host", "device"):
        with pytest.raises(ValueError, match="Column must not contain NaN values: a"):
            data.pack_timeseries(bad, pack=mode, **kw)


def test_a_failed_device_allocation_falls_back_to_the_host_with_one_warning(monkeypatch):
    df = _long_frame()
    kw = dict(column_id="id", column_kind="kind", column_value="value", column_sort="t")
    want = data.pack_timeseries(df, pack="host", **kw)[0]

    def refuse(*a, **k):
        raise _native.NativeError(_native.TSFA_ERR_HIP, "cannot allocate")

    monkeypatch.setattr(_native, "DevicePackSet", refuse)
    monkeypatch.setattr(_native, "DevicePack", refuse)
    monkeypatch.setattr(_native, "device_count", lambda: 1)
    monkeypatch.setattr(data, "_DEVICE_PACK_MIN_ROWS", 1)
    with pytest.warns(RuntimeWarning) as caught:
        got = data.pack_timeseries(df, pack="auto", **kw)[0]
    assert len(caught) == 1
    _assert_same_packing(got, want)
    with pytest.raises(_native.NativeError):
        data.pack_timeseries(df, pack="device", **kw)
