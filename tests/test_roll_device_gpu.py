"""`extract_rolled_features(pack="device")` -- device packer, windows built by tsfa_roll_windows, kernels on the device
buffers -- against `pack="host"` on the GPU: the same index, the same columns, bit-equal values with NaNs in the same cells
(both routes run the same kernels on the same windows in the same order).  And the C-ABI pieces on their own:
`DeviceWindows` against `roll_views`, `tsfa_roll_shift_values` against the packed sort column."""
import warnings

import numpy as np
import pandas as pd
import pytest

import conftest
from tsfresh_amd import EfficientFCParameters, MinimalFCParameters, _native, extract_rolled_features
from tsfresh_amd.feature_extraction import data
from tsfresh_amd.utilities.dataframe_functions import roll_views

pytestmark = pytest.mark.gpu


def _both(container, **kw):
    kw.setdefault("default_fc_parameters", MinimalFCParameters())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = extract_rolled_features(container, pack="host", **kw)
        got = extract_rolled_features(container, pack="device", **kw)
    assert list(got.index) == list(want.index) and list(got.columns) == list(want.columns)
    a, b = got.to_numpy(), want.to_numpy()
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(np.nan_to_num(a).view(np.int64), np.nan_to_num(b).view(np.int64))   # bit-equal
    return got


def _series_frame(lengths, seed, ids=None):
    rng = np.random.default_rng(seed)
    return pd.concat([pd.DataFrame({"id": sid if ids is None else ids[sid], "time": np.arange(L), "a": rng.standard_normal(L)})
                      for sid, L in enumerate(lengths)], ignore_index=True)


def _time_order(df):
    return df.sort_values(["time", "id"], kind="stable").reset_index(drop=True)


@pytest.mark.parametrize("kw", [dict(max_timeshift=30, min_timeshift=9), dict(rolling_direction=-3, max_timeshift=25, min_timeshift=5)])
def test_shuffled_two_column_frame(gpu, kw):
    """The frame of tests/test_roll.py: two value columns, so the pack set serves both kinds from one sort."""
    rng = np.random.default_rng(5)
    rows = []
    for sid, L in enumerate([60, 45, 80, 12]):
        rows.append(pd.DataFrame({"id": sid, "time": np.arange(L), "a": rng.standard_normal(L),
                                  "b": np.cumsum(rng.standard_normal(L))}))
    df = pd.concat(rows, ignore_index=True).sample(frac=1.0, random_state=2)
    got = _both(df, column_id="id", column_sort="time", default_fc_parameters=EfficientFCParameters(), **kw)
    assert len(got) > 0 and any(c.startswith("b__") for c in got.columns)


def _two_kinds():
    rng = np.random.default_rng(6)
    rows = []
    for kind, lens in (("a", [31, 20]), ("b", [47, 40])):
        for sid, L in enumerate(lens):
            rows.append(pd.DataFrame({"id": sid, "time": np.arange(L), "kind": kind, "value": rng.standard_normal(L)}))
    return pd.concat(rows, ignore_index=True)


def test_long_frame_whose_other_kind_owns_the_longest_series(gpu):
    df = _two_kinds().sort_values(["time", "id", "kind"], kind="stable").reset_index(drop=True)   # the kinds interleave
    got = _both(df, column_id="id", column_sort="time", column_kind="kind", column_value="value", rolling_direction=3,
                max_timeshift=12, min_timeshift=2)
    shifts_a = {i[1] for i in got.index[got["a__length"].notna()]}
    assert shifts_a and {(s + 1) % 3 for s in shifts_a} == {47 % 3}   # kind a is rolled with kind b's 47 steps


def test_dict_container_rolls_every_entry_with_its_own_steps(gpu):
    long = _two_kinds()
    frames = {k: long[long["kind"] == k].drop(columns="kind").sample(frac=1.0, random_state=3) for k in ("a", "b")}
    got = _both(frames, column_id="id", column_sort="time", column_value="value", rolling_direction=3, max_timeshift=12,
                min_timeshift=2)
    shifts_a = {i[1] for i in got.index[got["a__length"].notna()]}
    assert shifts_a and {(s + 1) % 3 for s in shifts_a} == {31 % 3}


def test_string_ids_and_duplicate_stamps(gpu):
    df = _time_order(_series_frame([14, 9, 20, 3], 7, ids=["s10", "s9", "b", "a"]))
    _both(df, column_id="id", column_sort="time", max_timeshift=4)
    dup = _time_order(_series_frame([14, 9, 20, 3], 8))
    dup["time"] = dup["time"] // 2
    got = _both(dup, column_id="id", column_sort="time", max_timeshift=4)
    assert got.index.duplicated().any()   # duplicate window ids: their rows come in the host route's order


def test_frame_without_a_sort_column_and_frame_in_packed_order(gpu):
    df = _time_order(_series_frame([14, 9, 20, 3], 9))
    got = _both(df.drop(columns="time"), column_id="id", rolling_direction=-2, max_timeshift=6)
    assert {i[1] for i in got.index} <= set(range(20))            # the shift value is ts - 1
    _both(_series_frame([14, 9, 20, 3], 9), column_id="id", column_sort="time", max_timeshift=6)   # uploaded as it is


def test_many_short_series_in_time_order(gpu):
    lengths = np.random.default_rng(10).integers(1, 4, size=5000)
    df = _time_order(_series_frame(lengths, 11))
    got = _both(df, column_id="id", column_sort="time")
    assert len(got) == int(lengths.sum())


def test_more_than_8192_windows_of_real_length_cross_the_chunk_cuts(gpu):
    """70 series of 130 samples, max_timeshift 40: 9 100 windows of 1 .. 41 samples, which the host pipeline cuts into two
    chunks.  A launch sizes its workgroups by its batch, so the device route is bit-equal only while it launches the same
    chunks (tsfa_extract_chunks); EfficientFCParameters has the reductions whose association would show a drift."""
    df = _time_order(_series_frame([130] * 70, 14))
    got = _both(df, column_id="id", column_sort="time", max_timeshift=40, default_fc_parameters=EfficientFCParameters())
    assert len(got) == 70 * 130 > 8192


def test_min_timeshift_above_max_timeshift_gives_no_window(gpu):
    df = _time_order(_series_frame([14, 9, 20, 3], 12))
    outcome = []
    for mode in ("host", "device"):
        try:
            outcome.append(extract_rolled_features(df, column_id="id", column_sort="time", max_timeshift=3, min_timeshift=5,
                                                   default_fc_parameters=MinimalFCParameters(), pack=mode))
        except Exception as exc:   # the same result or the same error
            outcome.append((type(exc), str(exc)))
    if isinstance(outcome[0], tuple):
        assert outcome[1] == outcome[0]
    else:
        assert outcome[0].shape == outcome[1].shape and len(outcome[1]) == 0
        assert list(outcome[0].columns) == list(outcome[1].columns)


def _pack_of(lengths, sort_dtype, seed=13):
    """A DevicePack of series with the given lengths from a frame in time order, its sort column kept."""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.arange(len(lengths)), lengths)
    t = np.concatenate([np.sort(rng.integers(0, 10 ** 6, size=L)) for L in lengths])
    order = np.lexsort((ids, t))
    sort = t.astype(sort_dtype)
    cols = data._device_pack_columns(ids[order], rng.standard_normal(len(ids))[order], sort[order])[1]
    pack = _native.DevicePack(cols[0], cols[2], cols[3], keep_sort=True)
    return pack, sort   # (sort: the column in packed order)


@pytest.mark.parametrize("direction, mts, mn, extra", [(1, None, 0, 0), (1, 7, 2, 0), (-1, 5, 0, 3), (3, 10, 1, 16), (-2, None, 3, 0),
                                                       (1, 3, 5, 0)])
def test_device_windows_equal_roll_views(gpu, direction, mts, mn, extra):
    lengths = np.concatenate([[1, 2, 5, 33, 64, 65, 130], np.random.default_rng(1).integers(1, 41, size=30)])
    pack, _ = _pack_of(lengths, np.int64)
    steps = int(lengths.max()) + extra
    with _native.DeviceWindows(pack, direction, mts, mn, steps) as win:
        gi, frm, until, ts = roll_views(np.concatenate([lengths, [steps]]), direction, mts, mn)
        keep = gi < len(lengths)
        assert win.n_windows == int(keep.sum())
        assert np.array_equal(win.series, gi[keep]) and np.array_equal(win.timeshifts, ts[keep])
        assert np.array_equal(win.starts, pack.offsets[gi[keep]] + frm[keep])
        assert np.array_equal(win.ends, pack.offsets[gi[keep]] + until[keep])
    with pytest.raises(_native.NativeError) as ei:
        _native.DeviceWindows(pack, direction, mts, mn, int(lengths.max()) - 1)
    assert ei.value.code == _native.TSFA_ERR_INVALID
    with pytest.raises(_native.NativeError) as ei:
        _native.DeviceWindows(pack, 0, mts, mn, steps)
    assert ei.value.code == _native.TSFA_ERR_INVALID
    pack.close()


@pytest.mark.parametrize("sort_dtype", ["int64", "float64", "datetime64[ns]"])
def test_shift_values_equal_the_packed_sort_column(gpu, sort_dtype):
    lengths = np.random.default_rng(2).integers(1, 41, size=30)
    pack, sort = _pack_of(lengths, sort_dtype)
    for direction in (1, -2):
        with _native.DeviceWindows(pack, direction, 7, 1) as win:
            got = win.shift_values()
            want = sort[win.ends - 1] if direction > 0 else sort[win.starts]
            assert got.itemsize == sort.itemsize and np.array_equal(got.view(sort.dtype), want)
    pack.close()
    ids = np.repeat(np.arange(3), 4)[::-1].copy()
    cols = data._device_pack_columns(ids, np.arange(12.0), np.arange(12))[1]
    plain = _native.DevicePack(cols[0], cols[2], cols[3])            # no kept sort column
    with _native.DeviceWindows(plain, 1, None, 0) as win:
        with pytest.raises(ValueError):
            win.shift_values()
        lib = _native.load()
        out = np.empty(win.n_windows, dtype=np.int64)
        assert lib.tsfa_roll_shift_values(win._h, plain._h, out.ctypes.data) == _native.TSFA_ERR_INVALID
    plain.close()


def test_extract_windows_pack_writes_every_cell(gpu):
    """conftest's sentinel audit wraps extract_host / extract_windows_host only; on a GPU box its fixture pre-fills every
    plan's result matrix, so a cell no kernel wrote would still hold the sentinel here.  Several row chunks, the last one
    partial, against one chunk; a composite plan (two augmented_dickey_fuller lag selections) equals its host form."""
    from tsfresh_amd.feature_extraction.extraction import _acquire_plan
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    lengths = [60, 45, 80, 12]
    pack, _ = _pack_of(lengths, np.int64)
    values = pack.values_host()
    settings = [EfficientFCParameters(),
                {"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"},
                                                           {"attr": "teststat", "autolag": "BIC"}]}]
    with _native.DeviceWindows(pack, 1, 30, 9) as win:
        assert win.n_windows > 7
        for k, fc in enumerate(settings):
            plan = _acquire_plan(compile_fc_parameters(fc), 0, set())
            assert (type(plan) is not _native.Plan) == (k == 1)
            whole = plan.extract_windows_pack(pack, win)
            parts = plan.extract_windows_pack(pack, win, chunk_rows=7)
            host = plan.extract_windows_host(values, win.starts, win.ends)
            assert whole.shape == (win.n_windows, plan.n_cols)
            for m in (whole, parts, host):
                assert not np.any(m == conftest.SENTINEL)
            assert np.array_equal(np.isnan(whole), np.isnan(host))
            assert np.array_equal(np.nan_to_num(whole).view(np.int64), np.nan_to_num(host).view(np.int64))   # the same launches
            # other cuts are other batches: the workgroup size of a launch follows its longest window and decides the association
            # of the reductions (tests/test_gpu_parity.py, the length classes: "equal to 1e-12, not bit for bit", same bound)
            assert np.array_equal(np.isnan(whole), np.isnan(parts))
            assert np.allclose(np.nan_to_num(whole), np.nan_to_num(parts), rtol=1e-9, atol=1e-9)
            if k == 0:   # the plan's "host_chunks" option moves the host pipeline's cuts: the device form follows them
                plan.set_option("host_chunks", 3)
                try:
                    lib = _native.load()
                    edges = (__import__("ctypes").c_int64 * 17)()
                    assert lib.tsfa_extract_chunks(plan._h, win.n_windows, edges, 17) == 3
                    assert [edges[c] for c in range(4)] == [win.n_windows * c // 3 for c in range(4)]
                    three = plan.extract_windows_pack(pack, win)
                    host3 = plan.extract_windows_host(values, win.starts, win.ends)
                    assert np.array_equal(np.nan_to_num(three).view(np.int64), np.nan_to_num(host3).view(np.int64))
                finally:
                    plan.set_option("host_chunks", 0)
    pack.close()
