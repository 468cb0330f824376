"""`extract_features_long_tensor` on the device against `extract_features(frame, pack="host")` on the equivalent frame: `==` on
the bits, equal NaN placement, equal names, equal ids.  Base shape: 37 ids with ragged lengths 1 .. 70, rows in several
orders, the wide and the long form, stamps, a composite plan, the three NaN errors, a frame past one PK_TILE, and the inputs
on the device, on the host and as numpy arrays.  Minimal and Efficient settings only."""
import numpy as np
import pandas as pd
import pytest
import torch

from tsfresh_amd import EfficientFCParameters, MinimalFCParameters, _native, extract_features, extract_features_long_tensor, tensor_long

pytestmark = pytest.mark.gpu

N_IDS = 37
MINIMAL = MinimalFCParameters()
TIMED = dict(MinimalFCParameters(), linear_trend_timewise=[{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")])
COMPOSITE = {"mean": None, "augmented_dickey_fuller": [{"attr": "teststat", "autolag": "AIC"}, {"attr": "pvalue", "autolag": "BIC"}],
             "maximum": None}


def _base(seed=0, C=3, dtype=np.float64, n_ids=N_IDS, max_len=70):
    """ids, sort keys and values [N, C] in packed order: n_ids ids (negative ones among them), ragged lengths 1 .. max_len."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_len + 1, size=n_ids)
    lens[:2] = (1, max_len)
    ids = np.repeat(np.arange(n_ids) * 5 - 40, lens).astype(np.int64)
    sort = np.concatenate([np.arange(L) for L in lens]).astype(np.int64)
    if np.dtype(dtype).kind == "f":
        x = rng.standard_normal((len(ids), C)).astype(dtype)
    else:
        x = rng.integers(-3000, 3000, size=(len(ids), C)).astype(dtype)
    return ids, sort, x


def _wide_frame(ids, sort, x, names, index=None):
    cols = {"id": ids}
    if sort is not None:
        cols["t"] = sort
    for c, k in enumerate(names):
        cols[k] = x[:, c]
    return pd.DataFrame(cols, index=index)


def _assert_equal(got, want_df):
    feats, cols, ids_out = got
    assert cols == list(want_df.columns)
    assert ids_out.is_cuda and np.array_equal(ids_out.cpu().numpy(), want_df.index.to_numpy())
    g, w = feats.cpu().numpy(), want_df.to_numpy()
    assert feats.is_cuda and feats.dtype == torch.float64 and g.shape == w.shape
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert np.array_equal(g[ok].view(np.uint64), w[ok].view(np.uint64))


def _same(a, b):
    """torch.equal on the bit patterns: NaN cells count as equal where both hold the same NaN."""
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _check_wide(ids, sort, x, names=None, params=MINIMAL, **kw):
    names = [str(c) for c in range(x.shape[1])] if names is None else names
    want = extract_features(_wide_frame(ids, sort, x, names), column_id="id", column_sort=None if sort is None else "t",
                            default_fc_parameters=params, pack="host", device=0)
    got = extract_features_long_tensor(torch.from_numpy(ids).cuda(), torch.from_numpy(x).cuda(),
                                       sort=None if sort is None else torch.from_numpy(sort).cuda(),
                                       kind_names=names, default_fc_parameters=params, **kw)
    _assert_equal(got, want)
    return got


@pytest.fixture
def sets_made(monkeypatch):
    """The pack sets the entry makes, for a look at their flags."""
    made = []

    class Recording(_native.DevicePackSet):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append((self.flags, self.n_passes))
    monkeypatch.setattr(tensor_long._native, "DevicePackSet", Recording)
    return made


def test_rows_shuffled_interleaved_and_already_packed(gpu, sets_made):
    ids, sort, x = _base()
    rng = np.random.default_rng(1)
    shuffle = rng.permutation(len(ids))
    _check_wide(ids[shuffle], sort[shuffle], x[shuffle], names=["b", "a", "c"])
    by_time = np.lexsort((ids, sort))   # rows in time order, the ids interleaved
    _check_wide(ids[by_time], sort[by_time], x[by_time])
    assert not any(flags & _native.TSFA_PACK_IN_ORDER for flags, _ in sets_made) and all(p > 0 for _, p in sets_made)
    del sets_made[:]
    _check_wide(ids, sort, x)
    assert sets_made == [(_native.TSFA_PACK_IN_ORDER, 0)]


def test_ties_in_sort_and_no_sort_keep_the_row_order(gpu):
    ids, sort, x = _base(seed=2)
    shuffle = np.random.default_rng(3).permutation(len(ids))
    ids, sort, x = ids[shuffle], sort[shuffle], x[shuffle]
    _check_wide(ids, sort // 3, x)            # ties: the sort is stable
    _check_wide(ids, (sort // 3).astype(np.float64) * 0.5 - 4.0, x)
    _check_wide(ids, None, x)                 # the order inside an id is the row order


@pytest.mark.parametrize("id_dtype", (np.int32, np.int64, np.int16, np.uint8))
def test_id_dtypes_and_negative_ids(gpu, id_dtype):
    ids, sort, x = _base(seed=4)
    if np.dtype(id_dtype).kind == "u":
        ids = ids + 40
    shuffle = np.random.default_rng(5).permutation(len(ids))
    ids = ids.astype(id_dtype)
    assert (ids < 0).any() or np.dtype(id_dtype).kind == "u"
    _, _, ids_out = _check_wide(ids[shuffle], sort[shuffle], x[shuffle])
    assert str(ids_out.dtype) == "torch." + np.dtype(id_dtype).name


@pytest.mark.parametrize("C", (1, 3, 33))
@pytest.mark.parametrize("dtype", (np.float32, np.float64, np.int16))
def test_column_counts_and_value_types(gpu, C, dtype):
    ids, sort, x = _base(seed=6 + C, C=C, dtype=dtype)
    shuffle = np.random.default_rng(7).permutation(len(ids))
    ids, sort, x = ids[shuffle], sort[shuffle], x[shuffle]
    got = _check_wide(ids, sort, x)
    if C == 1:   # a plain [N] column is the same frame
        one = extract_features_long_tensor(torch.from_numpy(ids).cuda(), torch.from_numpy(x[:, 0].copy()).cuda(),
                                           sort=torch.from_numpy(sort).cuda(), default_fc_parameters=MINIMAL)
        assert _same(one[0], got[0]) and one[1] == got[1]
    if C == 3:   # a column-major matrix and a sliced view give the same bits through the other kernel
        xt = torch.from_numpy(np.asfortranarray(x)).cuda()
        assert xt.stride() == (1, len(ids))
        big = torch.from_numpy(np.repeat(x, 2, axis=1)).cuda()[:, ::2]
        for view in (xt, big):
            other = extract_features_long_tensor(torch.from_numpy(ids).cuda(), view, sort=torch.from_numpy(sort).cuda(),
                                                 default_fc_parameters=MINIMAL)
            assert _same(other[0], got[0])


def test_efficient_settings(gpu):
    ids, sort, x = _base(seed=8, C=2, dtype=np.float32)
    shuffle = np.random.default_rng(9).permutation(len(ids))
    _check_wide(ids[shuffle], sort[shuffle], x[shuffle], names=["u", "v"], params=EfficientFCParameters())


def _long_rows(seed=10):
    """Three kinds with unequal id sets, names out of code order; rows shuffled."""
    ids, sort, x = _base(seed=seed)
    names = {2: "zeta", 11: "alpha", 7: "mid"}
    rng = np.random.default_rng(seed + 1)
    uniq = np.unique(ids)
    keep = {2: uniq[::2], 11: uniq[1:], 7: uniq[:20]}
    parts = []
    for c, code in enumerate(names):
        sel = np.isin(ids, keep[code])
        parts.append((ids[sel], np.full(sel.sum(), code), sort[sel], x[sel, c]))
    ids, kinds, sort, vals = (np.concatenate(p) for p in zip(*parts))
    shuffle = rng.permutation(len(ids))
    return ids[shuffle], kinds[shuffle], sort[shuffle], vals[shuffle], names


def test_long_form_unequal_id_sets_and_names_out_of_code_order(gpu):
    ids, kinds, sort, vals, names = _long_rows()
    df = pd.DataFrame({"id": ids, "kind": [names[k] for k in kinds], "t": sort, "v": vals})
    want = extract_features(df, column_id="id", column_sort="t", column_kind="kind", column_value="v", default_fc_parameters=MINIMAL,
                            pack="host", device=0)
    assert np.isnan(want.to_numpy()).any() and want.columns[0].startswith("alpha__")
    got = extract_features_long_tensor(torch.from_numpy(ids).cuda(), torch.from_numpy(vals).cuda(), sort=torch.from_numpy(sort).cuda(),
                                       kinds=torch.from_numpy(kinds.astype(np.int16)).cuda(), kind_names=names,
                                       default_fc_parameters=MINIMAL)
    _assert_equal(got, want)
    # equal id sets: the blocks are written in place
    both = np.concatenate([ids, ids])
    k2 = np.repeat([1, 0], len(ids))
    v2 = np.concatenate([vals, -vals])
    df = pd.DataFrame({"id": both, "kind": np.where(k2 == 1, "one", "nil"), "t": np.concatenate([sort, sort]),
                       "c": np.concatenate([kinds, kinds]), "v": v2})
    df["id"] = df["id"] * 100 + df["c"]
    want = extract_features(df.drop(columns="c"), column_id="id", column_sort="t", column_kind="kind", column_value="v",
                            default_fc_parameters=MINIMAL, pack="host", device=0)
    got = extract_features_long_tensor(df["id"].to_numpy(), v2, sort=df["t"].to_numpy(), kinds=k2, kind_names=["nil", "one"],
                                       default_fc_parameters=MINIMAL)
    _assert_equal(got, want)


@pytest.mark.parametrize("params", (TIMED, dict(COMPOSITE, **{"linear_trend_timewise": [{"attr": "slope"}]})), ids=("minimal", "composite"))
def test_times_against_the_datetime_index_frame(gpu, params):
    ids, sort, x = _base(seed=12, C=2)
    rng = np.random.default_rng(13)
    ticks = 1_600_000_000 * 10 ** 9 + rng.integers(0, 10 ** 13, size=len(ids))
    order = np.lexsort((ticks, ids))
    ids, ticks, x = ids[order], ticks[order], x[order]   # in an id the rows ascend in time, as a DatetimeIndex frame's do
    shuffle = rng.permutation(len(ids))
    ids, ticks, x = ids[shuffle], ticks[shuffle], x[shuffle]
    index = pd.DatetimeIndex(ticks.view("M8[ns]"))
    want = extract_features(_wide_frame(ids, None, x, ["p", "q"], index=index).assign(t=ticks), column_id="id", column_sort="t",
                            default_fc_parameters=params, pack="host", device=0)
    assert any("linear_trend_timewise" in c for c in want.columns)
    dev = [torch.from_numpy(a).cuda() for a in (ids, x, ticks)]
    got = extract_features_long_tensor(dev[0], dev[1], sort=dev[2], kind_names=["p", "q"], times=dev[2], default_fc_parameters=params)
    _assert_equal(got, want)
    same = extract_features_long_tensor(ids, x, sort=ticks, kind_names=["p", "q"], times=ticks.view("M8[ns]"), default_fc_parameters=params)
    assert _same(same[0], got[0])


def test_composite_plan(gpu):
    ids, sort, x = _base(seed=14, C=2)
    shuffle = np.random.default_rng(15).permutation(len(ids))
    _check_wide(ids[shuffle], sort[shuffle], x[shuffle], params=COMPOSITE)
    ids, kinds, sort, vals, names = _long_rows(seed=16)
    df = pd.DataFrame({"id": ids, "kind": [names[k] for k in kinds], "t": sort, "v": vals})
    want = extract_features(df, column_id="id", column_sort="t", column_kind="kind", column_value="v", default_fc_parameters=COMPOSITE,
                            pack="host", device=0)
    _assert_equal(extract_features_long_tensor(ids, vals, sort=sort, kinds=kinds, kind_names=names, default_fc_parameters=COMPOSITE), want)


def test_nan_value_sort_key_and_stamp_raise(gpu):
    ids, sort, x = _base(seed=18)
    shuffle = np.random.default_rng(19).permutation(len(ids))
    ids, sort, x = ids[shuffle], sort[shuffle], x[shuffle]
    xn = x.copy()
    xn[11, 1] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: v$"):
        extract_features_long_tensor(ids, xn, sort=sort, kind_names=["u", "v", "w"], default_fc_parameters=MINIMAL)
    with pytest.raises(ValueError, match="Column must not contain NaN values: v$"):
        extract_features(_wide_frame(ids, sort, xn, ["u", "v", "w"]), column_id="id", column_sort="t", default_fc_parameters=MINIMAL,
                         pack="host", device=0)
    kinds = np.arange(len(ids)) % 2
    with pytest.raises(ValueError, match="Column must not contain NaN values: odd$"):
        extract_features_long_tensor(ids, xn[:, 1], sort=sort, kinds=kinds, kind_names=["even", "odd"], default_fc_parameters=MINIMAL)
    fs = sort.astype(np.float64)
    fs[5] = np.nan
    with pytest.raises(ValueError, match="Column must not contain NaN values: sort$"):
        extract_features_long_tensor(ids, x, sort=fs, default_fc_parameters=MINIMAL)
    ticks = np.arange(len(ids), dtype=np.int64) * 10 ** 9
    ticks[7] = np.iinfo(np.int64).min
    with pytest.raises(ValueError, match="times must not contain NaT / NaN"):
        extract_features_long_tensor(ids, x, sort=sort, times=ticks, default_fc_parameters=TIMED)
    feats, _, _ = extract_features_long_tensor(ids, xn, sort=sort, default_fc_parameters=MINIMAL, check_nan=False)
    assert torch.isnan(feats).any()


def test_five_thousand_rows(gpu):
    """Past one PK_TILE of 4096 rows: two tiles of the sort, the boundary scan and the hours."""
    ids, sort, x = _base(seed=20, C=2, n_ids=200, max_len=66)
    ids, sort, x = ids[:5000], sort[:5000], x[:5000]
    assert len(ids) == 5000
    shuffle = np.random.default_rng(21).permutation(5000)
    _check_wide(ids[shuffle], sort[shuffle], x[shuffle])
    ticks = 10 ** 18 + sort * 10 ** 9 * 7
    index = pd.DatetimeIndex(ticks[shuffle].view("M8[ns]"))
    want = extract_features(_wide_frame(ids[shuffle], sort[shuffle], x[shuffle], ["0", "1"], index=index), column_id="id", column_sort="t",
                            default_fc_parameters=TIMED, pack="host", device=0)
    _assert_equal(extract_features_long_tensor(ids[shuffle], x[shuffle], sort=sort[shuffle], times=ticks[shuffle],
                                               default_fc_parameters=TIMED), want)


def test_device_host_and_numpy_inputs_give_the_same_bits(gpu):
    ids, sort, x = _base(seed=22, dtype=np.float32)
    shuffle = np.random.default_rng(23).permutation(len(ids))
    ids, sort, x = ids[shuffle], sort[shuffle], x[shuffle]
    as_numpy = extract_features_long_tensor(ids, x, sort=sort, default_fc_parameters=MINIMAL)
    host = extract_features_long_tensor(torch.from_numpy(ids), torch.from_numpy(x), sort=torch.from_numpy(sort), default_fc_parameters=MINIMAL)
    dev = _check_wide(ids, sort, x)
    for other in (as_numpy, host):
        assert other[0].is_cuda and _same(other[0], dev[0]) and other[1] == dev[1] and torch.equal(other[2], dev[2])
