"""`extract_features_long_tensor(..., nan_policy="drop")`: the rows with a NaN value, a NaN sort key or a NaT stamp are dropped
on the device.  Every case is compared on the bits (a) with `nan_policy="raise"` on the rows a torch boolean mask keeps and,
for one case per form, (b) with `extract_features(frame.dropna())`.  Rows N around one 64-row word and one block past
`TSFA_ROWS_VALID_BLOCK`; ids interleaved, so the pack sorts."""
import numpy as np
import pandas as pd
import pytest
import torch

from tsfresh_amd import MinimalFCParameters, _native, extract_features, extract_features_long_tensor

B = _native.TSFA_ROWS_VALID_BLOCK
TREND = [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]
PARAMS = dict(MinimalFCParameters(), first_location_of_maximum=None, last_location_of_minimum=None, linear_trend=TREND)
TIMED = dict(PARAMS, linear_trend_timewise=TREND)
NAMES = {0: "zeta", 1: "alpha"}
NAT = np.iinfo(np.int64).min


def _gap_rows(gap, N, ids, kinds):
    if gap == "word":   # one whole 64-row word
        return np.arange(64, 128) if N >= 128 else np.arange(min(N, 64))
    if gap == "id_kind":
        return np.flatnonzero((ids == 2) & (kinds == 1))
    return {"none": np.arange(0), "first": np.arange(1), "last": np.arange(N - 1, N), "block": np.arange(B),
            "id": np.flatnonzero(ids == 2), "one_col": np.arange(3, N, 5)}[gap]


def _table(N, layout, dtype, sort, timed, gap):
    """The gapped table as keyword arguments of the entry (tensors on the device) and the boolean mask of the kept rows.
    The gap rows take their NaN in turn from every column that can hold one: a value, the float sort key, the stamp."""
    rng = np.random.default_rng(N + len(layout) + len(gap))
    ids = (np.arange(N) % min(N, 5)).astype(np.int64)
    kinds = (np.arange(N) // 5 % 2).astype(np.int32)
    C = 1 if layout in ("vec", "long") else 3
    x = (rng.standard_normal((N, C)) * 100).astype(dtype)
    order = rng.permutation(N)
    key = {None: None, "int": order.astype(np.int64), "float": order * 0.5}[sort]
    ticks = 10 ** 18 + order.astype(np.int64) * 7 * 10 ** 9 if timed else None
    ways = [w for w, ok in (("value", x.dtype.kind == "f"), ("sort", sort == "float"), ("stamp", timed)) if ok]
    rows = _gap_rows(gap, N, ids, kinds)
    for k, r in enumerate(rows):
        way = "value" if gap == "one_col" else ways[k % len(ways)]
        if way == "value":
            x[r, 1 if gap == "one_col" else r % C] = np.nan
        elif way == "sort":
            key[r] = np.nan
        else:
            ticks[r] = NAT
    keep = np.ones(N, dtype=bool)
    keep[rows] = False
    v = torch.from_numpy(x).cuda()
    if layout == "col":
        v = v.t().contiguous().t()
    elif layout == "step":
        v = torch.from_numpy(np.repeat(x, 2, axis=0)).cuda()[::2]
    elif C == 1:
        v = v[:, 0].contiguous()
    kw = dict(ids=torch.from_numpy(ids).cuda(), values=v, sort=None if key is None else torch.from_numpy(key).cuda(),
              times=None if ticks is None else torch.from_numpy(ticks).cuda())
    if layout == "long":
        kw.update(kinds=torch.from_numpy(kinds).cuda(), kind_names=NAMES)
    return kw, torch.from_numpy(keep).cuda(), (ids, kinds, key, x)


def _same(got, want):
    return got[1] == want[1] and torch.equal(got[2], want[2]) and got[0].shape == want[0].shape and \
        torch.equal(got[0].view(torch.int64), want[0].view(torch.int64))


CASES = [   # N, layout, value dtype, sort, times, gap pattern
    (1, "vec", np.float32, None, False, "none"),
    (63, "row", np.float64, "int", False, "first"),
    (64, "row", np.float32, "float", False, "last"),
    (64, "long", np.float64, None, False, "none"),
    (65, "col", np.float64, "int", True, "word"),
    (65, "vec", np.float64, None, True, "first"),
    (B + 1, "row", np.float32, None, False, "block"),
    (B + 1, "vec", np.float32, "int", False, "block"),
    (B + 1, "row", np.float64, "float", True, "word"),
    (B + 1, "step", np.float32, "int", False, "id"),
    (B + 1, "step", np.float64, None, False, "word"),
    (B + 1, "long", np.float64, "int", False, "id_kind"),
    (B + 1, "long", np.float32, "float", True, "id"),
    (B + 1, "row", np.float64, "int", False, "one_col"),
    (B + 1, "col", np.float32, "float", False, "one_col"),
    (B + 1, "row", np.int32, "float", False, "last"),   # integer values: the drops come from the sort key alone
    (B + 1, "row", np.int32, "float", True, "id"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,layout,dtype,sort,timed,gap", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_drop_equals_raise_on_the_masked_rows(gpu, N, layout, dtype, sort, timed, gap):
    kw, keep, _ = _table(N, layout, dtype, sort, timed, gap)
    params = TIMED if timed else PARAMS
    got = extract_features_long_tensor(default_fc_parameters=params, nan_policy="drop", **kw)
    masked = {k: v[keep] if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    want = extract_features_long_tensor(default_fc_parameters=params, nan_policy="raise", **masked)
    assert int(keep.sum()) < N or gap == "none"
    assert got[0].is_cuda and _same(got, want)
    assert _same(extract_features_long_tensor(default_fc_parameters=params, nan_policy="drop", check_nan=False, **kw), want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,gap", (("row", "one_col"), ("long", "id_kind")))
def test_drop_equals_the_frame_after_dropna(gpu, layout, gap):
    kw, _, (ids, kinds, key, x) = _table(B + 1, layout, np.float64, "int", False, gap)
    if layout == "long":
        df = pd.DataFrame({"id": ids, "kind": [NAMES[k] for k in kinds], "t": key, "v": x[:, 0]})
        form = dict(column_kind="kind", column_value="v")
    else:
        df, form = pd.DataFrame({"id": ids, "t": key, "0": x[:, 0], "1": x[:, 1], "2": x[:, 2]}), {}
    assert df.isna().any().any()
    want = extract_features(df.dropna(), column_id="id", column_sort="t", default_fc_parameters=PARAMS, pack="host", device=0, **form)
    feats, cols, ids_out = extract_features_long_tensor(default_fc_parameters=PARAMS, nan_policy="drop", **kw)
    assert cols == list(want.columns) and np.array_equal(ids_out.cpu().numpy(), want.index.to_numpy())
    g, w = feats.cpu().numpy(), want.to_numpy()
    assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w))
    assert np.array_equal(g[~np.isnan(w)].view(np.uint64), w[~np.isnan(w)].view(np.uint64))


def test_unknown_policy_is_refused_before_the_device():
    with pytest.raises(ValueError, match='"raise" or "drop"'):
        extract_features_long_tensor(np.arange(3), np.zeros(3), nan_policy="bogus")
    with pytest.raises(ValueError, match='"raise" or "drop"'):
        extract_features_long_tensor(np.arange(3), np.zeros(3), nan_policy="drop_per_kind")


@pytest.mark.gpu
def test_no_row_left_raise_stays_and_integer_tables(gpu):
    kw, _, _ = _table(65, "row", np.float64, "int", False, "first")
    with pytest.raises(ValueError, match="Column must not contain NaN values: 0$"):
        extract_features_long_tensor(default_fc_parameters=PARAMS, **kw)
    with pytest.raises(ValueError, match="no row is left"):
        extract_features_long_tensor(kw["ids"], torch.full_like(kw["values"], float("nan")), nan_policy="drop",
                                     default_fc_parameters=PARAMS)
    ints = dict(kw, values=(kw["values"].nan_to_num() * 10).to(torch.int16))   # nothing can be NaN: today's path
    assert _same(extract_features_long_tensor(default_fc_parameters=PARAMS, nan_policy="drop", **ints),
                 extract_features_long_tensor(default_fc_parameters=PARAMS, nan_policy="raise", **ints))
