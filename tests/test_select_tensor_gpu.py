"""The tensor selection on the GPU: `impute_tensor`, `calculate_relevance_tensor`, `select_features_tensor` and
`extract_relevant_features_tensor` against scipy (oracle/selection.py), against `fdr_reject` on the downloaded p-values, and
against the frame entry points.

The input of the relevance tests is a 24-column matrix seeded `np.random.default_rng([n, classes, 1])` (classes = 0: regression):
y is a permutation of arange(n) % classes, or a standard normal vector rounded to one decimal; s is the class-0-minus-last-class
indicator, or the standardised y; the columns are 8 x `normal + 0.15 j s`, 4 x `round(normal + 0.3 j s)`, 6 x
`(0.4 j s + normal > 0)`, one column of zeros with a single 1, one constant column of 2.5 and 4 noise columns (j = 1, 2, ...; the
columns are drawn in this order, after y).  scipy finds 12 to 20 of the 24 columns relevant over the cases below, and no p-value
closer than 0.0078 (relative) to its step-up threshold.
n runs over the seams of the sort tiles (2048 / 4096 rows)."""
import functools
import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch   # before the native library: one HIP runtime in the process, the one torch brings

pytestmark = pytest.mark.gpu

P_TOL = dict(rel=1e-9, abs=1e-300)
NS = [40, 300, 2049, 4097]
# (n, classes): classes = 0 is the regression; 40 rows in 5 classes are 8 rows a class: the exact Mann-Whitney route, left out
TARGETS = [(n, c) for n in NS for c in (2, 3, 5, 0) if not (c and n // c <= 8)]
NAMES = ["shift%d" % j for j in range(1, 9)] + ["round%d" % j for j in range(1, 5)] + ["bin%d" % j for j in range(1, 7)] + [
    "single", "const", "noise1", "noise2", "noise3", "noise4"]


@functools.lru_cache(maxsize=None)
def _case(n, classes):
    rng = np.random.default_rng([n, classes, 1])
    if classes:
        y = rng.permutation(np.arange(n) % classes).astype(np.int64)
        s = (y == 0).astype(float) - (y == classes - 1).astype(float)
    else:
        y = np.round(rng.standard_normal(n), 1)
        s = (y - y.mean()) / y.std()
    cols = [rng.standard_normal(n) + 0.15 * j * s for j in range(1, 9)]
    cols += [np.round(rng.standard_normal(n) + 0.3 * j * s) for j in range(1, 5)]
    cols += [(0.4 * j * s + rng.standard_normal(n) > 0).astype(float) for j in range(1, 7)]
    single = np.zeros(n)
    single[int(rng.integers(n))] = 1.0
    cols += [single, np.full(n, 2.5)] + [rng.standard_normal(n) for _ in range(4)]
    X = np.ascontiguousarray(np.stack(cols, axis=1))
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@functools.lru_cache(maxsize=None)
def _reference(n, classes):
    """scipy on the CPU, once per input -> (types [24], p [24, T]); the p-values do not depend on the FDR settings.  For two
    classes the oracle only reports the smaller of the two tables' p-values; the two tables test the same split (Mann-Whitney
    and Fisher are symmetric in the samples), so both cells are held to it."""
    from oracle.selection import relevance_table
    X, y = _case(n, classes)
    frame, target = pd.DataFrame(X, columns=NAMES), pd.Series(y)
    table = relevance_table(frame, target, multiclass=classes > 2)
    types = np.array([{"constant": 0, "binary": 1, "real": 2}[table[f]["type"]] for f in NAMES])
    labels = sorted(set(y.tolist())) if classes else [None]
    p = np.full((len(NAMES), len(labels)), np.nan)
    for j, f in enumerate(NAMES):
        if types[j] == 0:
            continue
        for k, label in enumerate(labels):
            p[j, k] = table[f]["p_value_" + str(label)] if classes > 2 else table[f]["p_value"]
    return types, p


def _reference_masks(n, classes, independent, fdr_level=0.05):
    """-> (per-table masks by the oracle's FDR, smallest relative distance of a p-value to its step-up threshold)."""
    from oracle.selection import fdr
    types, p = _reference(n, classes)
    live = types != 0
    m = int(live.sum())
    masks = np.zeros(p.shape, dtype=bool)
    thr = np.arange(1, m + 1) / float(m) * fdr_level
    if not independent:
        thr = thr / np.sum(1.0 / np.arange(1, m + 1))
    distance = np.inf
    for k in range(p.shape[1]):
        masks[live, k] = fdr(p[live, k], fdr_level, independent)
        distance = min(distance, float(np.min(np.abs(np.sort(p[live, k]) - thr) / thr)))
    return masks, distance


def _device(n, classes, **kw):
    from tsfresh_amd import calculate_relevance_tensor
    X, y = _case(n, classes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return calculate_relevance_tensor(torch.from_numpy(X.copy()).cuda(), torch.from_numpy(y.copy()), columns=NAMES, **kw)


@pytest.mark.parametrize("n,classes", TARGETS)
def test_p_values_match_scipy_and_nothing_hides_behind_the_host_route(gpu, n, classes):
    from tsfresh_amd import _native as N
    types, want = _reference(n, classes)
    res = _device(n, classes)
    assert res.types.cpu().numpy().tolist() == types.tolist()
    routes, got = res.routes.cpu().numpy(), res.p_values.cpu().numpy()
    by_type = {0: N.TSFA_ROUTE_NONE, 1: N.TSFA_ROUTE_FISHER, 2: N.TSFA_ROUTE_MWU_NORMAL} if classes else {
        0: N.TSFA_ROUTE_NONE, 1: N.TSFA_ROUTE_HOST_KS, 2: N.TSFA_ROUTE_KENDALL}
    assert routes.tolist() == [[by_type[t]] * want.shape[1] for t in types]
    assert res.host_cells == (0 if classes else 7)   # regression: the six graded binary columns and the single-1 column
    assert res.labels == (sorted(set(_case(n, classes)[1].tolist())) if classes else [])
    for j in range(len(NAMES)):
        for k in range(want.shape[1]):
            print(NAMES[j], k, routes[j, k], got[j, k], want[j, k])
            assert (math.isnan(want[j, k]) and math.isnan(got[j, k])) or got[j, k] == pytest.approx(want[j, k], **P_TOL)


@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("n,classes", TARGETS)
def test_masks_match_fdr_reject_and_the_frame_entry(gpu, n, classes, independent):
    from tsfresh_amd import calculate_relevance_table
    from tsfresh_amd.feature_selection.significance_tests import fdr_reject
    res = _device(n, classes, hypotheses_independent=independent)
    p, types = res.p_values.cpu().numpy(), res.types.cpu().numpy()
    live = types != 0
    # the mask of the downloaded p-values
    want = np.zeros(p.shape, dtype=bool)
    for k in range(p.shape[1]):
        want[live, k] = fdr_reject(p[live, k], 0.05, independent)
    assert np.array_equal(res.relevant_per_table.cpu().numpy(), want)
    assert np.array_equal(res.relevant.cpu().numpy(), want.any(axis=1))
    assert np.array_equal(res.n_significant.cpu().numpy(), want.sum(axis=1).astype(np.int32))
    p_min = res.p_value.cpu().numpy()
    assert np.isnan(p_min[~live]).all() and np.array_equal(p_min[live], p[live].min(axis=1))
    # the frame entry: only comparable when no reference p-value sits on its threshold
    masks, distance = _reference_masks(n, classes, independent)
    assert distance > 1e-6
    assert 12 <= masks.any(axis=1).sum() <= 20   # what the oracle finds on these inputs: neither nothing nor everything
    X, y = _case(n, classes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        table = calculate_relevance_table(pd.DataFrame(X, columns=NAMES), pd.Series(y), hypotheses_independent=independent)
    assert res.relevant.cpu().numpy().tolist() == [bool(table.loc[f, "relevant"]) for f in NAMES]
    assert res.relevant.cpu().numpy().tolist() == masks.any(axis=1).tolist()


@pytest.mark.parametrize("n_significant", [1, 2, 3])
@pytest.mark.parametrize("n,classes", [(n, c) for n, c in TARGETS if c > 2])
def test_multiclass_counts_the_tables(gpu, n, classes, n_significant):
    from tsfresh_amd import calculate_relevance_table
    from tsfresh_amd.feature_selection.significance_tests import fdr_reject
    res = _device(n, classes, multiclass=True, n_significant=n_significant)
    p, types = res.p_values.cpu().numpy(), res.types.cpu().numpy()
    live = types != 0
    want = np.zeros(p.shape, dtype=bool)
    for k in range(p.shape[1]):
        want[live, k] = fdr_reject(p[live, k], 0.05, False)
    assert np.array_equal(res.relevant_per_table.cpu().numpy(), want)
    assert np.array_equal(res.n_significant.cpu().numpy(), want.sum(axis=1).astype(np.int32))
    assert np.array_equal(res.relevant.cpu().numpy(), want.sum(axis=1) >= n_significant)
    masks, distance = _reference_masks(n, classes, False)
    assert distance > 1e-6
    X, y = _case(n, classes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        table = calculate_relevance_table(pd.DataFrame(X, columns=NAMES), pd.Series(y), multiclass=True, n_significant=n_significant)
    assert res.relevant.cpu().numpy().tolist() == [bool(table.loc[f, "relevant"]) for f in NAMES]
    assert res.n_significant.cpu().numpy().tolist() == [int(table.loc[f, "n_significant"]) for f in NAMES]


def test_fdr_in_table_batches(gpu):
    """The batch loop of `tsfa_relevance_fdr`: the three tables of a 3-class target in batches of 2 (a batch of 2 and a batch
    of 1; the sweep in front of it then runs in column batches of 2 as well) against the oracle's masks and p-values, and
    against the single batch."""
    from tsfresh_amd import _native as N
    n, classes, n_significant = 300, 3, 2
    masks, distance = _reference_masks(n, classes, False)
    types, p = _reference(n, classes)
    assert masks.shape[1] == 3 and distance > 1e-6
    whole = _device(n, classes, multiclass=True, n_significant=n_significant)
    N.set_library_option("relevance_batch", 2)
    try:
        res = _device(n, classes, multiclass=True, n_significant=n_significant)
    finally:
        N.set_library_option("relevance_batch", 0)
    assert np.array_equal(res.relevant_per_table.cpu().numpy(), masks)
    assert np.array_equal(res.relevant.cpu().numpy(), masks.sum(axis=1) >= n_significant)
    assert np.array_equal(res.n_significant.cpu().numpy(), masks.sum(axis=1).astype(np.int32))
    live, p_min = types != 0, res.p_value.cpu().numpy()
    assert np.isnan(p_min[~live]).all() and p_min[live] == pytest.approx(p[live].min(axis=1), **P_TOL)
    assert np.array_equal(p_min[live], res.p_values.cpu().numpy()[live].min(axis=1))
    for name in ("p_values", "p_value", "relevant_per_table", "relevant", "n_significant"):   # NaN: the constant column
        assert np.array_equal(getattr(res, name).cpu().numpy(), getattr(whole, name).cpu().numpy(), equal_nan=True), name


@pytest.mark.parametrize("n,classes", [(300, 3), (2049, 0), (4097, 2)])
def test_selected_matrix_is_the_named_columns(gpu, n, classes):
    from tsfresh_amd import select_features, select_features_tensor
    X, y = _case(n, classes)
    Xd = torch.from_numpy(X.copy()).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = _device(n, classes)
        got, names, indices = select_features_tensor(Xd, y.copy(), columns=NAMES)
        plain = select_features_tensor(Xd, y.copy())
        frame = select_features(pd.DataFrame(X, columns=NAMES), pd.Series(y))
    mask = res.relevant
    assert got.is_cuda and got.dtype == torch.float64 and indices.dtype == torch.int32 and indices.is_cuda
    assert torch.equal(indices.long(), torch.nonzero(mask)[:, 0]) and 12 <= len(names) <= 20
    assert torch.equal(got, Xd[:, mask]) and got.shape == (n, len(names))
    assert names == [NAMES[j] for j in indices.tolist()] and plain[1] == indices.tolist() and torch.equal(plain[0], got)
    assert sorted(names) == sorted(frame.columns)
    # a row-strided view and a float32 copy of the same matrix
    wide = torch.full((n, 40), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 3:27] = Xd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert torch.equal(select_features_tensor(wide[:, 3:27], y.copy())[0], got)


def test_nothing_selected_gives_an_empty_matrix_and_the_warning(gpu):
    from tsfresh_amd import select_features_tensor
    X, y = _case(300, 3)
    shuffled = np.random.default_rng(5).permutation(y)
    with pytest.warns(RuntimeWarning, match="No feature was found relevant"):
        got, names, indices = select_features_tensor(torch.from_numpy(X.copy()).cuda(), shuffled, fdr_level=1e-12)
    assert got.shape == (300, 0) and names == [] and indices.shape == (0,)


def test_constant_columns_are_named_in_the_warning(gpu):
    from tsfresh_amd import calculate_relevance_tensor
    X, y = _case(300, 2)
    with pytest.warns(RuntimeWarning, match=r"\[test_feature_significance\] Constant features: const$"):
        calculate_relevance_tensor(torch.from_numpy(X.copy()).cuda(), y.copy(), columns=NAMES)


def test_host_routes_are_filled_in_before_the_fdr_step(gpu):
    """'smir' (every real cell is a Kolmogorov-Smirnov tail) and a class of 5 rows on untied columns (exact Mann-Whitney):
    the host's values land in the device array and the table equals the frame entry's."""
    from tsfresh_amd import _native as N
    from tsfresh_amd import calculate_relevance_table, calculate_relevance_tensor
    X, y = _case(300, 3)
    small = np.where(np.arange(300) < 5, 0, 1 + (np.arange(300) % 2))   # class 0 has 5 rows
    for target, kw in ((y, dict(test_for_binary_target_real_feature="smir")), (small, {})):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = calculate_relevance_tensor(torch.from_numpy(X.copy()).cuda(), target.copy(), columns=NAMES, **kw)
            table = calculate_relevance_table(pd.DataFrame(X, columns=NAMES), pd.Series(target), **kw)
        routes = res.routes.cpu().numpy()
        host = routes >= N.TSFA_ROUTE_HOST_MWU_EXACT
        assert res.host_cells == int(host.sum()) > 0
        if kw:
            assert (routes[res.types.cpu().numpy() == 2] == N.TSFA_ROUTE_HOST_KS).all()
        else:   # the untied real columns against class 0; the rounded columns have ties and keep the normal tail
            assert (routes[:8, 0] == N.TSFA_ROUTE_HOST_MWU_EXACT).all() and (routes[8:12] == N.TSFA_ROUTE_MWU_NORMAL).all()
            assert not host[:, 1:].any()
        assert not np.isnan(res.p_values.cpu().numpy()[host]).any()
        assert res.relevant.cpu().numpy().tolist() == [bool(table.loc[f, "relevant"]) for f in NAMES]
        for j, f in enumerate(NAMES):
            if f != "const":
                assert res.p_value.cpu().numpy()[j] == pytest.approx(table.loc[f, "p_value"], **P_TOL)


def test_impute_tensor(gpu):
    from tsfresh_amd import _native, impute_tensor
    rng = np.random.default_rng(9)
    X = rng.standard_normal((301, 7))
    X[rng.random(X.shape) < 0.1] = np.nan
    X[rng.random(X.shape) < 0.05] = np.inf
    X[rng.random(X.shape) < 0.05] = -np.inf
    X[:, 4] = np.nan
    want = X.copy()
    _native.impute_matrix(want)
    Xd = torch.from_numpy(X.copy()).cuda()
    assert impute_tensor(Xd) is Xd
    assert np.array_equal(Xd.cpu().numpy(), want) and not np.isnan(want).any()
    wide = torch.full((301, 12), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2:9] = torch.from_numpy(X)
    impute_tensor(wide[:, 2:9])                                  # a row-strided view: the cells around it stay
    assert np.array_equal(wide[:, 2:9].cpu().numpy(), want) and bool(torch.isnan(wide[:, :2]).all()) and bool(torch.isnan(wide[:, 9:]).all())
    host = torch.from_numpy(X.copy())
    assert np.array_equal(impute_tensor(host).numpy(), want)     # a CPU tensor, in place as well
    with pytest.raises(ValueError, match="contiguous rows"):
        impute_tensor(torch.from_numpy(X.copy()).cuda().t())     # column-strided
    with pytest.raises(ValueError, match="float64"):
        impute_tensor(torch.zeros((3, 3), dtype=torch.float32, device="cuda"))


def test_the_whole_chain_equals_the_frame_chain(gpu):
    from tsfresh_amd import MinimalFCParameters, extract_relevant_features, extract_relevant_features_tensor
    rng = np.random.default_rng(21)
    B, n = 60, 64
    labels = rng.permutation(np.arange(B) % 3)
    x = rng.standard_normal((B, 2, n))
    x[:, 0, :] += 0.8 * labels[:, None]                          # channel 0's level depends on the label
    fc = MinimalFCParameters()
    fc.update({"abs_energy": None, "cid_ce": [{"normalize": True}], "has_duplicate": None})
    frame = pd.DataFrame({"id": np.repeat(np.arange(B), n), "time": np.tile(np.arange(n), B),
                          "a": x[:, 0, :].reshape(-1), "b": x[:, 1, :].reshape(-1)})
    y = pd.Series(labels, index=np.arange(B))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = extract_relevant_features(frame, y, column_id="id", column_sort="time", default_fc_parameters=fc,
                                         device_resident=True)
        got, names = extract_relevant_features_tensor(torch.from_numpy(x).cuda(), torch.from_numpy(labels), kinds=["a", "b"],
                                                      default_fc_parameters=fc)
    assert len(names) > 0 and sorted(names) == sorted(want.columns) and got.shape == (B, len(names))
    host = got.cpu().numpy()
    for j, f in enumerate(names):
        assert np.array_equal(host[:, j], want[f].to_numpy()), f


def test_errors(gpu):
    from tsfresh_amd import calculate_relevance_tensor, select_features_tensor
    X, y = _case(40, 2)
    Xd = torch.from_numpy(X.copy()).cuda()
    bad = Xd.clone()
    bad[3, 5] = float("nan")
    with pytest.raises(ValueError, match="^Feature shift6 contains NaN values$"):
        calculate_relevance_tensor(bad, y.copy(), columns=NAMES)
    with pytest.raises(ValueError, match="^Feature 5 contains NaN values$"):
        select_features_tensor(bad, y.copy())
    yf = np.linspace(0.0, 1.0, 40)
    yf[7] = np.nan
    with pytest.raises(ValueError, match="^Target contains NaN values$"):
        calculate_relevance_tensor(Xd, yf)
    with pytest.raises(ValueError, match="^ml_task must be one of: 'auto', 'classification', 'regression'$"):
        calculate_relevance_tensor(Xd, y.copy(), ml_task="ranking")
    with pytest.raises(ValueError, match="Please use a valid entry for test_for_binary_target_real_feature"):
        calculate_relevance_tensor(Xd, y.copy(), test_for_binary_target_real_feature="other")
    with pytest.raises(ValueError, match="^Feature selection is only possible if more than 1 label/class is provided$"):
        calculate_relevance_tensor(Xd, np.zeros(40, dtype=np.int64))
    with pytest.raises(ValueError, match=r"one entry per row of X \(40\)"):
        calculate_relevance_tensor(Xd, y[:39].copy())
    with pytest.raises(ValueError, match="columns must name the 24 columns"):
        calculate_relevance_tensor(Xd, y.copy(), columns=NAMES[:5])
    # an explicit task wins over the dtype
    res = calculate_relevance_tensor(Xd, y.astype(np.float64), ml_task="classification", columns=NAMES, check_nan=False)
    assert res.ml_task == "classification" and res.p_values.shape == (24, 2)
