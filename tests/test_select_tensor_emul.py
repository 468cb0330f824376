"""The device tails, the FDR step-up and the mask compaction of the tensor selection (tsfresh_amd/csrc/rel_tails.h) without a
GPU: the g++ -DTSFA_EMUL build of the kernel bodies (tests/emul/emul_rel_tails.cpp) against scipy -- not against this package's
own host tails -- and against `fdr_reject`."""
import math

import numpy as np
import pytest

import emul_rel_tails_lib as E

P_TOL = dict(rel=1e-9, abs=1e-300)   # the project's tolerance for p-values (test_selection._check_against_golden)


def _same(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == pytest.approx(want, **P_TOL)


def _class_stats(X, codes, n_classes):
    """What tsfa_relevance_classes leaves per column, by scipy / numpy: (n_unique, tie_term, rank_sums, hi_counts, class_n)."""
    from scipy import stats
    n, m = X.shape
    n_unique, tie, rs, hc = np.zeros(m, np.int64), np.zeros(m), np.zeros((m, n_classes)), np.zeros((m, n_classes), np.int64)
    for j in range(m):
        _, cnt = np.unique(X[:, j], return_counts=True)
        n_unique[j] = len(cnt)
        tie[j] = float(np.sum(cnt.astype(float) ** 3 - cnt))
        ranks = stats.rankdata(X[:, j])
        for k in range(n_classes):
            rs[j, k] = ranks[codes == k].sum()
            hc[j, k] = int(np.sum(X[codes == k, j] == X[:, j].max()))
    return n_unique, tie, rs, hc, np.bincount(codes, minlength=n_classes)


def test_mann_whitney_normal_tail_matches_scipy():
    from scipy import stats
    rng = np.random.default_rng(1)
    for trial in range(200):
        n1, n2 = int(rng.integers(9, 41)), int(rng.integers(9, 41))   # below 9 an untied trial is the exact route (flagged, below)
        x, z = rng.standard_normal(n1), rng.standard_normal(n2)
        if trial % 2:
            x, z = np.round(x, 0), np.round(z, 0)
        allv = np.concatenate([x, z])
        _, cnt = np.unique(allv, return_counts=True)
        got = E.mwu_normal(stats.rankdata(allv)[:n1].sum(), n1, n2, float(np.sum(cnt.astype(float) ** 3 - cnt)))
        want = stats.mannwhitneyu(x, z, use_continuity=True, alternative="two-sided").pvalue
        assert _same(got, want), (trial, got, want)
    # every value equal: s == 0 and u - mu - 0.5 < 0 -> z = -inf, p = erfc(-inf) = 2 clipped to 1 (scipy says the same)
    assert E.mwu_normal(10 * 21 / 2.0, 10, 10, 20.0 ** 3 - 20) == 1.0


def test_small_untied_samples_are_flagged_not_served():
    rng = np.random.default_rng(3)
    for trial in range(20):
        n1, n0 = int(rng.integers(1, 9)), int(rng.integers(1, 30))
        X = rng.standard_normal((n1 + n0, 1))
        codes = np.array([0] * n1 + [1] * n0)
        p, route, typ, n_host = E.tails_classes(*_class_stats(X, codes, 2))
        assert typ.tolist() == [2] and route.tolist() == [[E.HOST_MWU_EXACT, E.HOST_MWU_EXACT]]
        assert np.isnan(p).all() and n_host == 2


# (a, b, c, d) by the length of the support lo .. hi of the hypergeometric distribution, lo = max(0, a + c - (c + d)),
# hi = min(a + b, a + c).  With both row sums >= the first column's sum n the support is 0 .. n: length n + 1.
# Length 1 needs an empty margin (then the answer is 1.0 without a sum).  `a, c = b, d` (the symmetric tables of
# test_host_tails_match_scipy) gives the odd lengths 2 min(a, c) + 1; tables with equal row sums have the same mirror
# property (pmf(k) = pmf(n - k), equal up to rounding: the 1e-7 slack decides) and reach the even lengths too.
FISHER_TABLES = {
    1: [(0, 0, 3, 4), (3, 4, 0, 0), (0, 5, 0, 7), (5, 0, 7, 0), (0, 0, 0, 0)],
    2: [(1, 4, 0, 5), (0, 5, 1, 4), (1, 0, 0, 1), (0, 3, 1, 9)],
    63: [(31, 31, 40, 40), (10, 80, 52, 38), (20, 70, 42, 48), (62, 10, 0, 90), (0, 100, 62, 1)],
    64: [(20, 60, 43, 37), (43, 37, 20, 60), (5, 95, 58, 12), (63, 40, 0, 80)],
    65: [(32, 32, 50, 50), (10, 90, 54, 46), (54, 46, 10, 90), (30, 40, 34, 80)],
    128: [(50, 150, 77, 123), (77, 123, 50, 150), (127, 3, 0, 200), (60, 70, 67, 300)],
    129: [(64, 64, 100, 100), (30, 170, 98, 102), (98, 102, 30, 170), (1, 500, 127, 140)],
    4097: [(2048, 2048, 2500, 2500), (2000, 3000, 2096, 2904), (2096, 2904, 2000, 3000), (1900, 2200, 2196, 2000)],
}


@pytest.mark.parametrize("length", sorted(FISHER_TABLES))
def test_fisher_tail_matches_scipy_across_the_wavefront_seams(length):
    from scipy import stats
    for a, b, c, d in FISHER_TABLES[length]:
        n1, n2, n = a + b, c + d, a + c
        empty = n1 == 0 or n2 == 0 or n == 0 or b + d == 0
        if empty:
            assert length == 1 and E.fisher(a, b, c, d) == 1.0
            continue
        assert min(n1, n) - max(0, n - n2) + 1 == length
        want = stats.fisher_exact([[a, b], [c, d]])[1]
        assert E.fisher(a, b, c, d) == pytest.approx(want, **P_TOL), (a, b, c, d)


def test_fisher_tail_matches_scipy_on_random_tables():
    from scipy import stats
    rng = np.random.default_rng(1)
    for trial in range(200):
        a, b, c, d = [int(v) for v in rng.integers(0, 50, 4)]
        if trial % 5 == 0:
            a, c = b, d
        assert E.fisher(a, b, c, d) == pytest.approx(stats.fisher_exact([[a, b], [c, d]])[1], **P_TOL), (a, b, c, d)


def _kendall_stats(x, y):
    from tsfresh_amd.feature_selection.significance_tests import target_tie_statistics
    n = len(x)
    dis = sum(1 for i in range(n) for j in range(n) if x[i] < x[j] and y[i] > y[j])
    _, cnt = np.unique(x, return_counts=True)
    cnt = cnt[cnt > 1].astype(float)
    xtie, x0, x1 = int((cnt * (cnt - 1) // 2).sum()), float((cnt * (cnt - 1) * (cnt - 2)).sum()), float(
        (cnt * (cnt - 1) * (2 * cnt + 5)).sum())
    _, cj = np.unique(np.stack([x, y], 1), axis=0, return_counts=True)
    ntie = int((cj * (cj - 1) // 2).sum())
    ytie, y0, y1 = target_tie_statistics(np.unique(y, return_inverse=True)[1])
    return n, dis, xtie, ntie, x0, x1, ytie, y0, y1


def test_kendall_tail_matches_scipy():
    from scipy import stats
    rng = np.random.default_rng(2)
    for trial in range(60):   # the draws test_ks_tail_matches_scipy makes before its Kendall pairs
        n1, n2 = int(rng.integers(2, 400)), int(rng.integers(2, 400))
        rng.standard_normal(n1), rng.standard_normal(n1 if trial % 4 == 0 else n2)
    rng.standard_normal(12000), rng.standard_normal(9000)
    pairs = []
    for trial in range(20):
        n = int(rng.integers(5, 60))
        pairs.append((np.round(rng.standard_normal(n), 1), np.round(rng.standard_normal(n), 1)))
    x = np.zeros(30)
    x[7] = 1.0                                     # tied with itself everywhere except one row
    pairs.append((x, np.round(rng.standard_normal(30), 1)))
    pairs.append((np.zeros(12), np.arange(12.0)))  # xtie == tot: NaN
    for x, y in pairs:
        want = stats.kendalltau(x, y, method="asymptotic").pvalue
        got = E.kendall(*_kendall_stats(x, y))
        assert _same(got, want), (got, want)
    assert math.isnan(E.kendall(*_kendall_stats(*pairs[-1])))


def test_routes_of_the_class_tables():
    rng = np.random.default_rng(5)
    n = 45
    codes = np.array([0] * 5 + [1] * 20 + [2] * 20)
    untied = rng.standard_normal(n)
    X = np.stack([untied, np.round(untied, 0), (untied > 0).astype(float), np.full(n, 2.5)], axis=1)
    stats_ = _class_stats(X, codes, 3)
    p, route, typ, n_host = E.tails_classes(*stats_)
    assert typ.tolist() == [2, 2, 1, 0]
    assert route[0].tolist() == [E.HOST_MWU_EXACT, E.MWU_NORMAL, E.MWU_NORMAL] and math.isnan(p[0, 0])   # class 0 has 5 rows
    assert route[1].tolist() == [E.MWU_NORMAL] * 3 and not np.isnan(p[1]).any()                           # ... but ties
    assert route[2].tolist() == [E.FISHER] * 3 and not np.isnan(p[2]).any()
    assert route[3].tolist() == [E.NONE] * 3 and np.isnan(p[3]).all()
    assert n_host == 1
    # 'smir': every real cell is the host's, the binary and the constant column keep their routes
    p, route, typ, n_host = E.tails_classes(*stats_, with_ks=True)
    assert route[0].tolist() == [E.HOST_KS] * 3 and route[1].tolist() == [E.HOST_KS] * 3 and np.isnan(p[:2]).all()
    assert route[2].tolist() == [E.FISHER] * 3 and route[3].tolist() == [E.NONE] * 3 and n_host == 6
    # the Fisher cells against scipy, from the counts the sweep leaves
    from scipy import stats
    for k in range(3):
        x1, y1 = X[:, 2] == 1.0, codes == k
        tab = [[int(np.sum(y1 & x1)), int(np.sum(y1 & ~x1))], [int(np.sum(~y1 & x1)), int(np.sum(~y1 & ~x1))]]
        assert p[2, k] == pytest.approx(stats.fisher_exact(tab)[1], **P_TOL)


def test_routes_of_the_real_table():
    cols = np.zeros(3, dtype=E.REAL_COL_DTYPE)
    cols["n_unique"] = [1, 2, 17]
    cols["dis"][2], cols["n_hi"][1], cols["ks_d"][1] = 40, 5, 0.4
    p, route, typ, n_host = E.tails_real(cols, 20, 0, 0.0, 0.0)
    assert typ.tolist() == [0, 1, 2] and route.tolist() == [E.NONE, E.HOST_KS, E.KENDALL] and n_host == 1
    assert math.isnan(p[0]) and math.isnan(p[1]) and 0.0 < p[2] < 1.0


def _c_m(m, independent):
    return 1.0 if independent else float(np.sum(1.0 / np.arange(1, m + 1)))


def _check_fdr(p, alpha=0.1):
    from tsfresh_amd.feature_selection.significance_tests import fdr_reject
    p = np.asarray(p, dtype=np.float64)
    for independent in (True, False):
        rel_t, rel, nsig, pmin = E.fdr(p, np.full(len(p), 2, np.uint8), alpha, _c_m(len(p), independent))
        want = fdr_reject(p, alpha, independent)
        assert np.array_equal(rel_t[:, 0], want) and np.array_equal(rel, want) and np.array_equal(nsig, want.astype(np.int32))
        assert np.array_equal(pmin, p, equal_nan=True)
    return want


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_fdr_equals_fdr_reject(m):
    rng = np.random.default_rng([m, 7])
    p = rng.random(m) ** 3
    want = _check_fdr(p)
    assert m < 63 or (want.any() and not want.all())
    q = p.copy()
    q[rng.random(m) < 0.2] = np.nan                        # NaN sorts last and is never rejected
    _check_fdr(q)
    _check_fdr(np.round(p, 2))                              # exact ties
    assert _check_fdr(np.zeros(m)).all()
    assert not _check_fdr(np.ones(m)).any()


def test_fdr_at_a_threshold_bit_for_bit():
    from tsfresh_amd.feature_selection.significance_tests import fdr_reject
    m, alpha = 40, 0.1
    for independent in (True, False):
        factor = np.arange(1, m + 1) / float(m)
        if not independent:
            factor = factor / np.sum(1.0 / np.arange(1, m + 1))
        thr = factor * alpha
        p = np.ones(m)
        p[:12] = thr[11]                                     # p_(12) equals its threshold, p_(1) .. p_(11) exceed theirs
        rel = E.fdr(p, np.full(m, 2, np.uint8), alpha, _c_m(m, independent))[1]
        assert rel.tolist() == fdr_reject(p, alpha, independent).tolist() == [True] * 12 + [False] * 28
        p[:12] = np.nextafter(thr[11], 1.0)                  # one ulp above: nothing is rejected
        rel = E.fdr(p, np.full(m, 2, np.uint8), alpha, _c_m(m, independent))[1]
        assert not rel.any() and not fdr_reject(p, alpha, independent).any()


def test_fdr_leaves_constant_columns_out_and_combines_tables():
    from tsfresh_amd.feature_selection.significance_tests import fdr_reject
    rng = np.random.default_rng(11)
    n_cols, alpha = 300, 0.1
    types = rng.integers(0, 3, n_cols).astype(np.uint8)
    p = rng.random((n_cols, 3)) ** 4
    p[types == 0] = np.nan
    live = types != 0
    for independent in (True, False):
        want = np.zeros((n_cols, 3), dtype=bool)
        for t in range(3):
            want[live, t] = fdr_reject(p[live, t], alpha, independent)   # m = the columns that are not constant
        counts = want.sum(axis=1)
        assert 0 < counts.max() and (counts == 1).any() and (counts == 3).any()
        c_m = _c_m(int(live.sum()), independent)
        rel_t, rel, nsig, pmin = E.fdr(p, types, alpha, c_m)
        assert np.array_equal(rel_t, want) and np.array_equal(rel, want.any(axis=1)) and np.array_equal(nsig, counts)
        assert np.isnan(pmin[~live]).all() and np.array_equal(pmin[live], p[live].min(axis=1))
        for n_significant in (1, 2, 3):
            rel_t, rel, nsig, _ = E.fdr(p, types, alpha, c_m, n_significant=n_significant, multiclass=True)
            assert np.array_equal(rel_t, want) and np.array_equal(nsig, counts) and np.array_equal(rel, counts >= n_significant)


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_compaction(n):
    rng = np.random.default_rng(n)
    for mask in (np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.3, rng.random(n) < 0.97):
        for nt in (1024, 64, 3):
            assert E.compact(mask, nt).tolist() == np.nonzero(mask)[0].tolist()
