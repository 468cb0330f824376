"""Plain references for the statistics of tsfresh_amd/csrc/tsfa_relevance.hip (tests/test_relevance_kernels.py): exact
integer or order-statistic arithmetic from the definitions, numpy only.  Nothing here sorts by merging."""
import numpy as np

REAL_FIELDS = ("n_unique", "v_lo", "v_hi", "dis", "xtie", "ntie", "x0", "x1", "n_hi", "ks_d")
DIS_BRUTE_MAX_ROWS = 4097   # up to here `dis` is the O(n^2) definition, above it the Fenwick counter


def dense_rank(v):
    """0-based dense ranks (equal values share a rank; -0.0 == 0.0)."""
    return np.unique(np.asarray(v, dtype=np.float64), return_inverse=True)[1].reshape(-1).astype(np.int64)


def _group_sums(cnt):
    """(sum t(t-1)/2, sum t(t-1)(t-2), sum t(t-1)(2t+5)) over tie-group sizes, in Python integers."""
    pairs = x0 = x1 = 0
    for t in cnt[cnt > 1].tolist():
        pairs += t * (t - 1) // 2
        x0 += t * (t - 1) * (t - 2)
        x1 += t * (t - 1) * (2 * t + 5)
    return pairs, x0, x1


def dis_brute(x, y):
    """#{(i, j): x_i < x_j and y_i > y_j}, the O(n^2) definition in row chunks (on dense ranks: the same order)."""
    xr, yr = dense_rank(x), dense_rank(y)
    dt = np.int16 if len(xr) < 32768 else np.int64
    xr, yr = xr.astype(dt), yr.astype(dt)
    total = 0
    for a in range(0, len(xr), 512):
        total += int(np.count_nonzero((xr[a:a + 512, None] < xr[None, :]) & (yr[a:a + 512, None] > yr[None, :])))
    return total


def dis_fenwick(x, y):
    """The same count in O(n log n): a Fenwick tree over the dense ranks of y, filled in ascending x one tie group of x
    at a time -- every member of a group first asks how many rows of the EARLIER groups have a larger y, then the group
    is inserted.  Rows with equal x never meet, rows with equal y are never counted."""
    xr, yr = dense_rank(x), dense_rank(y)
    order = np.argsort(xr, kind="stable")
    xs, ys = xr[order].tolist(), (yr[order] + 1).tolist()   # 1-based tree positions
    size = int(yr.max()) + 1 if len(ys) else 0
    tree = [0] * (size + 1)
    total = inserted = 0
    g0, n = 0, len(xs)
    while g0 < n:
        g1 = g0
        while g1 < n and xs[g1] == xs[g0]:
            g1 += 1
        for p in range(g0, g1):      # inserted rows with y rank <= ys[p]; the others are discordant with row p
            i, le = ys[p], 0
            while i > 0:
                le += tree[i]
                i -= i & -i
            total += inserted - le
        for p in range(g0, g1):
            i = ys[p]
            while i <= size:
                tree[i] += 1
                i += i & -i
        inserted += g1 - g0
        g0 = g1
    return total


def discordant_pairs(x, y):
    return dis_brute(x, y) if len(x) <= DIS_BRUTE_MAX_ROWS else dis_fenwick(x, y)


def ks_statistic(a, b):
    """The two-sample Kolmogorov-Smirnov statistic as scipy.stats.ks_2samp forms it: the empirical distribution
    functions of both samples over the pooled data (searchsorted(side="right") / n), one difference, then
    max(max(d), clip(-min(d), 0, 1))."""
    a, b = np.sort(np.asarray(a, dtype=np.float64)), np.sort(np.asarray(b, dtype=np.float64))
    pooled = np.concatenate([a, b])
    d = np.searchsorted(a, pooled, side="right") / len(a) - np.searchsorted(b, pooled, side="right") / len(b)
    return float(max(np.max(d), np.clip(-np.min(d), 0, 1)))


def real_column_stats(x, y):
    """The ten fields of tsfa_relevance_real_col for one column x against the real-valued target y."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    u, xr, cnt = np.unique(x, return_inverse=True, return_counts=True)
    xr = xr.reshape(-1).astype(np.int64)
    yr = dense_rank(y)
    xtie, x0, x1 = _group_sums(cnt)
    _, joint = np.unique(xr * (int(yr.max()) + 1) + yr, return_counts=True)
    out = {"n_unique": len(u), "v_lo": float(u[0]), "v_hi": float(u[-1]), "dis": discordant_pairs(x, y),
           "xtie": xtie, "ntie": _group_sums(joint)[0], "x0": float(x0), "x1": float(x1), "n_hi": 0, "ks_d": 0.0}
    if len(u) == 2:
        hi = x == u[-1]
        out["n_hi"] = int(np.count_nonzero(hi))
        out["ks_d"] = ks_statistic(y[hi], y[~hi])
    return out


def class_ks_stats(x, codes, C):
    """[C] Kolmogorov-Smirnov distances of x[codes == k] against x[codes != k] (every class present, none complete)."""
    x, codes = np.asarray(x, dtype=np.float64), np.asarray(codes)
    return np.array([ks_statistic(x[codes == k], x[codes != k]) for k in range(C)])


def impute_stats(col):
    """(max, min, median, count) of the finite cells of one column; (0, 0, 0, 0) without any."""
    col = np.asarray(col, dtype=np.float64)
    fin = col[np.isfinite(col)]
    if len(fin) == 0:
        return 0.0, 0.0, 0.0, 0
    return float(fin.max()), float(fin.min()), float(np.median(fin)), len(fin)
