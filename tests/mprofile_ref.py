"""Brute force of the matrix profile the `windows` route of the reference's matrix_profile computes (fc.py:2385-2470),
written from the definition ("matrix_profile"), not from the kernel's recurrence:

    rho(i, j) = sum_k (x[i+k] - mu_i)(x[j+k] - mu_j) / (w sigma_i sigma_j), clamped to <= 1
    P[i]      = sqrt(2 w (1 - max_j rho(i, j))),  j over |i - j| > ceil(w / 4), flat windows (max == min) excluded

Blocked: a block of rows against all windows at a time, never an L x L array.
"""
import numpy as np

FEATURES = ("min", "max", "mean", "median", "25", "75")
_F = {"min": np.min, "max": np.max, "mean": np.mean, "median": np.median,
      "25": lambda d: np.percentile(d, 25), "75": lambda d: np.percentile(d, 75)}


def exclusion(w):
    return -(-w // 4)   # ceil(w / 4)


def profile(x, w, block_cells=1 << 22):
    """-> P, float64 [n - w + 1] (NaN: a flat window or one without a neighbour), or None when no pair is admissible."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    L = n - w + 1
    e = exclusion(w)
    if w > n or L <= e + 1:
        return None
    win = np.lib.stride_tricks.sliding_window_view(x, w)
    mu = win.mean(axis=1)
    sd = win.std(axis=1)
    flat = win.max(axis=1) == win.min(axis=1)
    with np.errstate(all="ignore"):
        z = (win - mu[:, None]) / sd[:, None]          # L x w
    z[flat] = 0.0
    best = np.full(L, -np.inf)
    rows = max(1, block_cells // L)
    finite = bool(np.isfinite(z).all())
    band = np.arange(-e, e + 1)
    for i0 in range(0, L, rows):
        i1 = min(L, i0 + rows)
        rho = (z[i0:i1] @ z.T) / w
        r = np.repeat(np.arange(i0, i1), len(band))
        c = r + np.tile(band, i1 - i0)
        ok = (c >= 0) & (c < L)
        rho[r[ok] - i0, c[ok]] = -np.inf            # the exclusion zone |i - j| <= ceil(w / 4)
        if flat.any():
            rho[:, flat] = -np.inf                  # a flat window is nobody's neighbour
        if not finite:
            rho[~np.isfinite(rho)] = -np.inf
        best[i0:i1] = rho.max(axis=1)
    best = np.minimum(best, 1.0)
    with np.errstate(all="ignore"):
        p = np.sqrt(2.0 * w * (1.0 - best))
    p[flat | ~np.isfinite(best)] = np.nan
    return p


def feature(p, name):
    """The reference's statistic (fc.py:2455-2467) of a profile; NaN where there is none or nothing finite in it."""
    if p is None:
        return np.nan
    d = p[np.isfinite(p)]
    return float(_F[name](d)) if len(d) else np.nan


def tolerance(w):
    """(relative, absolute): the project's float rule (tests/parity.py) and a floor of 1e-6 sqrt(2 w) -- at P = 0 an error of
    1e-12 in rho, the bound the kernel's fixed restart stride is there to keep."""
    return 1e-6, 1e-6 * np.sqrt(2.0 * w)


def close(got, want, w):
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) and np.isnan(got))
    rel, floor = tolerance(w)
    return abs(got - want) <= max(rel * abs(want), floor)


def reference_unit_test_input():
    """tests/units/feature_extraction/test_feature_calculations.py:2043-2050 of the reference (windows = 36,
    min of the profile pinned at 2.825786727580335)."""
    rs = np.random.RandomState(9999)
    ts = rs.uniform(size=2 ** 10)
    w = 2 ** 5
    subq = ts[0:w].copy()
    ts[w + 100:w + 100 + w] = subq
    return ts
