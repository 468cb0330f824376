"""Inputs shared by the tests of the double-double passes (k_ar_degenerate, k_langevin_dd): tests/test_degenerate.py and
tests/test_offset.py run them through the g++ emulation, tests/test_dd_passes_gpu.py through the emulation AND the device,
against many-digit arithmetic (tests/adf_mp.py, tests/polyfit_mp.py).  The many-digit references are computed once per
process (functools.lru_cache) and are read-only."""
import functools
import math
from fractions import Fraction

import numpy as np

AR_ADF = {"ar_coefficient": [{"coeff": c, "k": 10} for c in range(11)],
          "augmented_dickey_fuller": [{"attr": a, "autolag": "AIC"} for a in ("teststat", "pvalue", "usedlag")]}
AUTOLAGS = ("AIC", "BIC", "t-stat", None)
MAX_LEN = 400    # many-digit references are ~1 s per 100 samples and lag selection: longer series are cut to their head


def ar_params(k):
    return {"ar_coefficient": [{"coeff": c, "k": k} for c in range(k + 1)]}


def adf_params(autolag):
    return {"augmented_dickey_fuller": [{"attr": a, "autolag": autolag} for a in ("teststat", "pvalue", "usedlag")]}


def pack(series):
    return np.concatenate(series), np.concatenate([[0], np.cumsum([len(s) for s in series])]).astype(np.int64)


def is_float32(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


def ill_conditioned_series():
    """Designs between the float64 normal equations' reach (pivot test, ~3e4) and the reference's own (1e10): noiseless
    float32 sines, ramps with small noise, large offsets."""
    rng = np.random.default_rng(11)
    t = np.arange(600, dtype=np.float64)
    return [
        np.sin(0.07 * t[:512]).astype(np.float32).astype(np.float64),
        (2.0 + np.cos(0.031 * t[:400])).astype(np.float32).astype(np.float64),
        t[:300] + 1e-4 * rng.standard_normal(300),
        3e4 + rng.standard_normal(256),
        np.round(50 * np.sin(0.02 * t), 3),
        np.concatenate([np.full(40, 2.0), 2.0 + 1e-3 * rng.standard_normal(80)]),
    ]


# (series, usedlag of autolag="AIC"): a lag-search regression fits perfectly (tests/parity.py R5)
def perfect_fit_series():
    return [(np.arange(64.0), 1), (5.0 - 0.5 * np.arange(100.0), 1), (np.tile([1.0, -1.0], 40), 0), (np.arange(200.0) ** 2, 1)]


def exact_nested_ssr(X, y):
    """Residual sums of squares of the nested fits y ~ X[:, :m], m = 1..p, in exact rational arithmetic (LDL^T)."""
    Xf = [[Fraction(float(v)) for v in r] for r in X]
    yf = [Fraction(float(v)) for v in y]
    p = len(Xf[0])
    G = [[sum(r[a] * r[c] for r in Xf) for c in range(p)] for a in range(p)]
    g = [sum(r[a] * v for r, v in zip(Xf, yf)) for a in range(p)]
    yy = sum(v * v for v in yf)
    L = [[Fraction(0)] * p for _ in range(p)]
    D, w, out, acc = [Fraction(0)] * p, [Fraction(0)] * p, [], Fraction(0)
    for j in range(p):
        D[j] = G[j][j] - sum(L[j][k] ** 2 * D[k] for k in range(j))
        for i in range(j + 1, p):
            L[i][j] = (G[i][j] - sum(L[i][k] * L[j][k] * D[k] for k in range(j))) / D[j]
        w[j] = (g[j] - sum(L[j][k] * w[k] * D[k] for k in range(j))) / D[j]
        acc += w[j] ** 2 * D[j]
        out.append(float(yy - acc))
    return out


@functools.lru_cache(maxsize=None)
def tiny_noise_ramp():
    """-> (tiny_noise_ramp_300 = t + 1e-9 noise, cond(X) ~ 5e11; the lag exact rational arithmetic selects by AIC)."""
    import goldens
    g = goldens.load("degenerate")
    x = g["series"][g["labels"].index("tiny_noise_ramp_300")]
    n = len(x)
    M = min(n // 2 - 2, int(math.ceil(12.0 * (n / 100.0) ** 0.25)))
    d = np.diff(x)
    rows = np.arange(M, len(d))
    X = np.column_stack([np.ones(len(rows)), x[rows]] + [d[rows - j] for j in range(1, M + 1)])
    ssr = exact_nested_ssr(X, d[rows])
    nobs = len(rows)
    aic = [nobs * math.log(ssr[m - 1] / nobs) + 2 * m for m in range(2, M + 3)]
    return x, int(np.argmin(aic))


@functools.lru_cache(maxsize=None)
def langevin_second_pass_cases():
    """off + (iid | walk) at offsets 1e2 .. 1e8 whose np.polyfit rank decision is not within BAND of the cut.
    -> ([series], [(60-digit coefficients, kappa of the kept part, rank)])"""
    import polyfit_mp
    rng = np.random.default_rng(5)
    series, want = [], []
    for off in (1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8):
        for kind in ("iid", "walk"):
            e = rng.standard_normal(400)
            x = off + (e if kind == "iid" else np.cumsum(e) * 0.1)
            bm = polyfit_mp.bin_means(x, 30)
            kappa, in_band = polyfit_mp.polyfit_conditioning(bm[0], 3)
            if in_band:
                continue
            coef, _, rank = polyfit_mp.exact_polyfit(bm[0], bm[1], 3)
            series.append(x)
            want.append((coef, kappa, rank))
    return series, want


# ---------------------------------------------------------------------------------------------------------------------
# many-digit references, one per (series, question), shared by every test of the session
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ar_mp(xbytes, k):
    from adf_mp import autoreg_params_pinv_mp
    beta, _, rank, _, ratios = autoreg_params_pinv_mp(np.frombuffer(xbytes, dtype=np.float64), k)
    beta = np.array(beta)
    beta.setflags(write=False)
    return beta, rank, tuple(ratios)


@functools.lru_cache(maxsize=None)
def _adf_mp(xbytes, autolag):
    from adf_mp import adf_pvalue, adfuller_pinv_mp
    t, lag, facts = adfuller_pinv_mp(np.frombuffer(xbytes, dtype=np.float64), autolag)
    return t, adf_pvalue(t), lag, facts


def ar_reference(x, k):
    """-> (AutoReg(x, lags=k, trend="c") params by the many-digit pinv rule, rank, s / s_max of the design)."""
    return _ar_mp(np.ascontiguousarray(x, dtype=np.float64).tobytes(), int(k))


def adf_reference(x, autolag):
    """-> (teststat, pvalue, usedlag, facts) of tests/adf_mp.py: adfuller_pinv_mp."""
    return _adf_mp(np.ascontiguousarray(x, dtype=np.float64).tobytes(), autolag)


EPS = float(np.finfo(np.float64).eps)


def ratios_well_defined(designs, p_of=len):
    """The pinv answer of a design is a function of the data, not of round-off, when no singular value sits between
    "exactly dependent" and "resolved by float64 input": none in (1e-25, 1e-11) s_max, none within 10x of the rank
    threshold p eps."""
    for r in designs:
        r = np.asarray(r, dtype=np.float64)
        cut = p_of(r) * EPS
        if np.any((r > 1e-25) & (r < 1e-11)) or np.any((r > cut / 10.0) & (r < cut * 10.0)):
            return False
    return True


def adf_well_defined(facts):
    return ratios_well_defined(facts["ratios"]) and facts["gap"] > 1e-6
