"""Inputs, truth and bar shared by the CPU and GPU tests of the p-value columns below tests/parity.py's 1e-9 floor
(tests/test_pvalue_floor.py, tests/test_pvalue_floor_gpu.py); measured numbers: profiles/pvalue_floor.md.

tests/parity.py bounds a dimensionless cell by 1e-6 |want| + 1e-9.  A linear_trend p-value of a trending series of 1024 samples
is 1e-20 .. 1e-300 and the ADF p-value of a stationary series 1e-10 .. 1e-30: below the floor such a cell is compared with
nothing.  Here they are compared a second time, RELATIVE to the true p-value:

  * TREND CASES.  x_i = s (i - (n - 1) / 2) + e_i with e fixed noise of unit variance whose own regression slope was removed,
    so that 1 - r^2 = See / (s^2 Sxx + See) and the slope for a wanted t or p is a closed form.  The slope is rounded to four
    digits and the series is cast ONCE to float32 for the float32 runs; the truth is taken on the values the kernels read.
  * TRUTH without many-digit arithmetic at test time: float64 samples are dyadic rationals, so the five sums of the
    regression are exact Python integers, r^2 and t^2 exact Fractions, |t| their correctly rounded square root and
    p = 2 scipy.special.stdtr(df, -|t|).  tests/test_pvalue_floor.py holds this chain to many-digit arithmetic
    (tests/pvalue_mp.py: r and t from the definition in 60 digits, p by two independent routes) on every case, so the GPU test
    needs neither mpmath nor time.
  * BAR: |got - p| <= 1e-6 p for p >= 1e-290 (parity.RTOL, no floor); a true p below 2^-1022: finite, >= 0, < 2^-1000.
  * CONDITIONING CAP.  p ~ (1 - r^2)^(df / 2) for a small p, and round-off in the sums moves r^2 by about n eps: the relative
    sensitivity of p to the arithmetic is (df / 2) n eps / (1 - r^2) (conditioning_of).  Every case keeps it at or below CAP, a
    tenth of the bar; a target p-value a length cannot reach under the cap (1e-30 from 5 samples asks for 1 - r^2 = 1e-20) is
    replaced by the slope AT half the cap -- the smallest p-value that length may be asked for.  At 65 536 samples the term is
    4.8e-7 / (1 - r^2) whatever the slope: CAP_65536 (below) is that length's own, still under the bar.
  * ADF CASES.  (series, autolag) pairs of stationary series whose many-digit test statistic lies in BAND, where the MacKinnon
    p-value is 1e-30 .. 1e-8; the truth is the oracle's MacKinnon function of the many-digit statistic, stored in
    tests/golden/pvalue_adf_truth.json (a recorded result; the CPU test recomputes every entry and compares).

compare_pvalues is the comparator; it never reads an absolute floor."""
import functools
import json
import math
import os
from fractions import Fraction

import numpy as np

import parity
import route_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float64).eps)
RTOL = parity.RTOL
P_MIN = 1e-290                    # the bar is relative down to here
P_UNDERFLOW = 2.0 ** -1022        # a true p below this: got is finite, >= 0 and < P_TINY
P_TINY = 2.0 ** -1000
CAP = 1e-7
CAP_65536 = 5e-7                  # (df / 2) n eps = 4.77e-7 at r = 0; the cases there keep 1 - r^2 >= 0.97
TINY = Fraction(1.0e-20)          # scipy/stats/_stats_py.py, linregress (the float64 value, exactly)
DTYPES = ("float64", "float32")

CROSS = rc.LAST_IN_LDS["TREND"] + 1      # the first length of the TREND family's HBM build (route_cases.family_params("TREND"))
LONGEST = 65536                          # a = df / 2 = 32 767: the lgamma differences of tsfa_betainc cancel hardest
SHORT_LENGTHS = (3, 4, 5, 8, 16, 17, 64, 65, 256)            # the row form (and, with row_form 0, the wavefront form)
MID_LENGTHS = (257, 1024, 1025, 2049)                        # k_trend, LDS build
LONG_LENGTHS = (CROSS, LONGEST)
LENGTHS = SHORT_LENGTHS + MID_LENGTHS + LONG_LENGTHS

# what a slope is chosen for: ("t2", f): t^2 = f x the branch switch of tsfa_betainc, x < (a + 1) / (a + b + 2) <=>
# t^2 > 3 df / (df + 2) (p around 0.1); ("p", p): that p-value; ("omr2", v): 1 - r^2 = v, for p-values that underflow
TARGETS = (("t2", 0.8), ("t2", 1.25), ("p", 1e-3), ("p", 3e-9), ("p", 3e-10), ("p", 1e-15), ("p", 1e-30), ("p", 1e-60),
           ("p", 1e-100), ("p", 1e-280))
UNDERFLOW = {256: 2.0e-3, 2049: 0.4, LONGEST: 0.97}      # 1 - r^2 per length: (1 - r^2)^(df / 2) = 1e-343, 1e-407, 1e-433


def cap_of(n):
    return CAP_65536 if n == LONGEST else CAP


def conditioning_of(n, omr2):
    return 0.5 * (n - 2) * n * EPS / omr2


# ---- exact sums
def _ints(a):
    """float64 array -> (Python ints m, e) with a[i] == m[i] * 2 ** e exactly."""
    a = np.asarray(a, dtype=np.float64)
    assert np.all(np.isfinite(a))
    m, ex = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    assert np.array_equal(np.ldexp(mi.astype(np.float64), ex - 53), a)
    e = (ex - 53).astype(np.int64)
    nz = mi != 0
    emin = int(e[nz].min()) if nz.any() else 0
    shift = np.where(nz, e - emin, 0)
    return [int(v) << int(s) for v, s in zip(mi.tolist(), shift.tolist())], emin


def exact_r2(t, y):
    """-> (r^2 as a Fraction, sign of the covariance), exactly, for float64 abscissae t and samples y; (0, 0) where a variance
    is 0 (scipy: `if ssxm == 0.0 or ssym == 0.0: r = 0.0`)."""
    tm, _ = _ints(t)
    ym, _ = _ints(y)
    n = len(ym)
    st, sy = sum(tm), sum(ym)
    cxx = n * sum(v * v for v in tm) - st * st
    cyy = n * sum(v * v for v in ym) - sy * sy
    cxy = n * sum(a * b for a, b in zip(tm, ym)) - st * sy
    if cxx == 0 or cyy == 0:
        return Fraction(0), 0
    return Fraction(cxy * cxy, cxx * cyy), (cxy > 0) - (cxy < 0)


def _sqrt_fraction(q):
    """Correctly rounded to within an ulp: float(q) is correctly rounded, and so is math.sqrt."""
    return math.sqrt(float(q))


class Truth:
    """r, t, df, 1 - r^2, p of one regression.  p: 2 * stdtr(df, -|t|); for two samples scipy's own rule."""

    def __init__(self, t, y):
        from scipy.special import stdtr
        y = np.asarray(y, dtype=np.float64)
        self.n, self.df = len(y), len(y) - 2
        if self.n == 2:
            self.r2, self.sign = (Fraction(1), 1 if y[1] > y[0] else -1) if y[0] != y[1] else (Fraction(0), 0)
            self.t, self.p = (math.inf * self.sign if self.sign else 0.0), (1.0 if y[0] == y[1] else 0.0)
        else:
            self.r2, self.sign = exact_r2(t, y)
            self.t2 = self.r2 * self.df / (1 - self.r2 + 2 * TINY + TINY * TINY)
            self.t = self.sign * _sqrt_fraction(self.t2)
            self.p = float(2.0 * stdtr(float(self.df), -abs(self.t)))
        self.r = self.sign * _sqrt_fraction(self.r2)
        self.omr2 = float(1 - self.r2)


# ---- the trend cases
def noise(n):
    """n samples of unit sample variance, zero mean and zero regression slope on 0 .. n - 1.  Deterministic in n."""
    rng = np.random.default_rng([20261021, n])
    e = rng.standard_normal(n)
    k = np.arange(n) - (n - 1) / 2.0
    e = e - e.mean()
    e = e - k * (k @ e) / (k @ k)
    return e / np.sqrt(e @ e / n)


def _t_for_p(df, p):
    """|t| with 2 stdtr(df, -|t|) = p, by bisection on log t (float64 is enough: the slope is rounded to four digits)."""
    from scipy.special import stdtr
    lo, hi = -3.0, 12.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if 2.0 * stdtr(float(df), -10.0 ** mid) > p:
            lo = mid
        else:
            hi = mid
    return 10.0 ** lo


def _slope(n, omr2):
    """s with See / (s^2 Sxx + See) = omr2 for noise(n): See = n, Sxx = n (n^2 - 1) / 12.  Four significant digits."""
    s = math.sqrt((1.0 - omr2) / omr2 * 12.0 / (n * n - 1.0))
    return float("%.4g" % s)


def _omr2_for(n, target):
    df = n - 2
    kind, v = target
    if kind == "omr2":
        return v
    t2 = v * 3.0 * df / (df + 2.0) if kind == "t2" else _t_for_p(df, v) ** 2
    return df / (df + t2)


class Case:
    def __init__(self, label, x, dtype_name, kind, times=None):
        dt = np.dtype(dtype_name)
        self.label, self.dtype_name, self.kind = "%s_%s" % (label, dtype_name), dtype_name, kind
        self.x = np.asarray(x, dtype=np.float64).astype(dt)
        self.n = len(self.x)
        self.times = None if times is None else np.asarray(times, dtype=np.float64)

    @functools.cached_property
    def truth(self):
        t = np.arange(self.n, dtype=np.float64) if self.times is None else self.times
        return Truth(t, self.x.astype(np.float64))


def _signs(n, j):
    """Both signs up to 2049 samples; one, alternating with the target, beyond (a long series costs the oracle and the
    emulation the most)."""
    return (1.0, -1.0) if n <= 2049 else ((1.0,) if j % 2 == 0 else (-1.0,))


def _grid(n):
    """-> [(tag, 1 - r^2, kind)] of one length: every target the cap allows, the others replaced by ONE slope at half the cap."""
    floor = conditioning_of(n, 1.0) / (0.5 * cap_of(n))      # the smallest 1 - r^2 a case of this length is given
    out, replaced = [], False
    for target in TARGETS:
        omr2 = _omr2_for(n, target)
        if n == LONGEST:
            assert omr2 >= 0.97, (target, omr2)      # what CAP_65536 was sized for
        elif omr2 < floor:
            if replaced:
                continue
            omr2, target, replaced = floor, ("cap", 0.5), True
        out.append(("%s%g" % target, omr2, "grid" if target[0] != "cap" else "cap"))
    if n in UNDERFLOW:
        out.append(("underflow", UNDERFLOW[n], "underflow"))
    return out


@functools.lru_cache(maxsize=None)
def trend_cases(dtype_name, lengths=LENGTHS):
    out = []
    for n in lengths:
        e, k = noise(n), np.arange(n) - (n - 1) / 2.0
        for j, (tag, omr2, kind) in enumerate(_grid(n)):
            for sign in _signs(n, j):
                out.append(Case("n%d_%s_%+d" % (n, tag, sign), sign * _slope(n, omr2) * k + e, dtype_name, kind))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases(dtype_name):
    """Two samples (both outcomes of the m == 2 branch), constants (r = 0, p = 1.0 exactly)."""
    return [Case("pair_equal", [1.5, 1.5], dtype_name, "pair"), Case("pair_up", [1.0, 2.0], dtype_name, "pair"),
            Case("pair_down", [0.25, -3.0], dtype_name, "pair"),
            Case("constant_3", np.full(3, 0.1), dtype_name, "constant"), Case("constant_64", np.full(64, -2.5), dtype_name, "constant"),
            Case("constant_300", np.full(300, 1e3), dtype_name, "constant")]


@functools.lru_cache(maxsize=None)
def exact_lines(dtype_name):
    """Lines of small integers: every sum of the regression is exact in float64 in any order, sqrt(ssxm ssym) is exact, and
    r = +-1 exactly in the reference and in the kernels (asserted).  t = sqrt(df / (TINY (2 + TINY))) is of order 1e10; the
    p-value, 6e-11 at 3 samples and 1e-19 at 4, is compared with what the reference returns (4: sum (i - 1.5)^2 = 5 and
    16: 340 are exact; 64 samples underflow: 0.0)."""
    return [Case("line_n%d_%+g" % (n, s), s * np.arange(n), dtype_name, "line") for n in (4, 16, 64) for s in (2.0, -3.0)]


def timewise_cases(dtype_name):
    """linear_trend_timewise: the same construction on time stamps, even (every 15 minutes) and uneven (gaps of 0.5 .. 2 hours
    on a grid of 2^-10 h).  `times` are float64 hours since the first stamp, as the engines take them."""
    out = []
    for n in (5, 17, 65, 256, 257, 1025):
        rng = np.random.default_rng([20261021, n, 2])
        for stamps, hours in (("even", 0.25 * np.arange(n)),
                              ("uneven", np.concatenate([[0.0], np.cumsum(np.round(rng.uniform(0.5, 2.0, n - 1) * 1024) / 1024)]))):
            k = hours - hours.mean()
            e = rng.standard_normal(n)
            e = e - e.mean()
            e = e - k * (k @ e) / (k @ k)
            e = e / np.sqrt(e @ e / n)
            floor = conditioning_of(n, 1.0) / (0.5 * CAP)
            for j, target in enumerate((("t2", 0.8), ("t2", 1.25), ("p", 3e-9), ("p", 3e-10), ("p", 1e-30), ("p", 1e-100), ("p", 1e-280))):
                omr2 = _omr2_for(n, target)
                if omr2 < floor:
                    continue      # (the index cases carry the cap slopes; here a target out of reach is simply not drawn)
                s = float("%.4g" % math.sqrt((1.0 - omr2) / omr2 * n / (k @ k))) * (1.0 if j % 2 == 0 else -1.0)
                out.append(Case("timewise_%s_n%d_%s%g" % ((stamps, n) + target), s * k + e, dtype_name, "grid", times=hours))
    return out


def pack(cases, negate=False):
    """-> (values in the cases' dtype, offsets, times or None) of one ragged batch; negate: the batch of the -x."""
    dt = np.dtype(cases[0].dtype_name)
    assert all(c.dtype_name == cases[0].dtype_name for c in cases)
    values = np.concatenate([(-c.x if negate else c.x) for c in cases]).astype(dt)
    offsets = np.concatenate([[0], np.cumsum([c.n for c in cases])]).astype(np.int64)
    times = None if cases[0].times is None else np.concatenate([c.times for c in cases])
    return values, offsets, times


TREND_PARAMS = {"linear_trend": [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]}
TIMEWISE_PARAMS = {"linear_trend_timewise": [{"attr": a} for a in ("pvalue", "rvalue", "intercept", "slope", "stderr")]}


def is_pvalue(col):
    return 'attr_"pvalue"' in col and parity.feature_of(col) in ("linear_trend", "linear_trend_timewise", "augmented_dickey_fuller")


def check_cell(got, p, underflows=False, extra=0.0):
    """-> None, or what is wrong with `got` against the true p.  extra: what the bar of an ADF cell adds for its statistic."""
    if not np.isfinite(got) or got < 0.0 or got > 1.0:
        return "not a probability"
    if underflows:
        return None if got < P_TINY else "the true p-value underflows float64"
    assert p == 0.0 or p >= P_MIN, p
    err = abs(got - p)
    return None if err <= RTOL * p + extra else "error %.3g = %.3g x the bar" % (err, err / (RTOL * p + extra) if p > 0 or extra > 0 else math.inf)


def compare_pvalues(cases, got_p, what="x", worst=None):
    """got_p[i]: the p-value column of case i.  -> list of mismatches.  worst, a dict, receives {length: largest relative
    error} over the cells with a p of at least P_MIN."""
    bad = []
    assert len(got_p) == len(cases)
    for c, g in zip(cases, got_p):
        tr, g = c.truth, float(g)
        why = check_cell(g, tr.p, underflows=c.kind == "underflow")
        if why:
            bad.append("%s(%s): got %r want %r: %s" % (what, c.label, g, tr.p, why))
        if worst is not None and c.kind != "underflow" and tr.p > 0 and np.isfinite(g):
            worst[c.n] = max(worst.get(c.n, 0.0), abs(g - tr.p) / tr.p)
    return bad


# ---- ADF
BAND = (-18.83, -5.7)
AUTOLAGS = ("AIC", "BIC", "t-stat", None)
# (kind, samples, seed) of adf_series: the three data-driven lag selections of these lie in the band with p < 1e-9 ...
#     (lags 0, 1, 2, 3 and 7 are selected among them)
ADF_SERIES = ((0, 60, 0), (0, 120, 1), (0, 250, 3), (1, 120, 0), (1, 160, 0), (1, 400, 0), (2, 120, 3), (2, 300, 5), (2, 400, 1))
# ... and the fixed lag (autolag None: 17 lags at 380 .. 400 samples, |t| ~ sqrt(n / 18)) of these, found among 115 seeds
ADF_SERIES_FIXED_LAG = ((0, 380, 7), (0, 400, 93), (0, 400, 79), (1, 380, 67))
PHI = (0.0, 0.3, 0.6)
# one series on each side of every cut of mackinnon_p_c1 (autolag "AIC"): t < -18.83 (p = 0.0) | the band | -1.61 | 2.74 | p = 1.0
ADF_EDGES = (("below_-18.83", ("ar", 0, 400, 0)), ("above_-18.83", ("ar", 0, 300, 0)), ("below_-1.61", ("walk", 3)),
             ("above_-1.61", ("walk", 2)), ("above_2.74", ("explosive", 3)))


def adf_series(kind, n, seed):
    """iid (kind 0) or AR(1) with phi = 0.3, 0.6 (kinds 1, 2): float32 values, so that both dtypes read the same numbers."""
    rng = np.random.default_rng([20261021, kind, n, seed])
    x = rng.standard_normal(n)
    for i in range(1, n):
        x[i] += PHI[kind] * x[i - 1]
    return x.astype(np.float32).astype(np.float64)


def adf_edge_series(spec):
    if spec[0] == "ar":
        return adf_series(*spec[1:])
    rng = np.random.default_rng([20261021, 7, spec[1]])
    e = rng.standard_normal(100)
    if spec[0] == "walk":
        return np.cumsum(e).astype(np.float32).astype(np.float64)
    x = e.copy()
    for i in range(1, 100):
        x[i] += 1.04 * x[i - 1]
    return x.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def adf_cases():
    """-> [(label, series, autolag)]"""
    out = [("adf_k%d_n%d_s%d_%s" % (k, n, s, al), adf_series(k, n, s), al) for k, n, s in ADF_SERIES for al in AUTOLAGS[:3]]
    out += [("adf_k%d_n%d_s%d_None" % (k, n, s), adf_series(k, n, s), None) for k, n, s in ADF_SERIES_FIXED_LAG]
    out += [("adf_edge_" + name, adf_edge_series(spec), "AIC") for name, spec in ADF_EDGES]
    return out


@functools.lru_cache(maxsize=None)
def adf_dd_cases():
    """Two stuck-sensor series of tests/test_dd_passes_gpu.py (11 noisy float32 samples, then one level to the end: 101 and 96
    samples) whose statistics, -8.44 and -9.48, lie in the band.  The first pass (fam_ar.h) hands them to the double-double
    pass (fam_ar_dd.h), which writes their p-value: in a build of the emulation whose second pass returned a constant in its
    place, these cells returned the constant.  Nothing a test can read says so at run time -- the launch record shows the
    family's launch, not the list the first pass fills."""
    from test_dd_passes_gpu import _rank_deficient_series
    out = []
    for i in (19, 23):
        x = _rank_deficient_series()[10][i]
        assert np.ptp(x[11:]) == 0 and np.ptp(x[:11]) > 0 and np.array_equal(x.astype(np.float32), x)
        out += [("adf_dd_stuck%d_%s" % (i, al), x, al) for al in ("AIC", "t-stat")]
    return out


ADF_TRUTH_FILE =os.path.join(HERE, "golden", "pvalue_adf_truth.json")


@functools.lru_cache(maxsize=None)
def adf_truth():
    """{label: {"teststat", "usedlag"}} of the many-digit reference (tests/adf_mp.py: adfuller_pinv_mp), as recorded."""
    with open(ADF_TRUTH_FILE) as f:
        return json.load(f)


def compute_adf_truth(cases=None):
    """The many-digit reference of every ADF case (seconds per series: tests/adf_mp.py in 120 digits).  -> what adf_truth
    reads, with the facts the CPU test asserts: "gap", the relative distance of the two best criterion values."""
    from dd_cases import adf_reference, ratios_well_defined
    out = {}
    for label, x, autolag in (adf_cases() + adf_dd_cases() if cases is None else cases):
        t, _, lag, facts = adf_reference(x, autolag)
        out[label] = {"teststat": t, "usedlag": lag, "gap": facts["gap"] if math.isfinite(facts["gap"]) else None,
                      "ratios_well_defined": bool(ratios_well_defined(facts["ratios"])), "perfect": bool(facts["perfect"])}
    return out


def adf_pvalue_bar(t, p):
    """tests/test_dd_passes_gpu.py: _pvalue_bound without its 1e-9: 1e-6 p, and how far the oracle's MacKinnon function moves
    when the statistic moves by its own bar (2e-7 relative)."""
    from oracle.third_party import mackinnonp_c
    moved = max(abs(float(mackinnonp_c(t * (1 + s * 2e-7))) - p) for s in (-1.0, 1.0))
    return RTOL * abs(p), moved


def adf_pvalue_of(t):
    from oracle.third_party import mackinnonp_c
    return float(mackinnonp_c(t))


def compare_adf(labels, names, got, what="x", worst=None):
    """names, got: the three ADF columns of ONE autolag for the cases `labels`.  -> mismatches: usedlag equal, teststat 2e-7
    relative, pvalue within adf_pvalue_bar -- no floor."""
    bad = []
    col = {a: [j for j, n in enumerate(names) if 'attr_"%s"' % a in n][0] for a in ("teststat", "pvalue", "usedlag")}
    for i, label in enumerate(labels):
        tr = adf_truth()[label]
        t, p = tr["teststat"], adf_pvalue_of(tr["teststat"])
        g_t, g_p, g_lag = (float(got[i, col[a]]) for a in ("teststat", "pvalue", "usedlag"))
        if g_lag != tr["usedlag"]:
            bad.append("%s(%s): usedlag got %r want %r" % (what, label, g_lag, tr["usedlag"]))
        if not abs(g_t - t) <= 2e-7 * abs(t):
            bad.append("%s(%s): teststat got %r want %r" % (what, label, g_t, t))
        rel, moved = adf_pvalue_bar(t, p)
        why = check_cell(g_p, p, extra=moved) if p == 0.0 or p >= P_MIN else "the case's p-value is below P_MIN"
        if why:
            bad.append("%s(%s): pvalue got %r want %r: %s" % (what, label, g_p, p, why))
        if worst is not None and p > 0:
            worst[label] = abs(g_p - p) / (rel + moved)
    return bad
