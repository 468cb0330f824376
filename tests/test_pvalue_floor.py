"""The p-value columns below tests/parity.py's 1e-9 floor, on the CPU: the oracle and the g++ build of the kernel sources against
the true p-value, RELATIVE (cases, truth and bar: tests/pvalue_cases.py; many-digit arithmetic: tests/pvalue_mp.py,
tests/adf_mp.py).  The `-m gpu` twin is tests/test_pvalue_floor_gpu.py.

What tests/parity.py cannot see: a linear_trend, linear_trend_timewise or augmented_dickey_fuller p-value below 1e-9 is
compared with its floor alone -- 0.0, or 1e40 times the value, passes (test_the_comparator_has_teeth_where_parity_has_none
writes the gap down).  The code behind these cells is hand-written: a Lanczos log-gamma, a continued fraction, the branch
switch of the incomplete beta function (tsfa_common.h), MacKinnon's polynomials (fam_ar.h).

Measured numbers (this file prints them; profiles/pvalue_floor.md keeps them)."""
import math
import os

import numpy as np
import pytest

import parity
import pvalue_cases as pc
from engines import emul_engine, oracle_engine

DTYPES = pc.DTYPES
_memo = {}


def _trend(dtype_name):
    return pc.trend_cases(dtype_name) + pc.edge_cases(dtype_name)


def _run(which, kind, dtype_name):
    """-> (cases, names, matrix) of the oracle / the emulation on the index cases ("trend"), the exact lines ("lines") or the
    time-stamped cases ("timewise") of a dtype.  Both engines read float64: the float32 samples widened."""
    key = (which, kind, dtype_name)
    if key not in _memo:
        cases = {"trend": _trend, "lines": pc.exact_lines, "timewise": pc.timewise_cases}[kind](dtype_name)
        values, offsets, times = pc.pack(cases)
        engine = oracle_engine if which == "oracle" else emul_engine
        params = pc.TIMEWISE_PARAMS if kind == "timewise" else pc.TREND_PARAMS
        names, got = engine(params, values.astype(np.float64), offsets, times=times)
        _memo[key] = (cases, names, got)
    return _memo[key]


def _pcol(names):
    js = [j for j, n in enumerate(names) if pc.is_pvalue(n)]
    assert len(js) == 1, names
    return js[0]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def test_the_trend_cases_cover_what_they_are_meant_to():
    below = 0
    for d in DTYPES:
        cs = pc.trend_cases(d)
        assert {c.n for c in cs} == set(pc.LENGTHS) and pc.CROSS == 19327 and pc.LONGEST == 65536
        for n in pc.LENGTHS:
            mine = [c for c in cs if c.n == n and c.kind != "underflow"]
            df = n - 2
            switch = 3.0 * df / (df + 2.0)      # tsfa_betainc: x < (a + 1) / (a + b + 2) <=> t^2 > 3 df / (df + 2)
            t2 = [c.truth.t ** 2 for c in mine]
            assert any(0.5 * switch < v < switch for v in t2) and any(switch < v < 2.0 * switch for v in t2), (n, switch, sorted(t2)[:4])
            assert {np.sign(c.truth.t) for c in mine} == {1.0, -1.0}, n
            ps = [c.truth.p for c in mine]
            assert any(1e-4 < p < 1e-2 for p in ps), (n, ps)
            if n >= 5:      # (3 and 4 samples: the conditioning cap ends at p = 4e-5 and 3e-8)
                assert any(1e-9 < p < 1e-8 for p in ps) and any(1e-10 < p < 1e-9 for p in ps), (n, ps)
            if n >= 16:
                assert any(1e-31 < p < 1e-29 for p in ps), (n, ps)
            if n >= 64:
                assert any(1e-101 < p < 1e-99 for p in ps), (n, ps)
            if n >= 256:
                assert any(1e-281 < p < 1e-279 for p in ps), (n, ps)
        for c in _trend(d) + pc.timewise_cases(d):
            tr = c.truth
            if c.kind in ("pair", "constant"):
                assert tr.p == (0.0 if c.label.startswith(("pair_up", "pair_down")) else 1.0), (c.label, tr.p)
                continue
            # the conditioning cap, case by case: the bar must never measure the conditioning of a case
            assert pc.conditioning_of(c.n, tr.omr2) <= pc.cap_of(c.n), (c.label, pc.conditioning_of(c.n, tr.omr2))
            if c.kind == "underflow":
                assert tr.p < pc.P_UNDERFLOW, (c.label, tr.p)
            else:
                assert tr.p >= pc.P_MIN, (c.label, tr.p)
        assert {c.n for c in cs if c.kind == "underflow"} == set(pc.UNDERFLOW)
        below += sum(0.0 < c.truth.p < 1e-9 for c in cs if c.kind != "underflow")
        # float32 cases are float32 values, and what a slope was chosen for survives the cast
        assert all(np.array_equal(c.x.astype(np.float32), c.x) for c in cs) == (d == "float32")
    print("\nlinear_trend cells with a true p below 1e-9: %d" % below)
    assert below >= 150, below      # the tests live where the old bar is blind
    assert pc.conditioning_of(pc.LONGEST, 1.0) > pc.CAP      # why that length has a cap of its own (pvalue_cases docstring)
    assert pc.CAP_65536 < pc.RTOL


def _mp_pair(job):
    """(df, |t|) -> (log10 of the many-digit p, relative distance of the two routes, of scipy from the quadrature)."""
    import mpmath as mp
    from scipy.special import stdtr
    import pvalue_mp as pm
    df, t = job
    q = pm.pvalue_quad_mp(t, df)
    lg = float(mp.log10(q))
    s = pm.pvalue_sum_mp(t, df, lg)
    sp = 2.0 * float(stdtr(float(df), -t))
    return lg, float(abs(s - q) / q), (float(abs(mp.mpf(sp) - q) / q) if lg > -300 else sp)


def _pairs():
    """Every distinct (df, |t|) whose p-value a test of this file or of the GPU file takes from scipy."""
    out = {}
    for d in DTYPES:
        for c in _trend(d) + pc.timewise_cases(d):
            if c.kind not in ("pair", "constant"):
                out[(c.truth.df, abs(c.truth.t))] = c
    return out


def test_the_two_many_digit_routes_agree_and_scipy_is_pinned_to_them():
    """p = 2 sf(|t|, df) by the finite sums (arctangent form for odd df) and by a quadrature after a change of variable: 1e-12
    relative on every (df, t) of the case set.  2 * scipy.special.stdtr(df, -|t|), the truth of every other test, lies within
    1e-10 of them: its argument x = df / (df + t^2) is formed in float64 and p ~ x^(df / 2) moves by (df / 2) eps = 4e-12 per ulp
    of it at 65 536 samples; 1e-10 leaves that room and is 1e-4 of the bar."""
    import multiprocessing as mpc
    pairs = _pairs()
    jobs = sorted(pairs, key=lambda k: -k[0])
    with mpc.get_context("spawn").Pool(min(os.cpu_count() or 1, 8)) as pool:
        res = pool.map(_mp_pair, jobs, chunksize=4)
    worst_routes = worst_scipy = 0.0
    for (df, t), (lg, routes, scipy_gap) in zip(jobs, res):
        c = pairs[(df, t)]
        assert routes <= 1e-12, (c.label, df, t, routes)
        worst_routes = max(worst_routes, routes)
        if c.kind == "underflow":
            assert lg < math.log10(pc.P_UNDERFLOW) and scipy_gap < pc.P_TINY, (c.label, lg, scipy_gap)      # (scipy's own value)
        else:
            assert lg > math.log10(pc.P_MIN), (c.label, lg)
            assert scipy_gap <= 1e-10, (c.label, df, t, scipy_gap)
            worst_scipy = max(worst_scipy, scipy_gap)
    print("\n%d (df, t) pairs: the two routes differ by at most %.2g, scipy from them by at most %.2g" % (len(jobs), worst_routes, worst_scipy))


def test_the_exact_sums_are_the_definition_in_60_digits():
    """r, t and 1 - r^2 of tests/pvalue_cases.py (exact integer sums, one rounding at the end) against the centred sums of the
    definition in 60 digits (tests/pvalue_mp.py): every index case up to 2049 samples, the deepest case of the two long lengths,
    and every time-stamped case."""
    import mpmath as mp
    import pvalue_mp as pm
    checked = 0
    for d in DTYPES:
        long_ones = [c for c in pc.trend_cases(d) if c.n > 2049 and "p1e-280" in c.label]
        assert len(long_ones) == 2
        for c in [c for c in pc.trend_cases(d) if c.n <= 2049] + long_ones + pc.timewise_cases(d):
            t = np.arange(c.n, dtype=np.float64) if c.times is None else c.times
            r, tstat, omr2 = pm.regression_mp(t, c.x.astype(np.float64))
            tr = c.truth
            assert abs(tr.r - r) <= 4e-16 * abs(r), (c.label, tr.r, float(r))
            assert abs(tr.t - tstat) <= 4e-16 * abs(tstat), (c.label, tr.t, float(tstat))
            assert abs(tr.omr2 - omr2) <= 4e-16 * omr2, (c.label, tr.omr2, float(omr2))
            checked += 1
    print("\nexact sums against the 60-digit definition: %d cases" % checked)
    assert checked >= 500, checked


# ---------------------------------------------------------------------------------------------------------------------
# the oracle and the emulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trend", "timewise"])
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("which", ["oracle", "emul"])
def test_the_bar_is_met_on_every_case(which, dtype_name, kind):
    cases, names, got = _run(which, kind, dtype_name)
    assert len(names) == 5 and got.shape == (len(cases), 5)
    worst = {}
    bad = pc.compare_pvalues(cases, got[:, _pcol(names)], what=which, worst=worst)
    print("\n%s %s %s: %d cases, largest relative error per length: %s"
          % (which, kind, dtype_name, len(cases), {n: "%.2g" % v for n, v in sorted(worst.items())}))
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    assert np.all((got[:, _pcol(names)] >= 0.0) & (got[:, _pcol(names)] <= 1.0))
    if which == "emul":      # the other four attributes, the way every other test compares them
        _, onames, want = _run("oracle", kind, dtype_name)
        assert onames == names
        bad = parity.compare(names, got, want, [c.x.astype(np.float64) for c in cases])
        assert not bad, bad[:8]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_exact_line_returns_what_the_reference_returns(dtype_name):
    """r = +-1 exactly, t of order 1e10: the p-value is a function of TINY alone -- 1e-19 at 4 samples, 3e-139 at 16, 0.0 at
    64 -- and is compared with the reference's own value, 1e-6 relative and no floor."""
    cases, names, want = _run("oracle", "lines", dtype_name)
    _, _, got = _run("emul", "lines", dtype_name)
    jp, jr = _pcol(names), names.index('value__linear_trend__attr_"rvalue"')
    for i, c in enumerate(cases):
        assert abs(want[i, jr]) == 1.0 and got[i, jr] == want[i, jr], (c.label, want[i, jr], got[i, jr])
        assert abs(got[i, jp] - want[i, jp]) <= pc.RTOL * want[i, jp], (c.label, got[i, jp], want[i, jp])
        assert (want[i, jp] == 0.0) == (c.n == 64) and (c.n == 64 or want[i, jp] < 1e-18), (c.label, want[i, jp])


def tight_bound(c):
    """What float64 arithmetic on a correctly rounded math library owes the true p-value of a case (the emulation's glibc; the
    device's library is held to the bar alone): twice (df / 2) (n + 8) eps / (1 - r^2) -- d(r^2) = 2 r dr, and eight roundings
    outside the sums -- and 4 eps M for the exponent lbt of tsfa_betainc, a sum of terms of the sizes M = 4 (a + 8) log(a + 8)
    (two Lanczos log-gammas, each a difference of (x + 1/2) log(x + 15/2) and x + 15/2) and a |log x|, each the product of
    rounded factors."""
    tr = c.truth
    a = 0.5 * tr.df
    x = tr.df / (tr.df + tr.t * tr.t)
    m = 4.0 * (a + 8.0) * math.log(a + 8.0) + a * abs(math.log(x)) + 1.0
    return 2.0 * pc.conditioning_of(c.n, tr.omr2) * (c.n + 8.0) / c.n + 4.0 * pc.EPS * m


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_emulation_owes_the_truth_no_more_than_its_arithmetic(dtype_name):
    """The bar, 1e-6, is what a user needs; the special functions themselves are good for 1e-13.  On the CPU, where log, log1p,
    exp and sin are correctly rounded, the kernel source is held to tight_bound: a Lanczos coefficient off in its tenth digit
    moves a p-value by 1e-10 (measured: profiles/pvalue_floor.md), far below the bar and far above this bound at 3 .. 257
    samples."""
    cases, names, got = _run("emul", "trend", dtype_name)
    jp = _pcol(names)
    worst, small = 0.0, 0
    for i, c in enumerate(cases):
        if c.kind in ("pair", "constant", "underflow"):
            continue
        p, bound = c.truth.p, tight_bound(c)
        ratio = abs(got[i, jp] - p) / p / bound
        assert ratio <= 1.0, (c.label, got[i, jp], p, ratio)
        worst, small = max(worst, ratio), small + (bound < 1e-11)
    print("\nemul %s: largest error / tight bound %.3g; %d cases with a bound below 1e-11" % (dtype_name, worst, small))
    assert small >= 40, small


# ---------------------------------------------------------------------------------------------------------------------
# augmented_dickey_fuller
# ---------------------------------------------------------------------------------------------------------------------
def _adf_groups(cases):
    """{autolag: [(label, series)]}: one plan per lag selection."""
    out = {}
    for label, x, al in cases:
        out.setdefault(al, []).append((label, x))
    return out


def test_the_adf_cases_lie_where_they_are_meant_to_and_the_recorded_truth_is_the_many_digit_one():
    stored = pc.adf_truth()
    fresh = pc.compute_adf_truth()
    assert set(stored) == set(fresh)
    for label, f in fresh.items():
        s = stored[label]
        assert s["usedlag"] == f["usedlag"] and abs(s["teststat"] - f["teststat"]) <= 1e-13 * abs(f["teststat"]), (label, s, f)
    below = 0
    for label, x, al in pc.adf_cases():
        t = stored[label]["teststat"]
        assert 60 <= len(x) <= 400 and stored[label]["ratios_well_defined"] and not stored[label]["perfect"], label
        assert stored[label]["gap"] is None or stored[label]["gap"] > 1e-6, (label, stored[label])      # the lag is the data's
        if "_edge_" not in label:
            assert pc.BAND[0] < t < pc.BAND[1], (label, t)
            assert 1e-30 < pc.adf_pvalue_of(t) < 1e-6, (label, t)
            below += pc.adf_pvalue_of(t) < 1e-9
    assert {al for label, _, al in pc.adf_cases() if "_edge_" not in label} == set(pc.AUTOLAGS)      # every lag selection of the plan
    print("\nADF cells with a true p below 1e-9: %d" % below)
    assert below >= 20, below
    assert len({stored[l]["usedlag"] for l, _, _ in pc.adf_cases()}) >= 5
    # one series on each side of every cut of mackinnon_p_c1
    t = {name: stored["adf_edge_" + name]["teststat"] for name, _ in pc.ADF_EDGES}
    assert t["below_-18.83"] < -18.83 < t["above_-18.83"] < -1.61 and t["below_-1.61"] < -1.61 < t["above_-1.61"] < 2.74 < t["above_2.74"]
    assert pc.adf_pvalue_of(t["below_-18.83"]) == 0.0 and pc.adf_pvalue_of(t["above_2.74"]) == 1.0
    for label, _, _ in pc.adf_dd_cases():
        assert pc.BAND[0] < stored[label]["teststat"] < pc.BAND[1] and stored[label]["ratios_well_defined"], stored[label]


@pytest.mark.parametrize("which", ["oracle", "emul"])
def test_adf_p_values_meet_the_bar(which):
    engine = oracle_engine if which == "oracle" else emul_engine
    worst, bad = {}, []
    for al, group in _adf_groups(pc.adf_cases() + pc.adf_dd_cases()).items():
        from dd_cases import adf_params, pack
        values, offsets = pack([x for _, x in group])
        names, got = engine(adf_params(al), values, offsets)
        bad += pc.compare_adf([l for l, _ in group], names, got, what=which, worst=worst)
    print("\n%s: %d ADF cases, largest error / bar %.3g" % (which, len(worst), max(worst.values())))
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------------------------------
# the gap, written down
# ---------------------------------------------------------------------------------------------------------------------
def test_the_comparator_has_teeth_where_parity_has_none():
    """The emulation's p-values below 1e-9 replaced by 0.0, then those below 1e-49 by 1e40 times themselves (still below the
    floor: a larger one even parity.compare would see): parity.compare, given the same matrices, the reference and the series,
    reports nothing; compare_pvalues / compare_adf report every such cell.  ADF p-values end at 1e-30: 1e10 times those below
    1e-19."""
    cases, names, got = _run("emul", "trend", "float64")
    _, _, want = _run("oracle", "trend", "float64")
    series = [c.x.astype(np.float64) for c in cases]
    jp = _pcol(names)
    before = parity.compare(names, got, want, series)
    assert not before and not pc.compare_pvalues(cases, got[:, jp])
    for below, factor, at_least in ((1e-9, 0.0, 75), (1e-49, 1e40, 40)):
        small = [i for i, c in enumerate(cases) if 0.0 < c.truth.p < below and c.kind != "underflow"]
        assert len(small) >= at_least, len(small)
        spoiled = got.copy()
        spoiled[small, jp] *= factor
        assert np.all(spoiled[small, jp] < 1e-9)
        assert parity.compare(names, spoiled, want, series) == before
        bad = pc.compare_pvalues(cases, spoiled[:, jp])
        assert len(bad) == len(small) and all(cases[i].label in line for i, line in zip(small, bad)), (len(bad), len(small))
    # ... and the ADF column
    from dd_cases import adf_params, pack
    group = _adf_groups(pc.adf_cases())["AIC"]
    labels = [l for l, _ in group]
    values, offsets = pack([x for _, x in group])
    names, got = emul_engine(adf_params("AIC"), values, offsets)
    _, want = oracle_engine(adf_params("AIC"), values, offsets)
    jp = _pcol(names)
    truth_p = [pc.adf_pvalue_of(pc.adf_truth()[l]["teststat"]) for l in labels]
    before = parity.compare(names, got, want, [x for _, x in group])
    assert not pc.compare_adf(labels, names, got)
    for below, factor, at_least in ((1e-9, 0.0, 8), (1e-19, 1e10, 2)):
        small = [i for i, p in enumerate(truth_p) if 0.0 < p < below]
        assert len(small) >= at_least, truth_p
        spoiled = got.copy()
        spoiled[small, jp] *= factor
        assert np.all(spoiled[small, jp] < 1e-9)
        assert parity.compare(names, spoiled, want, [x for _, x in group]) == before
        assert len(pc.compare_adf(labels, names, spoiled)) == len(small)
