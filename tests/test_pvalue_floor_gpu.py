"""`-m gpu`: the p-value columns below tests/parity.py's 1e-9 floor on the device, RELATIVE to the true p-value (the twin of
tests/test_pvalue_floor.py; cases, truth and bar: tests/pvalue_cases.py).  On the device the incomplete beta function and
MacKinnon's normal tail run on the GPU math library's log, log1p, exp, sin and erfc: the CPU emulation cannot speak for those.

One test per route that evaluates a p-value, each one ragged batch of the cases AND of their negatives (p of x and of -x meet
the same bar), each with the route read from the launch record (Plan.last_launches):
    k_trend_rows        series of at most 256 samples, four to a wavefront
    the wavefront form  the same series with the plan option row_form 0.  The launch record does not name the form: that the
                        option changed the route is shown by the two matrices differing in their bits (other reduction trees)
    k_trend             257 .. 2049 samples, the LDS build
    the long build      the first length past the TREND family's crossover (route_cases.LAST_IN_LDS), and 65 536 samples
    blk_linregress_xy   linear_trend_timewise with times=
    k_ar                the ADF p-value (mackinnon_p_c1), every lag selection
    k_ar_degenerate     the ADF p-value of two stuck-sensor series, written by the double-double pass.  The record shows the
                        family's launch, not which series the first pass listed: that these are listed was shown once, on the
                        emulation (pvalue_cases.adf_dd_cases)
The truth is 2 * scipy.special.stdtr(df, -|t|) of the exactly summed regression (the CPU test pins it to many-digit
arithmetic), and the recorded many-digit ADF statistics: no mpmath runs here."""
import time

import numpy as np
import pytest

import parity
import pvalue_cases as pc
import route_cases as rc
from engines import hip_engine, oracle_engine

pytestmark = pytest.mark.gpu
DTYPES = pc.DTYPES
ROW_MAXN = 256      # TSFA_ROW_MAXN, tsfa_common.h
_memo = {}


def _pcol(names):
    js = [j for j, n in enumerate(names) if pc.is_pvalue(n)]
    assert len(js) == 1, names
    return js[0]


def _extract(cases, params, options=None):
    """-> (names, rows of the cases, rows of their negatives, launch records) of ONE extract."""
    values, offsets, times = pc.pack(cases)
    neg, _, _ = pc.pack(cases, negate=True)
    both_off = np.concatenate([offsets, offsets[-1] + offsets[1:]])
    both_times = None if times is None else np.concatenate([times, times])
    records = []
    names, got = hip_engine(params, np.concatenate([values, neg]), both_off, times=both_times, options=options, launches=records)
    assert got.shape[0] == 2 * len(cases)
    return names, got[:len(cases)], got[len(cases):], records


def _hold(cases, names, got_x, got_neg, what, params=None):
    """The bar on x and on -x, every p in [0, 1], and the other columns of x the way every other test compares them."""
    jp = _pcol(names)
    worst = {}
    bad = pc.compare_pvalues(cases, got_x[:, jp], what=what, worst=worst)
    bad += pc.compare_pvalues(cases, got_neg[:, jp], what=what + " of -x", worst=worst)
    print("\n%s: %d cases, largest relative error per length: %s" % (what, len(cases), {n: "%.2g" % v for n, v in sorted(worst.items())}))
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    for g in (got_x[:, jp], got_neg[:, jp]):
        assert np.all((g >= 0.0) & (g <= 1.0)), g[~((g >= 0.0) & (g <= 1.0))]
    if params is not None:
        values, offsets, times = pc.pack(cases)
        onames, want = oracle_engine(params, values.astype(np.float64), offsets, times=times)
        cols = [names.index(n) for n in onames]
        bad = parity.compare(onames, got_x[:, cols], want, [c.x.astype(np.float64) for c in cases])
        assert not bad, bad[:8]


def _trend_record(records, max_len, long_build):
    assert {r["family"] for r in records} == {"TREND"}, records
    rec = rc.record_of(records, "TREND")
    assert (rec["max_len"], rec["long_build"], rec["length_class"]) == (max_len, long_build, 0), rec
    return rec


def _short_cases(dtype_name):
    cases = pc.trend_cases(dtype_name, pc.SHORT_LENGTHS) + [c for c in pc.edge_cases(dtype_name) if c.n <= ROW_MAXN]
    assert max(c.n for c in cases) == ROW_MAXN and {c.kind for c in cases} == {"grid", "cap", "underflow", "pair", "constant"}
    return cases + pc.exact_lines(dtype_name)


def _short(dtype_name, form):
    key = (dtype_name, form)
    if key not in _memo:
        _memo[key] = _extract(_short_cases(dtype_name), pc.TREND_PARAMS, options=None if form == "rows" else {"row_form": 0})
    return _memo[key]


def _check_lines(cases, names, got_x, got_neg):
    """The exact lines: r = +-1 exactly, and the p-value the reference returns for it (1e-6 relative, no floor)."""
    lines = [i for i, c in enumerate(cases) if c.kind == "line"]
    assert len(lines) == 6
    values, offsets, _ = pc.pack([cases[i] for i in lines])
    onames, want = oracle_engine(pc.TREND_PARAMS, values.astype(np.float64), offsets)
    assert onames == names
    jp, jr = _pcol(names), names.index('value__linear_trend__attr_"rvalue"')
    for k, i in enumerate(lines):
        assert abs(want[k, jr]) == 1.0 and got_x[i, jr] == want[k, jr] and got_neg[i, jr] == -want[k, jr], (cases[i].label, got_x[i, jr])
        for g in (got_x[i, jp], got_neg[i, jp]):
            assert abs(g - want[k, jp]) <= pc.RTOL * want[k, jp], (cases[i].label, g, want[k, jp])


@pytest.mark.parametrize("form", ["rows", "waves"])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_short_series_in_the_row_form_and_in_the_wavefront_form(gpu, dtype_name, form):
    t0 = time.perf_counter()
    cases = _short_cases(dtype_name)
    names, got_x, got_neg, records = _short(dtype_name, form)
    rec = _trend_record(records, ROW_MAXN, 0)
    assert rec["n_series"] == 2 * len(cases), rec
    graded = [i for i, c in enumerate(cases) if c.kind != "line"]
    _hold([cases[i] for i in graded], names, got_x[graded], got_neg[graded], "%s %s" % (form, dtype_name), params=pc.TREND_PARAMS)
    _check_lines(cases, names, got_x, got_neg)
    # the option chose another route: same inputs, same kernels' arithmetic, other reduction trees -- other bits somewhere
    _, other_x, _, _ = _short(dtype_name, "waves" if form == "rows" else "rows")
    assert not np.array_equal(got_x, other_x, equal_nan=True), "row_form 0 and 1 returned the same bits: one route ran twice"
    jp = _pcol(names)
    assert np.allclose(got_x[graded][:, jp], other_x[graded][:, jp], rtol=2 * pc.RTOL, atol=0)
    print("%.1f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_k_trend_on_257_to_2049_samples(gpu, dtype_name):
    cases = pc.trend_cases(dtype_name, pc.MID_LENGTHS) + [c for c in pc.edge_cases(dtype_name) if c.n > ROW_MAXN]
    assert min(c.n for c in cases) == 257 and max(c.n for c in cases) == 2049 and any(c.kind == "underflow" for c in cases)
    names, got_x, got_neg, records = _extract(cases, pc.TREND_PARAMS)
    rec = _trend_record(records, 2049, 0)
    assert rec["lds_bytes"] <= 160 * 1024, rec
    _hold(cases, names, got_x, got_neg, "k_trend %s" % dtype_name, params=pc.TREND_PARAMS)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_long_build_past_the_crossover_and_at_65536_samples(gpu, dtype_name):
    """Comprehensive's TREND calculators (route_cases.family_params: the plan LAST_IN_LDS["TREND"] was read for), whose
    linear_trend holds all five attributes.  Two extracts: the crossover length with shorter series riding in its launch, and
    the 65 536-sample cases."""
    t0 = time.perf_counter()
    params = rc.family_params("TREND")
    assert sorted(p["attr"] for p in params["linear_trend"]) == sorted(p["attr"] for p in pc.TREND_PARAMS["linear_trend"])
    dt = np.dtype(dtype_name)
    # just past: one sample fewer is the LDS build
    records = []
    hip_engine(params, rc.series_at(pc.CROSS - 1, "iid", 2).astype(dt), np.array([0, pc.CROSS - 1], dtype=np.int64), launches=records)
    _trend_record(records, pc.CROSS - 1, 0)
    riders = [c for c in pc.trend_cases(dtype_name, (65, 1025)) if "p1e-30" in c.label or "t2" in c.label]
    for cases in (pc.trend_cases(dtype_name, (pc.CROSS,)) + riders, pc.trend_cases(dtype_name, (pc.LONGEST,))):
        longest = max(c.n for c in cases)
        names, got_x, got_neg, records = _extract(cases, params)
        rec = _trend_record(records, longest, 1)
        assert rec["threads"] == 256, rec
        _hold(cases, names, got_x, got_neg, "long build at %d, %s" % (longest, dtype_name))
    print("%.1f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_linear_trend_timewise_with_time_stamps(gpu, dtype_name):
    cases = pc.timewise_cases(dtype_name)
    assert sum(0.0 < c.truth.p < 1e-9 for c in cases) >= 30 and {c.n <= ROW_MAXN for c in cases} == {True, False}
    names, got_x, got_neg, records = _extract(cases, pc.TIMEWISE_PARAMS)
    _trend_record(records, 1025, 0)
    _hold(cases, names, got_x, got_neg, "timewise %s" % dtype_name, params=pc.TIMEWISE_PARAMS)


def _adf(cases, dtype_name, pad=()):
    """compare_adf on every lag selection's batch of x and of -x (the statistic does not change with the sign); pad: series
    that ride along uncompared.  -> number of cells compared."""
    from dd_cases import adf_params
    groups, bad, worst, compared = {}, [], {}, 0
    for label, x, al in cases:
        groups.setdefault(al, []).append((label, x))
    for al, group in groups.items():
        labels = [l for l, _ in group]
        series = [x for _, x in group]
        batch = series + [-x for x in series] + list(pad)
        values = np.concatenate(batch).astype(np.dtype(dtype_name))
        assert np.array_equal(values.astype(np.float64), np.concatenate(batch))      # the dtype holds the series
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in batch])]).astype(np.int64)
        records = []
        names, got = hip_engine(adf_params(al), values, offsets, launches=records)
        assert {r["family"] for r in records} == {"AR"}, records
        rec = rc.record_of(records, "AR")
        assert (rec["n_series"], rec["max_len"], rec["long_build"]) == (len(batch), max(len(x) for x in batch), 0), rec
        k = len(series)
        compared += k
        bad += pc.compare_adf(labels, names, got[:k], what="hip", worst=worst)
        bad += pc.compare_adf(labels, names, got[k:2 * k], what="hip of -x", worst=worst)
        jp = _pcol(names)
        assert np.all((got[:2 * k, jp] >= 0.0) & (got[:2 * k, jp] <= 1.0)), got[:2 * k, jp]
    print("\nADF %s: %d cases, largest error / bar %.3g" % (dtype_name, compared, max(worst.values())))
    assert not bad, bad[:8]
    return compared


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_k_ar_adf_p_values(gpu, dtype_name):
    assert _adf(pc.adf_cases(), dtype_name) == len(pc.adf_cases())


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_double_double_pass_writes_adf_p_values_in_the_band(gpu, dtype_name):
    """The stuck-sensor series among 24 ordinary ones, so that they reach the second pass through the list the first pass fills
    (tests/test_dd_passes_gpu.py: _ill_conditioned_batch)."""
    pad = [pc.adf_series(k, n, 50 + k) for k in range(3) for n in (60, 90, 150, 200, 250, 300, 350, 400)]
    assert _adf(pc.adf_dd_cases(), dtype_name, pad=tuple(pad)) == 4
