"""The double-double passes (k_ar_degenerate: fam_ar_dd.h, k_langevin_dd: fam_langevin_dd.h, on tsfa_dd.h) against
many-digit arithmetic, on the g++ emulation AND on the device -- including the cells tests/parity.py skips against the
float64 reference (R4: the reference inverts round-off, R5: perfect fits), which are compared with nothing else.

The references (tests/adf_mp.py: statsmodels' pinv rule in 120 digits; tests/polyfit_mp.py: np.polyfit's definition in 60)
are computed once per session in tests/dd_cases.py.  The bars are the ones the project applies to the emulation:
    coefficients / teststat   rtol 2e-7, atol 1e-10 max|beta|        (tests/test_degenerate.py, ill-conditioned series)
    usedlag                   equal
    pvalue                    the oracle's MacKinnon function of the many-digit teststat; the bar is how far the teststat's
                              bar moves that function, over parity.py's plain cell tolerance (1e-6 relative, 1e-9)
    friedrich_coefficients    1e-9 + 0.02 eps kappa                     (tests/test_offset.py)
    max_langevin_fixed_point  parity.tolerance_for
A perfect fit (many-digit ssr == 0) follows test_perfect_fit_behaviour_is_pinned: usedlag equal, t is 0/0 or x/0.

Every comparison runs as float64 and, on the device, as float32 for the series float32 holds exactly (the emulation reads
float64 only: its float32 run would be the same run).  Each test prints one line per run: cells compared, series the
well-definedness conditions left out, largest error over its bound."""
import functools
import math

import numpy as np
import pytest

import dd_cases
import parity
from dd_cases import AUTOLAGS, adf_params, adf_reference, adf_well_defined, ar_params, ar_reference, is_float32, pack, \
    ratios_well_defined
from engines import emul_engine

RUNS = [pytest.param(("emul", np.float64), id="emul-float64"),
        pytest.param(("hip", np.float64), id="hip-float64", marks=pytest.mark.gpu),
        pytest.param(("hip", np.float32), id="hip-float32", marks=pytest.mark.gpu)]


@pytest.fixture(params=RUNS)
def run(request):
    """-> (engine(fc_parameters, list of series) -> (names, matrix), dtype)"""
    which, dtype = request.param
    if which == "hip":
        request.getfixturevalue("gpu")
        from engines import hip_engine as engine
    else:
        engine = emul_engine

    def call(fc_parameters, series):
        values, offsets = pack(series)
        values = values.astype(dtype)
        assert np.array_equal(values.astype(np.float64), np.concatenate(series)) or dtype == np.float64
        return engine(fc_parameters, values if which == "hip" else values.astype(np.float64), offsets)
    return call, dtype


class _Tally:
    """Mismatches and the bookkeeping the summary line prints."""

    def __init__(self, what):
        self.what, self.cells, self.worst, self.bad, self.left_out = what, 0, 0.0, [], set()

    def cell(self, label, got, want, bound):
        self.cells += 1
        err = abs(got - want)
        ratio = 0.0 if err == 0 else (err / bound if bound > 0 else math.inf)
        if not ratio <= 1.0:
            self.bad.append("%s: got %r want %r (error / bound %.3g)" % (label, got, want, ratio))
        elif ratio > self.worst:
            self.worst = ratio

    def equal(self, label, got, want):
        self.cells += 1
        if got != want:
            self.bad.append("%s: got %r want %r" % (label, got, want))

    def true(self, label, ok, shown):
        self.cells += 1
        if not ok:
            self.bad.append("%s: %r" % (label, shown))

    def finish(self, n_series, cap=None):
        print("\n[dd passes] %s: %d cells compared, %d of %d series left out, largest error / bound %.3g"
              % (self.what, self.cells, len(self.left_out), n_series, self.worst))
        assert not self.bad, "%d mismatches, first: %s" % (len(self.bad), self.bad[:8])
        if cap is not None:
            assert len(self.left_out) <= cap * n_series, (sorted(self.left_out), n_series)


def _columns(names, needle):
    return [j for j, n in enumerate(names) if needle in n]


def _check_ar(tally, label, names, row, x, k, conditions):
    beta, _, ratios = ar_reference(x, k)
    if conditions and not ratios_well_defined([ratios]):
        tally.left_out.add(label)
        return 0
    amax = float(np.abs(beta).max())
    for c in range(k + 1):
        j = names.index("value__ar_coefficient__coeff_%d__k_%d" % (c, k))
        tally.cell("%s AR(%d) coeff %d" % (label, k, c), row[j], beta[c], 2e-7 * abs(beta[c]) + 1e-10 * amax)
    return k + 1


def _pvalue_bound(t, p):
    from adf_mp import adf_pvalue
    moved = max(abs(adf_pvalue(t * (1 + s * 2e-7)) - p) for s in (-1.0, 1.0))
    return moved + parity.RTOL * abs(p) + 1e-9


def _check_adf(tally, label, names, row, x, autolag, conditions):
    t, p, lag, facts = adf_reference(x, autolag)
    if conditions and not adf_well_defined(facts):
        tally.left_out.add(label)
        return 0
    label = "%s ADF[%s]" % (label, autolag)
    got_t, got_p, got_lag = (row[_columns(names, 'attr_"%s"' % a)[0]] for a in ("teststat", "pvalue", "usedlag"))
    tally.equal(label + " usedlag", got_lag, lag)
    if math.isnan(t) or math.isinf(t):      # a perfect fit: 0 / 0 or x / 0
        tally.true(label + " teststat of a perfect fit", np.isnan(got_t) or np.isinf(got_t), got_t)
        tally.true(label + " pvalue of a perfect fit", np.isnan(got_p) or got_p in (0.0, 1.0), got_p)
    else:
        tally.cell(label + " teststat", got_t, t, 2e-7 * abs(t))
        tally.cell(label + " pvalue", got_p, p, _pvalue_bound(t, p))
    return 3


def _head(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:dd_cases.MAX_LEN])


# ---------------------------------------------------------------------------------------------------------------------
# a. full-rank, ill-conditioned designs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ill_conditioned_batch():
    """-> (batch, positions of the 18 listed series in it): the listed series spread among 200 ordinary noise series of
    ragged length, so that they reach the second pass through the list the first pass fills with atomics."""
    from test_offset import offset_fuzz_series
    listed = [_head(x) for x in dd_cases.ill_conditioned_series() + offset_fuzz_series(20260924)[:12]]
    rng = np.random.default_rng(20261017)
    noise = [rng.standard_normal(int(n)).astype(np.float32).astype(np.float64) for n in rng.integers(30, 400, size=200)]
    batch, where = [], []
    for i, x in enumerate(noise):
        if i % 11 == 0 and len(where) < len(listed):
            where.append(len(batch))
            batch.append(listed[len(where) - 1])
        batch.append(x)
    assert len(where) == len(listed) == 18
    return batch, where


def test_ill_conditioned_designs_match_many_digit_arithmetic(run):
    call, dtype = run
    batch, where = _ill_conditioned_batch()
    if dtype == np.float32:
        keep = [i for i, x in enumerate(batch) if is_float32(x)]
        where = [keep.index(w) for w in where if w in keep]
        batch = [batch[i] for i in keep]
        assert len(where) >= 4
    tally = _Tally("ill-conditioned, %s" % np.dtype(dtype).name)
    for autolag in AUTOLAGS:
        params = dict(ar_params(10), **adf_params(autolag))
        names, got = call(params, batch)
        _, again = call(params, batch)
        assert np.array_equal(got, again, equal_nan=True), "two runs of one batch differ in their bits"
        for w in where:
            label = "series %d (%d samples)" % (w, len(batch[w]))
            if autolag == "AIC":
                _check_ar(tally, label, names, got[w], batch[w], 10, conditions=False)
            _check_adf(tally, label, names, got[w], batch[w], autolag, conditions=False)
    tally.finish(len(where))


# ---------------------------------------------------------------------------------------------------------------------
# b. exactly rank-deficient designs
# ---------------------------------------------------------------------------------------------------------------------
CONSTANTS = [(0.1, 50), (3.0, 100), (-1.7, 64), (250.0, 300), (0.5, 30), (-2.0, 77), (0.1, 1000), (1e-3, 200)]


@functools.lru_cache(maxsize=None)
def _rank_deficient_series():
    """-> {AR order: [series]} (the ADF regressions do not depend on the order).  np.full(1000, 0.1) is the one series beyond
    400 samples: its 11 AR cells are all skipped by R4 and its many-digit reference costs a second."""
    rng = np.random.default_rng(12)
    t = np.arange(400.0)
    k10 = [np.full(n, c) for c, n in CONSTANTS]
    k10 += [0.25 + 0.125 * t[:120], 5.0 - 0.5 * t[:100], t[:64], -2.0 + 0.25 * t[:333]]
    k10 += [np.resize(p, n) for p, n in (([1.0, -1.0], 80), ([3.0, 1.0], 61), ([1.0, -2.0, 0.5], 150), ([1.0, 2.0, 4.0], 200),
                                         ([0.0, 1.0, 0.0, -1.0], 120), ([2.0, -1.0, 0.0, 1.0], 97))]
    out = {4: [], 10: k10, 16: []}
    for k in (4, 10, 16):      # k + 1 noisy samples, then a stuck level (tests/test_ar_stuck.py: _low_order_batches)
        for i in range(6):
            n = int(rng.integers(2 * k + 6, 400))
            head = rng.standard_normal(k + 1) * [1.0, 1e-3, 50.0][i % 3]
            if i % 2:
                head = head.astype(np.float32).astype(np.float64)
            lvl = [head[-1], 0.0, 3.25, -1e4, head[-1], 3.25][i]
            out[k].append(np.concatenate([head, np.full(n - k - 1, lvl)]))
    assert sum(len(v) for v in out.values()) <= 40
    return out


def test_rank_deficient_designs_match_many_digit_arithmetic(run):
    call, dtype = run
    tally = _Tally("rank-deficient, %s" % np.dtype(dtype).name)
    n_series = 0
    for k, series in _rank_deficient_series().items():
        series = [x for x in series if dtype == np.float64 or is_float32(x)]
        n_series += len(series)
        for autolag in AUTOLAGS:
            names, got = call(dict(ar_params(k), **adf_params(autolag)), series)
            for i, x in enumerate(series):
                label = "AR order %d series %d (%d samples, first %r last %r)" % (k, i, len(x), x[0], x[-1])
                if autolag == "AIC":
                    _check_ar(tally, label, names, got[i], x, k, conditions=True)
                    if np.ptp(x) == 0 and k == 10:
                        c = x[0]    # the design [1, c, ..., c] has rank 1: b0 + c sum(b_i) = c, minimum norm
                        want = c / (1 + 10 * c * c) * np.array([1.0] + [c] * 10)
                        ours = np.array([got[i, names.index("value__ar_coefficient__coeff_%d__k_10" % j)] for j in range(11)])
                        assert np.allclose(ours, want, rtol=1e-12, atol=0), (c, ours, want)
                _check_adf(tally, label, names, got[i], x, autolag, conditions=True)
    assert n_series >= (20 if dtype == np.float32 else 36)
    tally.finish(n_series, cap=0.10)


# ---------------------------------------------------------------------------------------------------------------------
# c. perfect fits and the exact lag search
# ---------------------------------------------------------------------------------------------------------------------
def test_perfect_fit_behaviour_is_pinned(run):
    """tests/test_degenerate.py's test of the same name, on every engine."""
    call, dtype = run
    for x, want_lag in dd_cases.perfect_fit_series():
        assert is_float32(x)
        names, got = call(adf_params("AIC"), [x])
        row = dict(zip([n.split('attr_"')[1].split('"')[0] for n in names], got[0]))
        assert row["usedlag"] == want_lag, (row, want_lag)
        assert np.isnan(row["teststat"]) or np.isinf(row["teststat"]), row
        assert all(parity.excluded(n, x) for n in names)


def test_near_degenerate_lag_search_agrees_with_exact_arithmetic(run):
    """tiny_noise_ramp_300 (cond 5e11; float64 only: float32 does not hold it): exact rational arithmetic selects lag 12."""
    call, dtype = run
    x, exact_lag = dd_cases.tiny_noise_ramp()
    if dtype == np.float32:
        assert not is_float32(x)
        return
    names, got = call({"augmented_dickey_fuller": [{"attr": "usedlag", "autolag": "AIC"}]}, [x])
    assert got[0, 0] == exact_lag == 12
    assert parity.excluded(names[0], x)


# ---------------------------------------------------------------------------------------------------------------------
# d. the Langevin second pass
# ---------------------------------------------------------------------------------------------------------------------
LANGEVIN = {"friedrich_coefficients": [{"coeff": c, "m": 3, "r": 30} for c in range(4)],
            "max_langevin_fixed_point": [{"m": 3, "r": 30}]}


@functools.lru_cache(maxsize=None)
def _largest_root(coef):
    """fc.py:2134, max(real(roots)) of the many-digit cubic, in 60 digits."""
    import mpmath as mp
    with mp.workdps(60):
        c = [mp.mpf(v) for v in coef]
        while c and c[0] == 0:
            c = c[1:]
        return float(max(mp.re(r) for r in mp.polyroots(c, maxsteps=500, extraprec=400)))


def test_langevin_second_pass_agrees_with_60_digit_arithmetic(run):
    call, dtype = run
    series, want = dd_cases.langevin_second_pass_cases()
    assert len(series) >= 10 and {w[2] for w in want} >= {2, 3, 4}     # full rank and both truncated ranks occur
    if dtype == np.float32:      # offset + noise: float32 holds none of them
        assert not any(is_float32(x) for x in series)
        return
    names, got = call(LANGEVIN, series)
    tally = _Tally("langevin, %s" % np.dtype(dtype).name)
    cj = [names.index("value__friedrich_coefficients__coeff_%d__m_3__r_30" % c) for c in range(4)]
    rj = names.index("value__max_langevin_fixed_point__m_3__r_30")
    for i, (x, (coef, kappa, rank)) in enumerate(zip(series, want)):
        label = "series %d (mean %.3g, rank %d)" % (i, x.mean(), rank)
        for c in range(4):
            tally.cell("%s coefficient %d" % (label, c), got[i, cj[c]], coef[c], (1e-9 + 0.02 * parity.EPS * kappa) * abs(coef[c]))
        root = _largest_root(tuple(float(v) for v in coef))
        rt, at = parity.tolerance_for(names[rj], x, root, parity._SeriesFacts(x))
        tally.cell(label + " fixed point", got[i, rj], root, rt * abs(root) + at)
    tally.finish(len(series))


# ---------------------------------------------------------------------------------------------------------------------
# e. the cells the parity exclusions skip in the existing GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _skipped_cells(series, names):
    """[(series index, column)] that tests/parity.py excludes (the predicates read the series only)."""
    out = []
    for i, x in enumerate(series):
        facts = parity._SeriesFacts(x)
        out += [(i, n) for n in names if parity.excluded(n, x, facts=facts)]
    return out


def _check_formerly_skipped(tally, cells, series, names, got, k, autolag):
    compared = 0
    for i in sorted({i for i, _ in cells}):
        cols = [n for j, n in cells if j == i]
        label = "series %d (%d samples)" % (i, len(series[i]))
        if any("ar_coefficient" in n for n in cols):
            assert sum("ar_coefficient" in n for n in cols) == k + 1      # R4 reads the design: all of them or none
            compared += _check_ar(tally, label, names, got[i], series[i], k, conditions=True)
        adf = [n for n in cols if "augmented_dickey_fuller" in n]
        if adf:
            assert len(adf) == 3
            compared += _check_adf(tally, label, names, got[i], series[i], autolag, conditions=True)
    return compared


@functools.lru_cache(maxsize=None)
def _degenerate_adf_set():
    import os
    from test_adf_autolag import FILES, G
    g = np.load(os.path.join(G, FILES["degenerate"]))
    v, o = g["values"], g["offsets"]
    return [_head(v[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def test_skipped_cells_of_the_degenerate_adf_set_match_many_digit_arithmetic(run):
    """tests/test_adf_autolag.py allows 55 % of this set's cells to be skipped; here they are compared."""
    from test_adf_autolag import MODES
    call, dtype = run
    series = _degenerate_adf_set()
    if dtype == np.float32:
        series = [x for x in series if is_float32(x)]
        assert len(series) >= 10
    tally = _Tally("degenerate ADF set, %s" % np.dtype(dtype).name)
    total = compared = 0
    for autolag in MODES:
        names, got = call(adf_params(autolag), series)
        cells = _skipped_cells(series, names)
        total += len(cells)
        compared += _check_formerly_skipped(tally, cells, series, names, got, None, autolag)
    print("\n[dd passes] %d of %d formerly skipped cells compared" % (compared, total))
    assert total >= 0.3 * 9 * len(series) and compared >= 0.8 * total, (compared, total)
    tally.finish(len(series), cap=0.10)


@functools.lru_cache(maxsize=None)
def _stuck_sensor_batch(dtype):
    """tests/test_gpu_parity.py: test_hip_second_pass_handles_a_batch_of_stuck_sensors draws 600 series; the first 40 of them
    that hold a skipped AR / ADF cell are compared here (a many-digit reference per series)."""
    rng = np.random.default_rng(3)
    lens = rng.integers(30, 400, size=600)
    names = ["value__ar_coefficient__coeff_%d__k_10" % c for c in range(11)] + \
            ['value__augmented_dickey_fuller__attr_"%s"__autolag_"AIC"' % a for a in ("teststat", "pvalue", "usedlag")]
    chosen = []
    for i, n in enumerate(lens):
        kind = i % 4
        if kind == 0:
            x = np.full(n, float(rng.integers(-3, 4)) * 0.5)
        elif kind == 1 and dtype == np.float64:
            x = float(rng.integers(-8, 9)) * 0.25 + float(rng.integers(-4, 5)) * 0.125 * np.arange(n)
        elif kind == 2:
            x = np.resize(rng.integers(-2, 3, int(rng.integers(2, 5))).astype(float), n)
        else:
            x = rng.standard_normal(n)
        x = x.astype(dtype).astype(np.float64)
        if len(chosen) < 40 and kind != 3 and any(parity.excluded(c, x) for c in (names[0], names[-1])):
            chosen.append(x)
    assert len(chosen) == 40
    return chosen


@pytest.mark.parametrize("drawn_as", [np.float32, np.float64], ids=["drawn-float32", "drawn-float64"])
def test_skipped_cells_of_the_stuck_sensor_batch_match_many_digit_arithmetic(run, drawn_as):
    """The batch allows 17.8 % (float32) / 24.5 % (float64, which adds exact ramps) of its cells to be skipped."""
    call, dtype = run
    series = _stuck_sensor_batch(drawn_as)
    if dtype == np.float32:
        series = [x for x in series if is_float32(x)]
        assert len(series) >= 20
    tally = _Tally("stuck-sensor batch drawn as %s, %s" % (np.dtype(drawn_as).name, np.dtype(dtype).name))
    names, got = call(dict(ar_params(10), **adf_params("AIC")), series)
    cells = _skipped_cells(series, names)
    compared = _check_formerly_skipped(tally, cells, series, names, got, 10, "AIC")
    print("\n[dd passes] %d of %d formerly skipped cells compared" % (compared, len(cells)))
    assert len(cells) >= 3 * len(series) and compared >= 0.8 * len(cells), (compared, len(cells))
    tally.finish(len(series), cap=0.10)
