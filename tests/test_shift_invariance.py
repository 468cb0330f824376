"""Level-invariant columns against the SPREAD of offset series (tests/shift_cases.py), on the CPU: the oracle and the g++
build of the kernel sources.  The `-m gpu` twin is tests/test_shift_invariance_gpu.py.

What tests/parity.py cannot see: its absolute floor, 1e-9 max|x| ** dimension, is 1e3 .. 1e10 times the true variance, slope
or spectral density of a series at a level of 1e5 .. 1e9 (test_the_comparator_has_teeth_where_parity_has_none writes the
gap down).  Here the series are exact shifts x = c + b of a base on a dyadic grid, the truth of an invariant column is the
oracle's value on b, and the bound is parity.py's rule with ptp(b) in the place of max|x|.

change_quantiles(f_agg="var") of a jittered sawtooth (truth: exact rational arithmetic; bound: 1e-6 relative, no floor).
Worst relative error of the emulated kernel over the sawtooth series (300, 1000 and 8197 samples), with the one-pass sums
alone (before TSFA_CQ_REFINE, fam_sort.h: 36 of their 156 cells fail) and with the refinement (none fails):
    j = 1e-2: 3.4e-14 / 3.4e-14    j = 1e-4: 5.4e-10 / 5.4e-10    j = 1e-6: 1.4e-5 / 3.4e-15    j = 1e-8: 7.3e-2 / 2.8e-15
and over the zig-zag series (the absolute half of the refinement alone; 12 of their 48 cells fail before, none after):
    j = 1e-6: 3.7e-2 / 3.1e-15    j = 1e-8: 1.7e+2 / 8.1e-14          (the reference's np.var: <= 3.1e-16 on all of them)"""
import numpy as np
import pytest

import parity
import shift_cases as sc
from engines import emul_engine, oracle_engine_parallel

DTYPES = ("float64", "float32")
_memo = {}


def _cases(dtype_name):
    if ("cases", dtype_name) not in _memo:
        _memo["cases", dtype_name] = sc.cases(dtype_name)
    return _memo["cases", dtype_name]


def _truth(dtype_name):
    # (both dtypes at once: one pool of workers, and the long bases are shared)
    if "truth" not in _memo:
        every = [c for d in DTYPES for c in _cases(d)]
        names, rows = sc.truth_of(every)
        _memo["truth"] = (names, {d: rows[[i for i, c in enumerate(every) if c.dtype_name == d]] for d in DTYPES})
    names, by = _memo["truth"]
    return names, by[dtype_name]


def _reference_on_x(dtype_name):
    """oracle(params, x): the reference's own arithmetic on the shifted data."""
    if "ref" not in _memo:
        every = [c for d in DTYPES for c in _cases(d)]
        values, offsets = sc.pack([c.x for c in every])
        names, rows = oracle_engine_parallel(sc.params(), values, offsets)
        _memo["ref"] = (names, {d: rows[[i for i, c in enumerate(every) if c.dtype_name == d]] for d in DTYPES})
    names, by = _memo["ref"]
    return names, by[dtype_name]


def _emulated_on_x(dtype_name):
    if ("emul", dtype_name) not in _memo:
        values, offsets = sc.pack([c.x for c in _cases(dtype_name)])     # float32 samples widened: the emulation reads float64
        _memo["emul", dtype_name] = emul_engine(sc.params(), values, offsets)
    return _memo["emul", dtype_name]


def test_the_cases_cover_what_they_are_meant_to():
    for d in DTYPES:
        cs = _cases(d)
        assert {c.n for c in cs} == set(sc.SHORT_LENGTHS + sc.LONG_LENGTHS)
        assert {c.level for c in cs} == set(sc.TIER_A_LEVELS[d])
        assert {c.kind for c in cs if c.n in sc.SHORT_LENGTHS} == set(sc.BASES)
        assert sum(c.n > 2048 for c in cs) == len(sc.LONG_LENGTHS)      # one base and one level per long length
        for c in cs:
            assert np.ptp(c.b) > 0 and abs(c.level) >= 16 * np.ptp(c.b)
    names, _ = _truth("float64")
    tiers = {t: {parity.feature_of(n) for n in names if sc.tier_of(n) == t} for t in ("A", "B")}
    assert tiers["A"] | tiers["B"] == set(sc.INVARIANT), set(sc.INVARIANT) - tiers["A"] - tiers["B"]
    # no intercept, no bin 0 and nothing test_offset.py owns
    inv = [n for n in names if sc.tier_of(n)]
    assert not [n for n in inv if "intercept" in n or "coeff_0__" in n or n.endswith("coeff_0")]
    assert not {parity.feature_of(n) for n in inv} & {"ar_coefficient", "augmented_dickey_fuller", "friedrich_coefficients",
                                                      "max_langevin_fixed_point"}
    assert 500 <= len(inv) <= len(names), len(inv)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_reference_on_the_shifted_series_holds_a_quarter_of_the_bound(dtype_name):
    """The condition on the inputs: where the reference's own float64 arithmetic on x leaves 1/4 of shift_bound, the bound
    would ask more of the kernels than the reference delivers -- such a column belongs to a lower tier (shift_cases.INVARIANT),
    never to a wider bound."""
    cs = _cases(dtype_name)
    names, truth = _truth(dtype_name)
    rnames, ref = _reference_on_x(dtype_name)
    assert rnames == names
    skipped = []
    bad = sc.compare_shift(names, ref, truth, cs, share=0.25, skipped=skipped, what="oracle")
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    cells = sc.n_invariant_cells(names, cs)
    assert len(skipped) <= 0.02 * cells, (len(skipped), cells)
    assert not [col for _, col in skipped if parity.feature_of(col) in sc.MOMENTS], skipped[:8]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_truth_is_the_definition_in_50_digits_on_the_shifted_series(dtype_name):
    """oracle(b) == mpmath(x) to 1e-12 relative at n = 61 and 300, every base and every level of the dtype: the truth the
    other tests use is not the oracle agreeing with itself."""
    import shift_mp
    cs = _cases(dtype_name)
    names, truth = _truth(dtype_name)
    col = {n: j for j, n in enumerate(names)}
    checked = 0
    for i, c in enumerate(cs):
        if c.n not in (61, 300):
            continue
        want = shift_mp.core_columns(c.x.astype(np.float64))
        assert len(want) == 2 + 2 + 9 + 2 + 1 + 3 + 15 and set(want) <= set(col), set(want) - set(col)
        for name, w in want.items():
            g = truth[i, col[name]]
            scale = abs(w)
            assert abs(g - w) <= 1e-12 * scale, (c.label, name, g, float(w), float(abs(g - w) / scale))
            checked += 1
    assert checked == 34 * 2 * len(sc.BASES) * len(sc.TIER_A_LEVELS[dtype_name])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_the_emulated_kernels_hold_the_bound_on_the_shifted_series(dtype_name):
    cs = _cases(dtype_name)
    names, truth = _truth(dtype_name)
    gnames, got = _emulated_on_x(dtype_name)
    assert gnames == names
    skipped = []
    bad = sc.compare_shift(names, got, truth, cs, skipped=skipped, what="emul")
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    assert len(skipped) <= 0.02 * sc.n_invariant_cells(names, cs)
    assert not [col for _, col in skipped if parity.feature_of(col) in sc.MOMENTS], skipped[:8]


def test_the_comparator_has_teeth_where_parity_has_none():
    """1e-5 relative on the emulated `variance` and on one change_quantiles var cell of the iid series at -3 * 2^17: ten
    times the project's bar.  compare_shift reports both cells; parity.compare, given the same matrices and the shifted
    series, reports neither -- its floor for them is 1e-9 * 393 216^2 = 155, the values are ~1."""
    cs = _cases("float64")
    names, truth = _truth("float64")
    _, got = _emulated_on_x("float64")
    i = [k for k, c in enumerate(cs) if (c.kind, c.n, c.level) == ("iid", 1000, -3.0 * 2 ** 17)][0]
    cols = ["value__variance", 'value__change_quantiles__f_agg_"var"__isabs_False__qh_0.8__ql_0.2']
    js = [names.index(c) for c in cols]
    spoiled = got[i:i + 1].copy()
    for j in js:
        assert abs(truth[i, j]) > 0.1
        spoiled[0, j] *= 1.0 + 1e-5
    bad = sc.compare_shift(names, spoiled, truth[i:i + 1], [cs[i]])
    assert len(bad) == 2 and all(c in line for c, line in zip(cols, sorted(bad, key=lambda s: "variance" not in s))), bad
    # the gap, written down: the same matrices through the comparator every other parity test uses
    x = cs[i].x.astype(np.float64)
    assert parity.compare(names, spoiled, truth[i:i + 1], [x]) == parity.compare(names, got[i:i + 1], truth[i:i + 1], [x])
    for j in js:
        assert parity.atol_for(names[j], x) > 100.0 * abs(truth[i, j])
        sub = [names[j]]
        assert not parity.compare(sub, spoiled[:, [j]], truth[i:i + 1, [j]], [x])
        assert not parity.compare(sub, 1e2 * spoiled[:, [j]], truth[i:i + 1, [j]], [x])     # ... a hundred times too large


# ---- change_quantiles of the jittered sawtooth
def _saw():
    if "saw" not in _memo:
        cases = sc.sawtooth_cases()
        values, offsets = sc.pack([x for _, x in cases])
        names, ref = oracle_engine_parallel(sc.SAW_PARAMS, values, offsets)
        truth = np.array([sc.sawtooth_truth(x, names) for _, x in cases])
        _memo["saw"] = ([label for label, _ in cases], values, offsets, names, truth, ref)
    return _memo["saw"]


def test_sawtooth_truths_are_small_and_the_reference_holds_1e_9():
    labels, _, _, names, truth, ref = _saw()
    var = [k for k, n in enumerate(names) if 'f_agg_"var"' in n]
    assert len(var) == 6 and len(names) == 12 and len(labels) == 13 + 4
    saw = [i for i, label in enumerate(labels) if label.startswith("saw")]
    small = truth[saw][:, var]
    assert len(saw) == 13 and 1e-17 < small.min() < 1e-15 and small.max() < 1e-3, (small.min(), small.max())
    # the zig-zag tells the two halves of the refinement apart: the signed variances are large, the absolute ones j^2-small
    zig = [i for i, label in enumerate(labels) if label.startswith("zig")]
    signed = [k for k in var if "isabs_False" in names[k]]
    absolute = [k for k in var if "isabs_True" in names[k]]
    assert truth[zig][:, signed].min() > 1e-3 and 0 < truth[zig][:, absolute].min() and truth[zig][:, absolute].max() < 1e-13
    bad = sc.compare_sawtooth(names, ref, truth, labels, rtol=1e-9, what="oracle")
    assert not bad, bad[:8]


def test_emulated_change_quantiles_of_a_jittered_sawtooth():
    """Fails with the one-pass sums alone at j <= 1e-6 (module docstring); every corridor of the small-jitter series asks for
    the second sweep, and the shift to 2^20 changes no column beyond the bound."""
    import emul_lib
    labels, values, offsets, names, truth, _ = _saw()
    emul_lib.cq_refined()
    gnames, got = emul_engine(sc.SAW_PARAMS, values, offsets)
    swept = emul_lib.cq_refined()
    assert gnames == names
    worst = {}
    bad = sc.compare_sawtooth(names, got, truth, labels, worst=worst, what="emul")
    print("\nworst relative error per series:", {k: "%.2g" % v for k, v in worst.items()})
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    assert swept >= 3 * sum("j1e-06" in l or "j1e-08" in l for l in labels), swept
    # the zig-zag alone: its three corridors ask once each, for the absolute half (the signed variances are 0.002)
    zig = [i for i, label in enumerate(labels) if label.startswith("zig")]
    zv, zo = sc.pack([values[offsets[i]:offsets[i + 1]] for i in zig])
    emul_lib.cq_refined()
    emul_engine(sc.SAW_PARAMS, zv, zo)
    assert emul_lib.cq_refined() == 3 * len(zig)


def test_noise_never_asks_for_the_second_sweep():
    """The refinement must cost the headline workload nothing: 64 iid-normal series of 1024 samples (float32 values, as
    bench.py draws them), every change_quantiles column of ComprehensiveFCParameters -- not one corridor swept twice."""
    import emul_lib
    rng = np.random.default_rng(20261019)
    x = rng.standard_normal((64, 1024), dtype=np.float32).astype(np.float64)
    params = {"change_quantiles": sc.params()["change_quantiles"]}
    emul_lib.cq_refined()
    names, got = emul_engine(params, x.reshape(-1), np.arange(65, dtype=np.int64) * 1024)
    assert emul_lib.cq_refined() == 0
    assert len(names) == 60 and np.isfinite(got).all()      # 15 corridors x isabs x {mean, var}
