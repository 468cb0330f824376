"""Every series length from 1 to 70 (and 127 .. 129) of eight data families against outputs of the REAL reference, on
every route that serves short series: the oracle, the g++ build of the kernel sources, and on the device the series entry
(float32 and float64 samples, row form and wavefront form of k_basic / k_trend), the same series in a launch sized for
long ones, and the window entry that rolling uses.

Fixtures (tests/golden/golden_cases.py::short_series; they regenerate bit for bit with the committed generators):

    python tests/golden/gen_golden_main.py --set short                                  # ref_main_short.npz
    python tests/golden/gen_golden_main.py --set short --nosimd                         # ref_main_short_nosimd.npz
    python3.9 tests/golden/gen_golden_conda.py --set short                              # ref_conda_short.npz (the second
                                                                                        # interpreter: that file's docstring)

All comparisons use the bars of tests/parity.py as they are (counts exact, floats 1e-6 relative); no rule of it is new.
The cells its rules skip are bounded in every test: at most 1.5 % of all cells, at most 5 % of any family.

Measured with the oracle on the committed set (586 series x 783 columns = 458 838 cells; the emulation and every device
route skip the same cells, the rules read the series alone); each test prints its own table:

    pair          skipped          const          ramp          two           ints          digits       other five, each
    short         2 862 (0.62 %)   1 369 (2.40 %) 594 (1.04 %)  457 (0.80 %)  371 (0.65 %)  11 (0.70 %)  15 (0.03 %)
    short_nosimd  1 798 (0.39 %)   1 009 (1.77 %) 594 (1.04 %)  102 (0.18 %)   22 (0.04 %)  11 (0.70 %)  15 (0.03 %)

    by rule (both pairs): R3 fft_aggregated 320, spkt_welch_density 240, R3/R10 fourier_entropy 428, R4/R5
    augmented_dickey_fuller 231, R6/R11 max_langevin_fixed_point 72, R7 agg_linear_trend 159, linear_trend 144, R8
    number_cwt_peaks 204; `short` alone: R1 permutation_entropy 1 064 (the tie-holding windows, pinned by `short_nosimd`).
    The 146 window rows (prefix, suffix): 30 of 114 318 (0.03 %), all R3 (the one-sample windows).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import goldens
from engines import emul_engine, hip_engine, oracle_engine_parallel
from golden_cases import SHORT_FAMILIES, SHORT_LENGTHS, SHORT_WALK_LEN, short_walk
from parity import compare, feature_of, series_facts
from tsfresh_amd.feature_extraction.settings import ComprehensiveFCParameters

PAIRS = ("short", "short_nosimd")
CAP_ALL, CAP_FAMILY = 0.015, 0.05
UNIFORM_DIGITS = ("digits_9", "digits_90", "ramp_10")     # benford_correlation is 0/0 = NaN in the reference
RIDERS = (1000, 2049, 4097)

# the rule(s) of tests/parity.py that can skip a cell of a calculator
RULES = {"permutation_entropy": "R1", "fourier_entropy": "R3/R10", "spkt_welch_density": "R3", "fft_aggregated": "R3",
         "ar_coefficient": "R4", "augmented_dickey_fuller": "R4/R5", "max_langevin_fixed_point": "R6/R11",
         "friedrich_coefficients": "R11", "agg_linear_trend": "R7", "linear_trend": "R7", "partial_autocorrelation": "R9",
         "number_cwt_peaks": "R8"}

_FIXTURES = {}
_FACTS = []


def _fixture(pair):
    if pair not in _FIXTURES:
        _FIXTURES[pair] = goldens.load(pair)
    return _FIXTURES[pair]


def _family(label):
    return label.rsplit("_", 1)[0]


def _check(pair, got_names, got, rows=None):
    """Compare `got` (the fixture's rows `rows`, default all) with the fixture pair; assert no mismatch and the skip caps."""
    g = _fixture(pair)
    rows = list(range(len(g["series"]))) if rows is None else list(rows)
    series = [g["series"][i] for i in rows]
    labels = [g["labels"][i] for i in rows]
    if not _FACTS:   # the predicates' facts are functions of the series alone: every comparison of this module shares them
        _FACTS.extend(series_facts(g["series"]))
    skipped = []
    bad = compare(g["names"], goldens.align(g["names"], list(got_names), np.asarray(got)), g["matrix"][rows], series,
                  simd_golden=g["simd"], skipped=skipped, series_facts=[_FACTS[i] for i in rows])
    n_cols = len(g["names"])
    per_family, per_rule = {}, {}
    for i, col in skipped:
        per_family[_family(labels[i])] = per_family.get(_family(labels[i]), 0) + 1
        key = "%s %s" % (RULES.get(feature_of(col), "R12-R14"), feature_of(col))
        per_rule[key] = per_rule.get(key, 0) + 1
    sizes = {}
    for lb in labels:
        sizes[_family(lb)] = sizes.get(_family(lb), 0) + n_cols
    print("%s: %d of %d cells skipped (%.2f %%); by family: %s; by rule: %s" % (
        pair, len(skipped), len(rows) * n_cols, 100.0 * len(skipped) / (len(rows) * n_cols),
        ", ".join("%s %d (%.2f %%)" % (f, c, 100.0 * c / sizes[f]) for f, c in sorted(per_family.items())),
        ", ".join("%s %d" % kv for kv in sorted(per_rule.items()))))
    assert not bad, "%d mismatches, first: %s" % (len(bad), [b.replace("series %d " % int(b.split()[1]), labels[int(b.split()[1])] + " ") for b in bad[:10]])
    assert len(skipped) <= CAP_ALL * len(rows) * n_cols, (len(skipped), len(rows) * n_cols)
    for f, c in per_family.items():
        assert c <= CAP_FAMILY * sizes[f], (f, c, sizes[f])


def test_fixture_holds_every_comprehensive_column_and_case():
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    fplan = compile_fc_parameters(ComprehensiveFCParameters())
    for pair in PAIRS:
        g = _fixture(pair)
        assert sorted(g["names"]) == sorted("value__" + n for n in fplan.names) and len(g["names"]) == 783
        want = ["%s_%d" % (f, n) for n in SHORT_LENGTHS for f in SHORT_FAMILIES] + ["digits_9", "digits_90"]
        assert g["labels"] == want and "ramp_10" in want
        assert [len(x) for x in g["series"]] == [int(lb.rsplit("_", 1)[1]) for lb in want]
        assert np.array_equal(g["values"], g["values"].astype(np.float32).astype(np.float64))   # one fixture, both dtypes
        w = short_walk()
        for n in SHORT_LENGTHS:
            assert np.array_equal(g["series"][want.index("prefix_%d" % n)], w[:n])
            assert np.array_equal(g["series"][want.index("suffix_%d" % n)], w[SHORT_WALK_LEN - n:])
        # the reference's own answer for uniformly spread leading digits
        j = g["names"].index("value__benford_correlation")
        assert all(np.isnan(g["matrix"][want.index(lb), j]) for lb in UNIFORM_DIGITS)


_CPU = {}


def _cpu_rows(engine):
    if engine not in _CPU:
        g = _fixture("short")
        _CPU[engine] = engine(ComprehensiveFCParameters(), g["values"], g["offsets"])
    return _CPU[engine]


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("engine", [oracle_engine_parallel, emul_engine], ids=["oracle", "emul"])   # (the same oracle, a process per series)
def test_engine_matches_the_reference_on_the_ladder(engine, pair):
    names, got = _cpu_rows(engine)
    _check(pair, names, got)


def test_emulation_returns_nan_for_uniformly_spread_leading_digits():
    """np.corrcoef takes the mean of the nine digit shares in numpy's reduction order (eight partial sums combined pairwise,
    then the ninth): nine shares of 0.1 give exactly 0.1, every deviation is 0 and the result 0/0.  A serial sum gives
    0.09999999999999999 and divides round-off by round-off (3.97e-17 on arange(10))."""
    g = _fixture("short")
    names, got = _cpu_rows(emul_engine)
    j = list(names).index("value__benford_correlation")
    for lb in UNIFORM_DIGITS:
        assert np.isnan(got[g["labels"].index(lb), j]), (lb, got[g["labels"].index(lb), j])


# ---------------------------------------------------------------------------------------------------------------- device

_DEVICE = {}


def _device_rows(dtype, row_form):
    """The whole ladder in one batch through the series entry; one run per (dtype, row_form) and session."""
    key = (np.dtype(dtype).name, row_form)
    if key not in _DEVICE:
        g = _fixture("short")
        _DEVICE[key] = hip_engine(ComprehensiveFCParameters(), g["values"].astype(dtype), g["offsets"],
                                  options=None if row_form is None else {"row_form": row_form})
    return _DEVICE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("row_form", [None, 0], ids=["default", "row_form_0"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_hip_matches_the_reference_on_the_ladder(gpu, dtype, row_form, pair):
    names, got = _device_rows(dtype, row_form)
    g = _fixture(pair)
    j = list(names).index("value__benford_correlation")
    for lb in UNIFORM_DIGITS:
        assert np.isnan(got[g["labels"].index(lb), j]), (lb, got[g["labels"].index(lb), j])
    _check(pair, names, got)


_RIDDEN = {}


def _ridden_rows(dtype):
    key = np.dtype(dtype).name
    if key not in _RIDDEN:
        g = _fixture("short")
        rng = np.random.default_rng(20261022)
        riders = [rng.standard_normal(n, dtype=np.float32).astype(np.float64) for n in RIDERS]
        # a rider in front, one in the middle, one behind: the ladder rows sit at shifted offsets of the value buffer
        n = len(g["series"])
        order = [riders[0]] + g["series"][:n // 2] + [riders[1]] + g["series"][n // 2:] + [riders[2]]
        values = np.concatenate(order).astype(dtype)
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in order])]).astype(np.int64)
        records = []
        names, got = hip_engine(ComprehensiveFCParameters(), values, offsets, launches=records)
        # what the batch is for, from the record of the launch: ONE launch group, every family sized for the longest rider
        for fam in ("BASIC", "TREND", "SORT", "SPECTRAL", "AR", "CWT", "SEQ", "ENTROPY"):
            recs = [r for r in records if r["family"] == fam]
            assert recs, (fam, records)
            assert all(r["max_len"] == max(RIDERS) and r["length_class"] == 0 and r["n_series"] == n + len(RIDERS) for r in recs), recs
        keep = list(range(1, 1 + n // 2)) + list(range(2 + n // 2, 2 + n))
        assert np.all(np.isfinite(got[[0, 1 + n // 2, 2 + n], list(names).index("value__mean")]))
        _RIDDEN[key] = (names, got[keep])
    return _RIDDEN[key]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_hip_ladder_in_a_launch_sized_for_long_series(gpu, dtype, pair):
    """The ladder in one batch with riders of 1000, 2049 and 4097 samples: every family meets a short series in a launch
    configured for a long one.  Compared with the fixture again, not bit for bit with the batch of short series alone
    (k_spectral's workgroup size follows the launch group)."""
    names, got = _ridden_rows(dtype)
    _check(pair, names, got)


_WINDOWS = {}


def _window_cases():
    g = _fixture("short")
    rows, starts, ends = [], [], []
    for n in SHORT_LENGTHS:
        rows += [g["labels"].index("prefix_%d" % n), g["labels"].index("suffix_%d" % n)]
        starts += [0, SHORT_WALK_LEN - n]
        ends += [n, SHORT_WALK_LEN]
    return rows, np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64)


def _window_rows(dtype):
    key = np.dtype(dtype).name
    if key not in _WINDOWS:
        from tsfresh_amd import _native
        from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
        fplan = compile_fc_parameters(ComprehensiveFCParameters())
        plan = _native.Plan(fplan.native_specs(_native.calc_id), device=0)
        _, starts, ends = _window_cases()
        try:
            got = np.array(plan.extract_windows_host(short_walk().astype(dtype), starts, ends))
        finally:
            plan.close()
        _WINDOWS[key] = (["value__" + n for n in fplan.names], got)
    return _WINDOWS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_hip_window_entry_matches_the_reference_on_every_prefix_and_suffix(gpu, dtype, pair):
    """The 129-sample walk uploaded once; (start, end) views of it for every prefix_n and suffix_n: the windows rolling cuts,
    at every alignment of the value buffer."""
    names, got = _window_rows(dtype)
    rows, _, _ = _window_cases()
    snames, sgot = _device_rows(dtype, None)
    assert list(snames) == list(names)
    same = (got == sgot[rows]) | (np.isnan(got) & np.isnan(sgot[rows]))
    print("window entry vs series entry (%s): %d of %d cells differ in their bits" % (np.dtype(dtype).name, int((~same).sum()), same.size))
    _check(pair, names, got, rows=rows)
