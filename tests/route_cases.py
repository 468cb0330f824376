"""Inputs shared by the CPU (emulation) and GPU tests of the length-dependent launch routes
(tests/test_route_edges_emul.py, tests/test_route_edges_gpu.py).

run_batch (csrc/tsfa_api.cpp) picks, per kernel family, a build, a workgroup size and a scratch layout from the longest series
of a launch group.  The tests here put series on both sides of every such switch; which side a length is on is read from
the record of the launch (Plan.last_launches), never assumed."""
import numpy as np

from tsfresh_amd.feature_extraction import settings

# ---- one subset of ComprehensiveFCParameters per kernel family (the family column of TSFA_CALC_LIST, csrc/tsfa_specs.h, which
# Python cannot see: the GPU test checks from the launch record that a subset launched its family and nothing else).
# Left out: the two O(n^2) entropies (ENTROPY has a test of its own), matrix_profile (tests/test_mprofile_gpu.py walks its
# crossover), linear_trend_timewise (needs a DatetimeIndex) and cwt_coefficients (k_cwt_gemm reads the first samples of a
# series only: no route depends on the length).
_FAMILY_CALCS = {
    "BASIC": ["sum_values", "mean", "length", "standard_deviation", "variance", "root_mean_square", "maximum", "absolute_maximum",
              "minimum", "abs_energy", "variation_coefficient", "variance_larger_than_standard_deviation",
              "large_standard_deviation", "ratio_beyond_r_sigma", "skewness", "kurtosis", "mean_abs_change", "mean_change",
              "mean_second_derivative_central", "absolute_sum_of_changes", "cid_ce", "count_above_mean", "count_below_mean",
              "count_above", "count_below", "value_count", "range_count", "number_crossing_m", "first_location_of_maximum",
              "last_location_of_maximum", "first_location_of_minimum", "last_location_of_minimum", "has_duplicate_max",
              "has_duplicate_min", "longest_strike_above_mean", "longest_strike_below_mean", "number_peaks",
              "energy_ratio_by_chunks", "c3", "time_reversal_asymmetry_statistic", "autocorrelation", "binned_entropy",
              "benford_correlation", "query_similarity_count"],
    "TREND": ["index_mass_quantile", "linear_trend", "agg_linear_trend"],
    "SORT": ["median", "quantile", "symmetry_looking", "mean_n_absolute_max", "change_quantiles", "has_duplicate",
             "ratio_value_number_to_time_series_length", "percentage_of_reoccurring_values_to_all_values",
             "percentage_of_reoccurring_datapoints_to_all_datapoints", "sum_of_reoccurring_values",
             "sum_of_reoccurring_data_points", "permutation_entropy", "friedrich_coefficients", "max_langevin_fixed_point"],
    "SPECTRAL": ["fft_coefficient", "fft_aggregated", "spkt_welch_density", "fourier_entropy"],
    "AR": ["agg_autocorrelation", "partial_autocorrelation", "ar_coefficient", "augmented_dickey_fuller"],
    "CWT": ["number_cwt_peaks"],
    "SEQ": ["lempel_ziv_complexity"],
}
FAMILIES = tuple(_FAMILY_CALCS)


def family_params(family):
    """The calculators of one kernel family with Comprehensive's parameter grids."""
    comp = settings.ComprehensiveFCParameters()
    missing = [c for c in _FAMILY_CALCS[family] if c not in comp]
    assert not missing, missing
    return {c: comp[c] for c in _FAMILY_CALCS[family]}


def trend_params_wide():
    """TREND with the n-double work array.  tsfa_prepare_family (csrc/tsfa_host_tables.h) sets TsfaAltPlan::small_w unless an
    index_mass_quantile column is evaluated on its own or agg_linear_trend holds more than TSFA_ALT_MAXKEYS = 16 distinct
    (chunk_len, f_agg) keys.  Comprehensive's grids (8 quantiles, 12 keys) set it, and no subset of them can unset it: the
    plain form is reached with the same calculators and 17 quantiles, more than the indexed evaluation holds."""
    p = family_params("TREND")
    p["index_mass_quantile"] = [{"q": round(0.05 * k, 2)} for k in range(1, 18)]
    return p


def subset(name):
    """name: a family, or "TREND_wide" (trend_params_wide)."""
    return trend_params_wide() if name == "TREND_wide" else family_params(name)


def family_of(name):
    return "TREND" if name == "TREND_wide" else name


# ---- series.  Generated in float32 and cast up for the float64 runs: both dtypes see the same values, one oracle run
# serves both.  A series of n samples is the first n of a fixed stream of its (kind, seed), so the series at n and at n + 1
# differ in the last sample only and the parity predicates, which read the series alone, skip the same share at both.
KINDS = ("iid", "walk", "ints")
ALL_KINDS = KINDS + ("wave",)
_STREAM = 70000
_streams = {}


def series_at(n, kind, seed=0):
    """iid: standard normal noise.  walk: a random walk rounded to one decimal (ties).  ints: integers 0 .. 3.
    wave: a slow sine under noise -- stands in for `ints` where the parity predicates skip integer series (kinds_of)."""
    assert 1 <= n <= _STREAM and kind in ALL_KINDS
    key = (kind, seed)
    if key not in _streams:
        rng = np.random.default_rng([20261018, ALL_KINDS.index(kind), seed])
        if kind == "iid":
            x = rng.standard_normal(_STREAM)
        elif kind == "walk":
            x = np.round(np.cumsum(rng.standard_normal(_STREAM)), 1)
        elif kind == "ints":
            x = rng.integers(0, 4, _STREAM).astype(np.float64)
        else:
            x = np.sin(0.01 * np.arange(_STREAM)) + 0.3 * rng.standard_normal(_STREAM)
        _streams[key] = x.astype(np.float32)
    return _streams[key][:n].copy()


def batch(lengths_and_kinds, dtype=np.float32):
    """[(n, kind, seed)] -> (values, offsets, series as float64)."""
    xs = [series_at(n, kind, seed) for n, kind, seed in lengths_and_kinds]
    values = np.concatenate(xs).astype(dtype)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    return values, offsets, [x.astype(np.float64) for x in xs]


def kinds_of(name):
    """The three kinds of a subset.  number_cwt_peaks of a series of small integers is a cell the parity predicates skip
    (ridge lines through tied CWT maxima: parity._cwt_peaks_ambiguous) -- 2 of 2 columns, measured by
    tests/test_route_edges_emul.py -- so CWT takes `wave` in its place."""
    return ("iid", "walk", "wave") if name == "CWT" else KINDS


def edge_batch(name, n, short=300):
    """The batch of one side of a switch: the subset's three kinds at n samples and a short series that rides in the same
    launch."""
    return [(n, kind, 0) for kind in kinds_of(name)] + [(short, "iid", 1)]


# ---- the launch record
class Prober:
    """One native plan, asked what it launches for a single iid series of n samples (one extract per probe: milliseconds)."""

    def __init__(self, params, dtype, device=0):
        from tsfresh_amd import _native
        from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
        fplan = compile_fc_parameters(params)
        self.plan = _native.Plan(fplan.native_specs(_native.calc_id), device=device)
        self.dtype = dtype
        self.seen = {}

    def __call__(self, n):
        if n not in self.seen:
            x = series_at(n, "iid", 2).astype(self.dtype)
            self.plan.extract_host(x, np.array([0, n], dtype=np.int64))
            self.seen[n] = self.plan.last_launches()
        return self.seen[n]

    def close(self):
        self.plan.close()


def record_of(records, family):
    """The one record of `family` among the records of a single-group extract."""
    recs = [r for r in records if r["family"] == family]
    assert len(recs) == 1, (family, records)
    return recs[0]


def find_flip(params, dtype, lo, hi, key, probe=None):
    """The largest n in [lo, hi) with key(records at n) == key(records at lo) and key(records at n + 1) different, found by
    bisection on the launch record of single-series extracts (no table of expected lengths is assumed).  Fails when lo and hi
    agree.  With several flips in the bracket it finds one of them; the flip is asserted once more at (n, n + 1)."""
    own = probe is None
    probe = probe or Prober(params, dtype)
    try:
        k_lo = key(probe(lo))
        assert key(probe(hi)) != k_lo, "no crossover in the bracket %d .. %d (both: %r)" % (lo, hi, k_lo)
        a, b = lo, hi            # invariant: key(a) == k_lo, key(b) != k_lo
        while b - a > 1:
            m = (a + b) // 2
            if key(probe(m)) == k_lo:
                a = m
            else:
                b = m
        assert key(probe(a)) == k_lo and key(probe(a + 1)) != k_lo, (a, probe(a), probe(a + 1))
        return a
    finally:
        if own:
            probe.close()


def find_all_flips(params, dtype, lo, hi, key):
    """Every flip of `key` between lo and hi, walking up: [n] with key changing between n and n + 1."""
    probe = Prober(params, dtype)
    flips = []
    try:
        while lo < hi and key(probe(lo)) != key(probe(hi)):
            n = find_flip(params, dtype, lo, hi, key, probe=probe)
            flips.append(n)
            lo = n + 1
        return flips
    finally:
        probe.close()


# The last length whose carve fits LDS per family, from the carve functions of csrc/tsfa_layout.h evaluated on the CPU with the
# workgroup sizes run_batch uses above 4096 samples (a reading of the code: the GPU test locates the lengths itself and
# compares).  SEQ: Comprehensive's five `bins` values, whose launch shrinks from five chains to one before it leaves LDS.
LAST_IN_LDS = {"BASIC": 9680, "TREND": 19326, "TREND_wide": 9872, "SORT": 8192, "SPECTRAL": 9692, "AR": 18096, "CWT": 8990,
               "SEQ": 62909}
