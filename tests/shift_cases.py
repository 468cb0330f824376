"""Inputs, truth and bound shared by the CPU and GPU tests of the level-invariant columns (tests/test_shift_invariance.py,
tests/test_shift_invariance_gpu.py) and by profiles/shift_invariance.py.

tests/parity.py bounds a cell by 1e-6 |want| + 1e-9 max|x| ** dimension.  For a series whose level is far from its spread
(101 325 +- 5 Pa, 1e8 + N(0, 1), epoch seconds) that floor exceeds a variance, a slope or a spectral density by many
decades, so those columns are compared here a second time, against a bound scaled by the SPREAD:

  * EXACT SHIFTS.  A base series b lies on a dyadic grid, a level c is a multiple of the grid, and both are small enough that
    x = c + b and x - c == b hold without rounding (asserted).  A column that is mathematically invariant under x -> x + c
    then has ONE true value for b and for x: the oracle's value on b, where its float64 arithmetic is well conditioned
    (tests/shift_mp.py restates a core of the columns in 50-digit arithmetic ON x, so the truth is not circular).
  * shift_bound = 1e-6 |truth| + 1e-9 ptp(b) ** dimension: parity.py's own rule with the spread in the place of max|x|.
  * INVARIANT holds, column by column, what is compared: tier A at every level, tier B at the two lower levels of a dtype
    (the reference's own arithmetic leaves 1/4 of the bound for them above: profiles/shift_invariance.md).

The sawtooth family (sawtooth_cases) is the same idea for change_quantiles alone: the changes inside a corridor are a
constant slope plus a jitter of relative size j, the variance of the changes is j^2-small, and its truth comes from exact
rational arithmetic on the float64 samples."""
from fractions import Fraction

import numpy as np

import parity
import route_cases as rc
from tsfresh_amd.feature_extraction import settings

GRID = {"float64": 2.0 ** -10, "float32": 2.0 ** -6}
LIMIT = {"float64": 2.0 ** 6, "float32": 2.0 ** 4}
TIER_B_LEVELS = {"float64": (2.0 ** 10, -3.0 * 2 ** 17), "float32": (2.0 ** 10, -3.0 * 2 ** 15)}
TIER_A_LEVELS = {"float64": TIER_B_LEVELS["float64"] + (2.0 ** 24, 2.0 ** 30), "float32": TIER_B_LEVELS["float32"]}
BASES = ("iid", "walk", "ar1", "sine", "saw")
SHORT_LENGTHS = (61, 300, 1000)
# 2053: the 512-thread spectral group and the four-wave workgroups (beyond 2048 samples).  HBM_SIDE: five samples past the
# last length the sort family holds in LDS (route_cases.LAST_IN_LDS) -- also the HBM side of the entropy family's crossover
# (beyond 4096 samples a plan with several entropy columns takes the bit table in HBM: tests/test_route_edges_gpu.py) while
# every other family stays in LDS (asserted below, and from the launch record on the device).
HBM_SIDE = rc.LAST_IN_LDS["SORT"] + 5
assert all(HBM_SIDE <= last for fam, last in rc.LAST_IN_LDS.items() if fam != "SORT") and (HBM_SIDE - 1) % 5 != 0
LONG_LENGTHS = (2053, HBM_SIDE)
LONG_BASE = {2053: "ar1", HBM_SIDE: "sine"}   # one base and one level per dtype: the oracle's entropies are O(n^2)
LONG_LEVEL = {"float64": -3.0 * 2 ** 17, "float32": -3.0 * 2 ** 15}


def params():
    """ComprehensiveFCParameters without the self-join calculators (and linear_trend_timewise, which needs a DatetimeIndex)."""
    p = dict(settings.ComprehensiveFCParameters())
    for k in ("matrix_profile", "query_similarity_count", "linear_trend_timewise"):
        p.pop(k, None)
    return p


def _fold(raw, limit):
    """raw reflected into (-limit, limit): the identity inside, a walk stays a walk with the same steps."""
    y = np.mod(raw + limit, 4.0 * limit)
    return np.where(y > 2.0 * limit, 4.0 * limit - y, y) - limit


def base_series(kind, n, dtype_name):
    """n samples of `kind` on the grid of `dtype_name`, |b| < LIMIT.  Deterministic in (kind, n, dtype_name)."""
    rng = np.random.default_rng([20261019, BASES.index(kind), n, 64 if dtype_name == "float64" else 32])
    e = rng.standard_normal(n)
    t = np.arange(n)
    if kind == "iid":
        raw = e
    elif kind == "walk":
        raw = 0.1 * np.cumsum(e)
    elif kind == "ar1":
        raw = e.copy()
        for i in range(1, n):
            raw[i] += 0.8 * raw[i - 1]
    elif kind == "sine":
        raw = 2.0 * np.sin(0.05 * t) + 0.3 * e
    else:
        raw = (t % 37) * 0.05 + 0.05 * e
    grid, limit = GRID[dtype_name], LIMIT[dtype_name]
    b = np.round(_fold(raw, limit - 1.0) / grid) * grid
    assert np.max(np.abs(b)) < limit and np.array_equal(np.round(b / grid) * grid, b)
    return b


class Case:
    """One shifted series: x = level + b, exactly."""

    def __init__(self, kind, n, dtype_name, level, base_dtype=None):
        self.kind, self.n, self.dtype_name, self.level = kind, n, dtype_name, float(level)
        self.b = base_series(kind, n, base_dtype or dtype_name)
        dt = np.dtype(dtype_name)
        self.x = (self.level + self.b).astype(dt)
        # the shift is exact in the dtype the device reads: nothing was rounded on the way in, nothing on the way back
        assert np.array_equal(self.x.astype(np.float64), self.level + self.b)
        assert np.array_equal((self.x - dt.type(self.level)).astype(np.float64), self.b)
        assert np.array_equal(self.b.astype(dt).astype(np.float64), self.b)
        self.tier_b = self.level in TIER_B_LEVELS[dtype_name]

    @property
    def label(self):
        return "%s_%d_%s_%+g" % (self.kind, self.n, self.dtype_name, self.level)


def cases(dtype_name, long_lengths=LONG_LENGTHS):
    """Every short length x base x tier-A level of the dtype, and each long length once.  The long series share one base on
    the float32 grid (which lies on the float64 grid), so one oracle run serves both dtypes."""
    out = [Case(kind, n, dtype_name, level) for n in SHORT_LENGTHS for kind in BASES for level in TIER_A_LEVELS[dtype_name]]
    out += [Case(LONG_BASE[n], n, dtype_name, LONG_LEVEL[dtype_name], base_dtype="float32") for n in long_lengths]
    return out


def pack(series, dtype=np.float64):
    """-> (values, offsets) of one ragged batch."""
    values = np.concatenate([np.asarray(s, dtype=dtype) for s in series])
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in series])]).astype(np.int64)
    return values, offsets


_truth = {}


def truth_of(case_list):
    """-> (names, [len(case_list), n_cols]) = oracle(params, b) per case, each distinct base evaluated once per session (in
    worker processes: the entropies of the long bases dominate)."""
    from engines import oracle_engine_parallel
    todo = {}
    for c in case_list:
        key = c.b.tobytes()
        if key not in _truth:
            todo[key] = c.b
    if todo:
        values, offsets = pack(list(todo.values()))
        names, rows = oracle_engine_parallel(params(), values, offsets)
        _truth["names"] = list(names)
        for key, row in zip(todo, rows):
            _truth[key] = row
    return list(_truth["names"]), np.array([_truth[c.b.tobytes()] for c in case_list])


# ---- which columns are invariant under x -> x + c.  Explicit: a calculator joins only if it is mathematically invariant,
# keyed by attr / coeff where only some of its columns are.  Everything else (every intercept, bin 0, energies, sums,
# quantiles of mass, digit statistics, counts against a fixed threshold, the CWT) is compared by tests/parity.py alone;
# ar_coefficient, augmented_dickey_fuller, friedrich_coefficients and max_langevin_fixed_point belong to tests/test_offset.py;
# the location columns (mean, median, quantile, extrema) are of the size of the level and parity.py holds them tightly.
def _attr(col):
    return col.split('attr_"')[1].split('"')[0]


def _not_intercept(col):
    return _attr(col) in ("slope", "stderr", "rvalue", "pvalue")


def _bin_from_one(col):
    return int(col.split("coeff_")[1].split("__")[0]) >= 1


INVARIANT = {
    # tier A: compared at every level
    "variance": ("A", None), "standard_deviation": ("A", None), "cid_ce": ("A", None), "change_quantiles": ("A", None),
    "linear_trend": ("A", _not_intercept), "spkt_welch_density": ("A", None), "absolute_sum_of_changes": ("A", None),
    "mean_abs_change": ("A", None), "mean_change": ("A", None), "mean_second_derivative_central": ("A", None),
    "binned_entropy": ("A", None), "fourier_entropy": ("A", None), "sample_entropy": ("A", None),
    "approximate_entropy": ("A", None), "permutation_entropy": ("A", None), "lempel_ziv_complexity": ("A", None),
    "ratio_beyond_r_sigma": ("A", None), "symmetry_looking": ("A", None), "large_standard_deviation": ("A", None),
    "variance_larger_than_standard_deviation": ("A", None), "count_above_mean": ("A", None), "count_below_mean": ("A", None),
    "longest_strike_above_mean": ("A", None), "longest_strike_below_mean": ("A", None), "number_peaks": ("A", None),
    "first_location_of_maximum": ("A", None), "last_location_of_maximum": ("A", None),
    "first_location_of_minimum": ("A", None), "last_location_of_minimum": ("A", None),
    "has_duplicate": ("A", None), "has_duplicate_max": ("A", None), "has_duplicate_min": ("A", None),
    "percentage_of_reoccurring_values_to_all_values": ("A", None),
    "percentage_of_reoccurring_datapoints_to_all_datapoints": ("A", None),
    "ratio_value_number_to_time_series_length": ("A", None), "length": ("A", None),
    # tier B: compared at the two lower levels of a dtype
    "skewness": ("B", None), "kurtosis": ("B", None), "autocorrelation": ("B", None), "agg_autocorrelation": ("B", None),
    "partial_autocorrelation": ("B", None), "agg_linear_trend": ("B", _not_intercept), "fft_coefficient": ("B", _bin_from_one),
}
# the tier-A columns that are moments of the samples or of their changes: none of them may ever be skipped
MOMENTS = ("variance", "standard_deviation", "cid_ce", "change_quantiles", "absolute_sum_of_changes", "mean_abs_change",
           "mean_change", "mean_second_derivative_central")


def tier_of(col):
    """"A", "B" or None (not compared here)."""
    entry = INVARIANT.get(parity.feature_of(col))
    if entry is None or (entry[1] is not None and not entry[1](col)):
        return None
    return entry[0]


def group_of(col):
    """The row of a column in the tables of profiles/shift_invariance.md: the calculator, with attr where it has one."""
    f = parity.feature_of(col)
    return f + (" " + _attr(col) if 'attr_"' in col else "")


def shift_bound(col, b, truth):
    return 1e-6 * abs(truth) + 1e-9 * float(np.ptp(b)) ** parity.dimension_of(col)


def compare_shift(names, got, truth, case_list, share=1.0, skipped=None, worst=None, what="x", only_tier=None,
                  every_level=False):
    """got, truth: [len(case_list), len(names)].  -> list of mismatches over the invariant cells of every case: tier A at
    every level, tier B at the tier-B levels (only_tier="A": tier A alone).  share: the part of shift_bound the error may
    take (the condition on the inputs asks the reference for 1/4).  skipped receives (case index, column) of the cells
    parity.excluded skips for b or for x; worst, a dict, receives {(group, level): largest error / bound} over the compared
    cells."""
    bad = []
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape == (len(case_list), len(names)), (got.shape, truth.shape)
    tiers = [tier_of(col) for col in names]
    if only_tier is not None:
        tiers = [t if t == only_tier else None for t in tiers]
    for i, c in enumerate(case_list):
        fb, fx = parity._SeriesFacts(c.b), parity._SeriesFacts(c.x.astype(np.float64))
        spectrum = None
        for j, col in enumerate(names):
            # (every_level: profiles/shift_invariance.py measures tier B above its levels too -- that table is why it is tier B)
            if tiers[j] is None or (tiers[j] == "B" and not c.tier_b and not every_level):
                continue
            if parity.excluded(col, fb.x, facts=fb) or parity.excluded(col, fx.x, facts=fx):
                if skipped is not None:
                    skipped.append((i, col))
                continue
            g, w = got[i, j], truth[i, j]
            where = "%s(%s) %s" % (what, c.label, col)
            if np.isnan(w) or np.isnan(g) or np.isinf(w) or np.isinf(g):
                if not (g == w or (np.isnan(g) and np.isnan(w))):
                    bad.append("%s: got %r want %r" % (where, g, w))
                continue
            if parity.is_integer_feature(col):
                if g != w:
                    bad.append("%s: integer feature got %r want %r" % (where, g, w))
                continue
            if 'attr_"angle"' in col:
                k = int(col.split("coeff_")[1].split("__")[0])
                if spectrum is None:
                    spectrum = np.abs(np.fft.rfft(c.b))
                if k < len(spectrum) and spectrum[k] < 1e-9 * max(float(np.abs(c.b).sum()), 1e-300):   # parity.py R2, asked of b
                    if skipped is not None:
                        skipped.append((i, col))
                    continue
                err = abs(g - w)
                err = min(err, 360.0 - err)
                bound = 1e-6 * abs(w) + 1e-9 * 180.0
            else:
                err, bound = abs(g - w), shift_bound(col, c.b, w)
            if worst is not None:
                key = (group_of(col), c.level)
                worst[key] = max(worst.get(key, 0.0), err / bound)
            if err > share * bound:
                bad.append("%s: got %r want %r, error %.3g = %.3g x the bound" % (where, g, w, err, err / bound))
    return bad


def n_invariant_cells(names, case_list):
    tiers = [tier_of(col) for col in names]
    return sum(1 for c in case_list for t in tiers if t == "A" or (t == "B" and c.tier_b))


# ---- the sawtooth family: change_quantiles of x[t] = (t % 37) * 0.05 * (1 + j * N(0, 1))
SAW_JITTERS = (1e-2, 1e-4, 1e-6, 1e-8)
SAW_LENGTHS = (300, 1000)
SAW_LONG = HBM_SIDE    # the HBM side of the sort family's crossover
SAW_CORRIDORS = ((0.2, 0.8), (0.0, 0.6), (0.4, 1.0))
SAW_PARAMS = {"change_quantiles": [{"ql": ql, "qh": qh, "isabs": a, "f_agg": f} for ql, qh in SAW_CORRIDORS
                                   for a in (False, True) for f in ("var", "mean")]}


def sawtooth(n, j, shift=0.0):
    rng = np.random.default_rng([20261019, 37, n, int(round(-np.log10(j)))])
    x = (np.arange(n) % 37) * 0.05 * (1.0 + j * rng.standard_normal(n))
    if shift:
        grid = 2.0 ** -30
        x = np.round(x / grid) * grid
        y = x + shift
        assert np.array_equal(y - shift, x)
        return y
    return x


def zigzag(n, j):
    """Changes of the sizes 0.05 (1 + j N(0, 1)) with the signs + + - repeating: a climb with a wiggle.  Inside a corridor the
    signed changes have the variance (8 / 9) 0.05^2 and the mean 0.05 / 3, their absolute values a j^2-small variance, so only
    the absolute half of the refinement is asked for -- the sawtooth's changes are all positive, its signed and absolute
    columns are equal bit for bit and would not tell the two halves apart."""
    rng = np.random.default_rng([20261019, 2, n, int(round(-np.log10(j)))])
    d = 0.05 * (1.0 + j * rng.standard_normal(n - 1)) * np.where(np.arange(n - 1) % 3 == 2, -1.0, 1.0)
    return np.concatenate([[0.0], np.cumsum(d)])


ZIG_JITTERS = (1e-6, 1e-8)


def sawtooth_cases(lengths=SAW_LENGTHS + (SAW_LONG,)):
    """-> [(label, float64 series)]: every jitter at every length, the j = 1e-6 series of 1000 samples moved to 2^20 on a
    grid of 2^-30 (the changes, and with them every column, stay what they were), and a zig-zag of the smallest and of the
    largest length with the two small jitters."""
    out = [("saw_n%d_j%g" % (n, j), sawtooth(n, j)) for n in lengths for j in SAW_JITTERS]
    if 1000 in lengths:
        out.append(("saw_n1000_j1e-06_at_2^20", sawtooth(1000, 1e-6, shift=2.0 ** 20)))
    out += [("zig_n%d_j%g" % (n, j), zigzag(n, j)) for n in sorted({min(lengths), max(lengths)}) for j in ZIG_JITTERS]
    return out


def _exact_ints(d):
    """dyadic Fractions d -> (Python ints m, their common denominator den, a power of two) with d[i] == m[i] / den exactly."""
    fr = [Fraction(float(v)) for v in d]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr], den


def sawtooth_truth(x, names):
    """The columns of SAW_PARAMS in exact rational arithmetic on the float64 samples, rounded once at the end.  The
    corridor edges are np.quantile's, as in oracle/calculators.py (no sample of these series lies on an interpolated edge)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(len(names))
    for k, col in enumerate(names):
        ql, qh = parity._param(col, "ql"), parity._param(col, "qh")
        lo, hi = np.quantile(x, ql), np.quantile(x, qh)
        inside = (x >= lo) & (x <= hi)
        idx = np.where(inside[:-1] & inside[1:])[0]
        if len(idx) == 0:
            out[k] = 0.0
            continue
        m, den = _exact_ints([Fraction(float(x[i + 1])) - Fraction(float(x[i])) for i in idx])
        if "isabs_True" in col:
            m = [abs(v) for v in m]
        c, s1, s2 = len(m), sum(m), sum(v * v for v in m)
        if 'f_agg_"mean"' in col:
            out[k] = float(Fraction(s1, c * den))
        else:
            out[k] = float(Fraction(c * s2 - s1 * s1, c * c * den * den))
    return out


def compare_sawtooth(names, got, truth, labels, rtol=1e-6, worst=None, what="x"):
    """Relative only: |got - truth| <= rtol |truth| (the truths are 1e-16 .. 1e-1: no absolute floor means anything)."""
    bad = []
    for i, label in enumerate(labels):
        for k, col in enumerate(names):
            g, w = float(got[i][k]), float(truth[i][k])
            err = abs(g - w)
            rel = err / abs(w) if w != 0 else (0.0 if err == 0 else np.inf)
            if worst is not None:
                key = (label, 'var' if 'f_agg_"var"' in col else 'mean')
                worst[key] = max(worst.get(key, 0.0), rel)
            if not err <= rtol * abs(w):
                bad.append("%s(%s) %s: got %r want %r (rel %.3g)" % (what, label, col, g, w, rel))
    return bad
