"""The SORT family runs one 64-lane wavefront per series for every launch group up to 2048 samples (fam_sort.h under the
wave-local wait, tsfa_layout.h: SortLds' one-wavefront layout, the sorted series as a 16-bit order where k_entropy_bits left
one).  Checks every SORT column of ComprehensiveFCParameters against the oracle at the lengths around the wavefront (64), the
old workgroup-size boundary (256), the shared order's limit (1024) and the launch boundary (2048; 2049 stays on the
multi-wavefront path), in both dtypes, with and without the entropy family beside it; the order-statistic, count and boolean
columns against the two-wavefront form (plan option sort_waves = 2) bit for bit; a batch that fills the CUs' LDS against a
sentinel pre-fill; and that a series gives the same bits alone and in a ragged batch.  The kernel body runs the same inputs on
the CPU through the same layout (emul_sort_lib)."""
import numpy as np
import pytest

import emul_sort_lib
import route_cases as rc
from tsfresh_amd.feature_extraction import settings
from engines import emul_engine, hip_engine, oracle_engine
from parity import compare, feature_of

LENGTHS = (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
KINDS = ("noise", "walk", "constant", "ties", "sawtooth", "offset")
DTYPES = (np.float32, np.float64)

SORT_PARAMS = rc.family_params("SORT")
# ... beside the entropy family (two tolerances and more: the bit-matrix sweep, which leaves the sample order up to 1024 samples)
# and a BASIC column
SHARED_PARAMS = dict(SORT_PARAMS, sample_entropy=None, approximate_entropy=[{"m": 2, "r": 0.1}, {"m": 2, "r": 0.3}], mean=None)

# equal for any number of threads: order statistics, counts and what is decided from them
EXACT = ("median", "quantile", "symmetry_looking", "has_duplicate", "ratio_value_number_to_time_series_length",
         "percentage_of_reoccurring_values_to_all_values", "percentage_of_reoccurring_datapoints_to_all_datapoints")


def _series(n, kind):
    """float32 values (cast up for the float64 runs: one oracle run serves both dtypes)."""
    rng = np.random.default_rng([20261019, n, KINDS.index(kind)])
    if kind == "noise":
        x = rng.standard_normal(n)
    elif kind == "walk":
        x = np.cumsum(rng.standard_normal(n))
    elif kind == "constant":
        x = np.full(n, 2.5)
    elif kind == "ties":
        x = rng.integers(0, 5, n).astype(np.float64)
    elif kind == "sawtooth":   # slow flanks of nearly equal changes: change_quantiles' variances ask for the second sweep
        x = (np.arange(n) % 37) * 0.05 * (1.0 + 1e-4 * rng.standard_normal(n))
    else:                      # |mean| >> spread
        x = 4096.0 + 0.25 * rng.standard_normal(n)
    return x.astype(np.float32)


_cache = {}


def _batch():
    """-> (float32 values, offsets, the series as float64, SORT column names, the oracle's matrix): computed once."""
    if "batch" not in _cache:
        xs = [_series(n, kind) for n in LENGTHS for kind in KINDS]
        values = np.concatenate(xs)
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        names, want = oracle_engine(SORT_PARAMS, values.astype(np.float64), offsets)
        want.setflags(write=False)
        _cache["batch"] = (values, offsets, [x.astype(np.float64) for x in xs], names, want)
    return _cache["batch"]


def _sort_columns(names, got, sort_names):
    idx = [names.index(c) for c in sort_names]
    return got[:, idx]


def _launch_groups(offsets):
    """A batch of fewer than 2048 series is ONE launch group, sized by its longest series: the series up to 1024 samples (where
    the entropy kernel shares its order), those up to 2048 and the 2049-sample ones are extracted in a call each."""
    lens = np.diff(offsets)
    return [np.nonzero((lens > lo) & (lens <= hi))[0] for lo, hi in ((0, 1024), (1024, 2048), (2048, 1 << 30))]


def _extract_by_group(params, values, offsets, dtype, names, options=None):
    """-> (matrix of the columns `names`, the SORT launch record of every group)"""
    got = np.full((len(offsets) - 1, len(names)), np.nan)
    records = []
    for rows in _launch_groups(offsets):
        xs = [values[offsets[i]:offsets[i + 1]] for i in rows]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        launches = []
        hnames, out = hip_engine(params, np.concatenate(xs).astype(dtype), offs, options=options, launches=launches)
        records.append(rc.record_of(launches, "SORT"))
        got[rows] = _sort_columns(hnames, out, names)
    return got, records


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("mode", [1, 2], ids=["sorted_copy", "order16"])
def test_emulated_sort_columns_match_oracle(mode, dtype):
    """The kernel body on the CPU through the device's one-wavefront layout (tests/emul/emul_sort.cpp: SortLds carved from one
    poisoned buffer, the series resident in its input precision): with a sorted copy, and with the 16-bit order in its place.
    Launch groups as on the device, then every series as a launch of its own; 2049 samples: the general emulation."""
    values, offsets, series, names, want = _batch()
    for own_launch in (False, True):
        got = np.full(want.shape, np.nan)
        for rows in _launch_groups(offsets):
            xs = [values[offsets[i]:offsets[i + 1]] for i in rows]
            offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
            if max(len(x) for x in xs) <= 2048:
                enames, out = emul_sort_lib.emul_sort(SORT_PARAMS, np.concatenate(xs).astype(dtype), offs, mode, own_launch)
            else:
                enames, out = emul_engine(SORT_PARAMS, np.concatenate(xs).astype(np.float64), offs)
            got[rows] = _sort_columns(enames, out, names)
        bad = compare(names, got, want, series)
        assert not bad, (own_launch, bad[:10])


def test_headline_layout_puts_sixteen_series_on_a_cu():
    """1024 float32 samples, Comprehensive's Langevin scratch (320 doubles), k_basic's statistics at hand: at most 10 240 B."""
    assert emul_sort_lib.lds_bytes(1024, 4, 320, 2, False) <= 10240
    assert emul_sort_lib.lds_bytes(1024, 4, 320, 1, True) <= 160 * 1024 // 12   # without the shared order: twelve


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("plan", ["alone", "shared_order"])
def test_sort_columns_match_oracle_and_the_two_wavefront_form(plan, dtype):
    values, offsets, series, names, want = _batch()
    params = SORT_PARAMS if plan == "alone" else SHARED_PARAMS
    got, recs = _extract_by_group(params, values, offsets, dtype, names)
    assert [r["max_len"] for r in recs] == [1024, 2048, 2049], recs
    # one wavefront up to 2048 samples; up to 1024 the sorted series is the entropy kernel's order where that kernel runs
    assert [r["threads"] for r in recs[:2]] == [64, 64] and recs[2]["threads"] > 64, recs
    assert [r["variant"] & 6 for r in recs] == ([4, 2, 0] if plan == "shared_order" else [2, 2, 0]), recs
    bad = compare(names, got, want, series)
    assert not bad, bad[:10]
    got2, recs2 = _extract_by_group(params, values, offsets, dtype, names, options={"sort_waves": 2})
    assert [r["threads"] for r in recs2[:2]] == [128, 128] and [r["variant"] & 6 for r in recs2] == [0, 0, 0], recs2
    exact = [j for j, c in enumerate(names) if feature_of(c) in EXACT]
    assert len(exact) >= 20, len(exact)
    np.testing.assert_array_equal(got[:, exact], got2[:, exact])
    bad2 = compare(names, got2, want, series)
    assert not bad2, bad2[:10]


@pytest.mark.gpu
def test_sort_waves_takes_one_or_two():
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    fplan = compile_fc_parameters({"median": None})
    plan = _native.Plan(fplan.native_specs(_native.calc_id), device=0)
    try:
        plan.set_option("sort_waves", 1)
        plan.set_option("sort_waves", 2)
        for v in (0, 3, 1.5, -1):
            with pytest.raises(Exception):
                plan.set_option("sort_waves", v)
    finally:
        plan.close()


@pytest.mark.gpu
def test_a_batch_that_fills_the_lds_leaves_no_cell_unwritten():
    """About 600 series of 1024 samples: sixteen one-wavefront workgroups share a CU's LDS.  Pre-filled with a sentinel;
    every cell must be written, the SORT columns with the bits of the run without the pre-fill."""
    rng = np.random.default_rng(1024)
    n_series, n = 600, 1024
    x = rng.standard_normal((n_series, n)).astype(np.float32)
    x[1::2] = np.cumsum(x[1::2], axis=1)
    offsets = np.arange(n_series + 1, dtype=np.int64) * n
    sentinel = -9.87654321e33
    params = settings.ComprehensiveFCParameters()   # the headline plan: k_basic's statistics, the shared order, k_perm
    launches = []
    names, got = hip_engine(params, x.reshape(-1), offsets, options={"fill": sentinel}, launches=launches)
    rec = rc.record_of(launches, "SORT")
    assert (rec["threads"], rec["variant"] & 6) == (64, 4), rec
    assert rec["lds_bytes"] <= 10240, rec   # sixteen series per CU
    assert not np.any(got == sentinel), [names[j] for j in np.unique(np.nonzero(got == sentinel)[1])][:10]
    names2, plain = hip_engine(params, x.reshape(-1), offsets)
    sort_cols = [j for j, c in enumerate(names) if feature_of(c) in SORT_PARAMS]
    np.testing.assert_array_equal(got[:, sort_cols], plain[:, sort_cols])


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["alone", "shared_order"])
def test_sort_columns_do_not_depend_on_the_batch(plan):
    params = SORT_PARAMS if plan == "alone" else SHARED_PARAMS
    rng = np.random.default_rng(1500)
    probes = [rng.standard_normal(200).astype(np.float32), np.cumsum(rng.standard_normal(1500)).astype(np.float32)]
    alone = []
    for x in probes:
        names, got = hip_engine(params, x, np.array([0, len(x)], dtype=np.int64))
        alone.append(got[0])
    sort_cols = [j for j, c in enumerate(names) if feature_of(c) in SORT_PARAMS]
    assert len(sort_cols) == len(_batch()[3])
    ragged = [rng.standard_normal(2000).astype(np.float32), probes[0], rng.standard_normal(700).astype(np.float32), probes[1]]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in ragged])]).astype(np.int64)
    names2, got = hip_engine(params, np.concatenate(ragged), offsets)
    assert names2 == names
    np.testing.assert_array_equal(got[1][sort_cols], alone[0][sort_cols])
    np.testing.assert_array_equal(got[3][sort_cols], alone[1][sort_cols])
