"""`-m gpu`: every kernel family on both sides of the lengths at which run_batch (csrc/tsfa_api.cpp) switches its route.

The largest switch is per family: while the family's LDS carve for the longest series of a launch fits TSFA_LDS_LIMIT the LDS
build runs; one sample longer, the HBM-scratch build (tsfa_kernels_long.hip: 256 threads, a persistent grid, a scratch slot
per workgroup).  The last length in LDS is the carve at its largest -- an off-by-one in a carve overruns exactly there -- and the
first beyond it is the long build at its smallest.  The lengths are located on the device, by bisection on the record of what
an extract launched (Plan.last_launches, route_cases.find_flip); the results at both lengths are compared with the oracle in
float32 and float64, and with each other.

Wall time per case on an MI355X: the pull request that added this file lists them; the oracle of a subset runs once, in worker
processes, and serves both dtypes."""
import json
import os
import time

import numpy as np
import pytest

import route_cases as rc
from engines import hip_engine, oracle_engine_parallel
from parity import compare
from test_route_edges_emul import SKIP_SHARE
from tsfresh_amd.feature_extraction import settings

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [np.float32, np.float64]

# Where the crossover is looked for.  SEQ (Comprehensive's five lempel_ziv_complexity `bins`) first drops from five chains per
# launch to one and leaves LDS only near 62 900 samples: its bracket ends at the 65 535 samples the long-series build documents.
BRACKET = {name: (4097, 40000) for name in rc.LAST_IN_LDS}
BRACKET["SEQ"] = (4097, 65535)

_flips = {}
_oracle = {}
_hip = {}


def _long_build(fam):
    return lambda records: rc.record_of(records, fam)["long_build"]


def _variant(fam, mask=-1):
    return lambda records: rc.record_of(records, fam)["variant"] & mask


def _flip(tag, params, dtype, lo, hi, key):
    k = (tag, np.dtype(dtype).name)
    if k not in _flips:
        _flips[k] = rc.find_flip(params, dtype, lo, hi, key)
    return _flips[k]


def _want(tag, params, spec):
    """Oracle rows of the series of `spec` ([(n, kind, seed)]), once per (tag, spec)."""
    k = (tag, tuple(spec))
    if k not in _oracle:
        values, offsets, series = rc.batch(spec, np.float64)
        _oracle[k] = oracle_engine_parallel(params, values, offsets) + (series,)
    return _oracle[k]


def _got(tag, params, spec, dtype):
    """(names, matrix, launch records) of one extract of the series of `spec`."""
    k = (tag, tuple(spec), np.dtype(dtype).name)
    if k not in _hip:
        values, offsets, _ = rc.batch(spec, dtype)
        records = []
        names, got = hip_engine(params, values, offsets, launches=records)
        _hip[k] = (names, got, records)
    return _hip[k]


def _check_side(tag, name, params, n, dtype, expect):
    """One side of a switch: the subset's three kinds at n samples and a 300-sample series in one extract.  expect(record)
    asserts the route.  Against the oracle, and float32 against float64 (the same values: the same bar, counts equal)."""
    fam = rc.family_of(name)
    spec = rc.edge_batch(name, n)
    names, got, records = _got(tag, params, spec, dtype)
    assert {r["family"] for r in records} == {fam}, records      # the subset launched its family and no other
    rec = rc.record_of(records, fam)
    assert (rec["max_len"], rec["n_series"], rec["length_class"]) == (n, len(spec), 0), rec
    expect(rec)
    onames, want, series = _want(tag, params, spec)
    assert names == onames
    skipped = []
    bad = compare(names, got, want, series, skipped=skipped)
    assert not bad, "%s at %d samples (%s): %d mismatches, first: %s" % (name, n, rec, len(bad), bad[:8])
    # the share tests/test_route_edges_emul.py measured on these inputs, plus two points (the convention of test_hip_offset_fuzz)
    assert len(skipped) <= (SKIP_SHARE.get(name, 0.0) + 0.02) * got.size, (len(skipped), got.size)
    other = np.float64 if np.dtype(dtype) == np.float32 else np.float32
    _, got_other, _ = _got(tag, params, spec, other)
    bad = compare(names, got, got_other, series)
    assert not bad, "%s at %d samples: float32 and float64 disagree: %s" % (name, n, bad[:8])


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("name", list(rc.LAST_IN_LDS))
def test_family_at_its_lds_crossover(gpu, name, dtype):
    """Locate n with the LDS build at n and the long build at n + 1, then extract (three kinds at n + a 300-sample series) and
    (three kinds at n + 1 + a 300-sample series).  Two extracts, not one ragged batch: a batch is split into length classes only
    from 2048 series on, in groups of at least 512 (shape_from_stats), and n and n + 1 fall into one class anyway except at a
    power of two -- in one batch both lengths would take the long build.  The short series rides in the launch of the long
    ones, so each build also meets a series far shorter than its carve.
    TREND: Comprehensive's grids set TsfaAltPlan::small_w (the carve without the n-double work array); "TREND_wide" is the same
    three calculators with 17 quantiles, which unsets it (route_cases.trend_params_wide), so both carve forms meet their edge."""
    t0 = time.perf_counter()
    params = rc.subset(name)
    fam = rc.family_of(name)
    lo, hi = BRACKET[name]
    n = _flip(name, params, dtype, lo, hi, _long_build(fam))

    def in_lds(rec):
        assert rec["long_build"] == 0 and rec["lds_bytes"] <= 160 * 1024, rec

    def in_hbm(rec):
        assert rec["long_build"] == 1 and rec["threads"] == 256, rec

    _check_side(name, name, params, n, dtype, in_lds)
    _check_side(name, name, params, n + 1, dtype, in_hbm)
    print("\n%s %s: last length in LDS %d (carve arithmetic on the CPU: %d), %.1f s"
          % (name, np.dtype(dtype).name, n, rc.LAST_IN_LDS[name], time.perf_counter() - t0))


def _perm_params():
    return {"permutation_entropy": settings.ComprehensiveFCParameters()["permutation_entropy"]}


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("switch", ["cwt_rowv", "k_perm", "seq_group"])
def test_variant_switches_at_their_edge(gpu, switch, dtype):
    """The switches inside a build that depend on the length alone, same scheme on the record's `variant`:
    cwt_rowv   number_cwt_peaks keeps its row values in LDS while that carve fits 96 KB (bracket 2049 .. 8990)
    k_perm     permutation_entropy alone: k_perm runs beside k_sort while the series in its input precision and the pattern
               histogram fit LDS -- the one switch that depends on the dtype (bracket 4097 .. 45 000); k_sort itself has
               left LDS long before, so this edge lies inside the long-series build
    seq_group  every step of lempel_ziv_complexity's launch shape (chains per launch, symbol rows in LDS or HBM) between 2049
               samples and the family's crossover; its columns are counts: exact"""
    t0 = time.perf_counter()
    if switch == "cwt_rowv":
        name, params, key = "CWT", rc.subset("CWT"), _variant("CWT", 1)
        flips = [_flip(switch, params, dtype, 2049, 8990, key)]
    elif switch == "k_perm":
        name, params, key = "SORT", _perm_params(), _variant("SORT")
        flips = [_flip(switch, params, dtype, 4097, 45000, key)]
    else:
        name, params, key = "SEQ", rc.subset("SEQ"), _variant("SEQ")
        top = _flip("SEQ", params, dtype, *BRACKET["SEQ"], _long_build("SEQ"))
        k = (switch, np.dtype(dtype).name)
        if k not in _flips:
            _flips[k] = rc.find_all_flips(params, dtype, 2049, top, key)
        flips = _flips[k]
        assert len(flips) >= 2, flips      # (five `bins` values cannot stay one launch shape up to the crossover)
    fam = rc.family_of(name)
    if switch == "seq_group":      # one oracle run (one pool of workers) for the series of every step
        _want_many(switch, params, [rc.edge_batch(name, m) for n in flips for m in (n, n + 1)])
    seen = []
    for n in flips:
        for m in (n, n + 1):
            def note(rec):
                assert rec["long_build"] == (1 if switch == "k_perm" else 0), rec
                seen.append(key([rec]))
            _check_side(switch, name, params, m, dtype, note)
        assert seen[-2] != seen[-1], (switch, n, seen)
    if switch == "k_perm":
        assert seen == [1, 0], seen
    if switch == "cwt_rowv":
        assert seen == [1, 0], seen
    print("\n%s %s: variant %s at %s, %.1f s" % (switch, np.dtype(dtype).name, seen, flips, time.perf_counter() - t0))


def _want_many(tag, params, specs):
    todo = [s for s in specs if (tag, tuple(s)) not in _oracle]
    if not todo:
        return
    flat = [item for s in todo for item in s]
    values, offsets, series = rc.batch(flat, np.float64)
    names, want = oracle_engine_parallel(params, values, offsets)
    r = 0
    for s in todo:
        _oracle[(tag, tuple(s))] = (names, want[r:r + len(s)], series[r:r + len(s)])
        r += len(s)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_sample_entropy_just_beyond_the_bit_table(gpu, dtype):
    """TSFA_ENTH_MAXN = 17 408 samples is the last length of the bit-matrix sweep over HBM (fam_entropy_hbits.h, `ent_cnt` 4:
    taken only by a plan with at least two entropy columns, hence the approximate_entropy column); 17 409 takes the pair sweep
    of the long-series build.  sample_entropy against the oracle's stored values (tests/golden/oracle_route_entropy.json,
    gen_oracle_route_entropy.py: 40 s per series) to the 1e-9 relative bar test_series_beyond_65535_samples holds it to there;
    approximate_entropy must be finite -- the reference cannot evaluate it at this length."""
    t0 = time.perf_counter()
    doc = json.load(open(os.path.join(HERE, "golden", "oracle_route_entropy.json")))
    params = {"sample_entropy": None, "approximate_entropy": [{"m": 2, "r": 0.3}]}
    variants = []
    for n in (17408, 17409):
        x = rc.series_at(n, doc["kind"], doc["seed"]).astype(dtype)
        records = []
        names, got = hip_engine(params, x, np.array([0, n], dtype=np.int64), launches=records)
        assert {r["family"] for r in records} == {"ENTROPY"}, records
        rec = rc.record_of(records, "ENTROPY")
        assert rec["max_len"] == n and rec["long_build"] == 1, rec
        variants.append(rec["variant"])
        want = float(doc["sample_entropy"][str(n)])
        g = got[0, names.index("value__sample_entropy")]
        print("\nsample_entropy %s n %d: got %r want %r rel %.3g" % (np.dtype(dtype).name, n, g, want, abs(g - want) / want))
        assert abs(g - want) <= 1e-9 * abs(want), (n, g, want)
        assert np.all(np.isfinite(got)), got
    assert variants[0] == 4 and variants[1] != 4, variants
    print("entropy %s: variants %s, %.1f s" % (np.dtype(dtype).name, variants, time.perf_counter() - t0))
