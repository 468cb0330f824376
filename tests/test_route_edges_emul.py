"""The inputs of tests/test_route_edges_gpu.py on the CPU: the emulated kernel sources against the oracle, on the series and
parameter subsets of tests/route_cases.py at the last length whose carve fits LDS and the one after it (route_cases.LAST_IN_LDS;
on the CPU they are only representative lengths -- the emulation knows neither the long-series build nor the routing).  It
shows that the inputs and the oracle are sound before a GPU is involved, and it measures the share of cells the parity
predicates skip: they read the series alone, so the share measured here is the share the GPU test sees."""
import json
import os

import numpy as np
import pytest

import route_cases as rc
from engines import emul_engine, oracle_engine
from parity import compare

NAMES = list(rc.LAST_IN_LDS)

# Skipped cells of (three kinds at n, three at n + 1, twice the 300-sample series), measured here: none in any subset
# (0 of 832 BASIC, 488 TREND, 560 TREND_wide, 848 SORT, 3296 SPECTRAL, 216 AR, 16 CWT, 40 SEQ cells).  With `ints` in place
# of `wave` CWT would skip 4 of 16 (both columns of an integer series): route_cases.kinds_of.
SKIP_SHARE = {name: 0.0 for name in NAMES}


def both_sides(name):
    n = rc.LAST_IN_LDS[name]
    return rc.edge_batch(name, n) + rc.edge_batch(name, n + 1)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_kernels_match_the_oracle_on_both_sides_of_the_crossover(name):
    params = rc.subset(name)
    values, offsets, series = rc.batch(both_sides(name), np.float64)
    names, want = oracle_engine(params, values, offsets)
    gnames, got = emul_engine(params, values, offsets)
    assert gnames == names
    skipped = []
    bad = compare(names, got, want, series, skipped=skipped)
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:8])
    print("%s: %d of %d cells skipped" % (name, len(skipped), got.size))
    assert len(skipped) <= (SKIP_SHARE[name] + 0.02) * got.size, (len(skipped), got.size, skipped[:8])
    assert SKIP_SHARE[name] <= 0.05


def test_subsets_hold_their_family_alone():
    """The family column of TSFA_CALC_LIST is not visible from Python; the emulation's calculator ids are in the list's order,
    so at least every name resolves, no calculator sits in two subsets and the left-out ones are the documented ones."""
    from emul_lib import load
    from tsfresh_amd.feature_extraction import settings
    lib = load()
    seen = {}
    for fam in rc.FAMILIES:
        for calc in rc.family_params(fam):
            assert lib.tsfa_emul_calc_id(calc.encode()) >= 0, calc
            assert calc not in seen, (calc, fam, seen[calc])
            seen[calc] = fam
    left = set(settings.ComprehensiveFCParameters()) - set(seen)
    assert left == {"sample_entropy", "approximate_entropy", "linear_trend_timewise", "cwt_coefficients"}, left


def test_series_are_float32_values_and_prefixes_of_one_stream():
    for kind in rc.ALL_KINDS:
        a, b = rc.series_at(1000, kind), rc.series_at(1001, kind)
        assert a.dtype == np.float32 and np.array_equal(a, b[:1000])
        assert np.array_equal(a.astype(np.float64).astype(np.float32), a)
    walk = rc.series_at(5000, "walk").astype(np.float64)
    assert len(np.unique(walk)) < len(walk)                      # ties
    assert np.allclose(walk * 10, np.round(walk * 10), atol=1e-3)  # one decimal, as float32 holds it
    assert set(np.unique(rc.series_at(5000, "ints"))) == {0.0, 1.0, 2.0, 3.0}


def test_stored_sample_entropy_belongs_to_the_series_of_this_module():
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_route_entropy.json")))
    assert (doc["kind"], doc["seed"]) == ("iid", 0) and sorted(doc["sample_entropy"]) == ["17408", "17409"]
    assert all(np.isfinite(float(v)) and float(v) > 0 for v in doc["sample_entropy"].values())
