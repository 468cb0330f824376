"""`-m gpu`: the level-invariant columns of exactly shifted series against the spread-scaled bound, on the device (the twin of
tests/test_shift_invariance.py; inputs, truth and bound: tests/shift_cases.py).

One extract per dtype: every shifted series x and every base b in one ragged batch.  Its longest series, 8197 samples (shift_cases.HBM_SIDE), puts
the sort and the entropy families on the HBM side of their crossover while the other families stay in LDS (a launch is sized
for its longest series: the 61 .. 2053-sample series ride in the same launches) -- asserted from the launch record.  The
LDS build of k_sort meets the refinement of change_quantiles in the short sawtooth batch, the HBM build in the long one.
The truth is the oracle on the bases, in worker processes: the entropies of the 8197-sample base dominate the wall time."""
import time

import numpy as np
import pytest

import parity
import route_cases as rc
import shift_cases as sc
from engines import hip_engine

pytestmark = pytest.mark.gpu
DTYPES = ("float64", "float32")
_memo = {}


def _bases(cs):
    """The distinct bases of the cases and, per case, the index of its own."""
    keys, bases, own = {}, [], []
    for c in cs:
        k = c.b.tobytes()
        if k not in keys:
            keys[k] = len(bases)
            bases.append(c.b)
        own.append(keys[k])
    return bases, own


def _device(dtype_name):
    """(cases, names, hip(x) rows, hip(b) rows per case, launch records) of the one extract of a dtype."""
    if dtype_name not in _memo:
        cs = sc.cases(dtype_name)
        bases, own = _bases(cs)
        values, offsets = sc.pack([c.x for c in cs] + bases, dtype=np.dtype(dtype_name))
        records = []
        names, got = hip_engine(sc.params(), values, offsets, launches=records)
        _memo[dtype_name] = (cs, names, got[:len(cs)], got[len(cs):][own], records)
    return _memo[dtype_name]


def _truth(dtype_name):
    if "truth" not in _memo:
        every = [c for d in DTYPES for c in sc.cases(d)]
        names, rows = sc.truth_of(every)
        _memo["truth"] = (names, {d: rows[[i for i, c in enumerate(every) if c.dtype_name == d]] for d in DTYPES})
    names, by = _memo["truth"]
    return names, by[dtype_name]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_device_holds_the_spread_scaled_bound(gpu, dtype_name):
    t0 = time.perf_counter()
    cs, names, got_x, got_b, records = _device(dtype_name)
    t_dev = time.perf_counter() - t0
    # the routes the batch was sized for: one launch group, 8197 samples at its longest
    longest = max(sc.LONG_LENGTHS)
    for fam in ("BASIC", "TREND", "SORT", "SPECTRAL", "AR", "CWT", "SEQ", "ENTROPY"):
        recs = [r for r in records if r["family"] == fam]
        assert recs, (fam, records)
        for r in recs:
            assert r["max_len"] == longest and r["length_class"] == 0, r
            hbm = fam == "ENTROPY" or longest > rc.LAST_IN_LDS[fam]
            assert r["long_build"] == (1 if hbm else 0), r
            if not hbm:
                assert r["lds_bytes"] <= 160 * 1024, r
    assert {r["family"] for r in records if r["long_build"] == 1} == {"SORT", "ENTROPY"}, records
    assert [r["variant"] for r in records if r["family"] == "ENTROPY"] == [4], records      # the bit table in HBM

    tnames, truth = _truth(dtype_name)
    assert tnames == names
    skipped, worst = [], {}
    bad = sc.compare_shift(names, got_x, truth, cs, skipped=skipped, worst=worst, what="hip")
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print("\n%s: device %.1f s, total %.1f s; largest error / bound: %s" % (dtype_name, t_dev, time.perf_counter() - t0, top))
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
    assert len(skipped) <= 0.02 * sc.n_invariant_cells(names, cs)
    assert not [col for _, col in skipped if parity.feature_of(col) in sc.MOMENTS], skipped[:8]
    # the base itself (no level at all) against the same truth, every invariant column
    bad = sc.compare_shift(names, got_b, truth, cs, what="hip-of-base")
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_device_values_do_not_move_with_the_level(gpu, dtype_name):
    """Tier A: hip(x) against hip(b), the device against itself -- no oracle in between."""
    cs, names, got_x, got_b, _ = _device(dtype_name)
    bad = sc.compare_shift(names, got_x, got_b, cs, only_tier="A", what="hip(x) against hip(b)")
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])


@pytest.mark.parametrize("side", ["lds", "hbm"])
def test_device_change_quantiles_of_a_jittered_sawtooth(gpu, side):
    """float64 sawtooth series: the 300- and 1000-sample ones (and the one moved to 2^20) through the LDS build of k_sort, the
    8197-sample ones through its HBM build; truth by exact rational arithmetic, 1e-6 relative, no floor."""
    cases = sc.sawtooth_cases(sc.SAW_LENGTHS if side == "lds" else (sc.SAW_LONG,))
    assert len(cases) == (9 + 4 if side == "lds" else 4 + 2)      # (+ the zig-zag series)
    values, offsets = sc.pack([x for _, x in cases])
    records = []
    names, got = hip_engine(sc.SAW_PARAMS, values, offsets, launches=records)
    assert {r["family"] for r in records} == {"SORT"}, records
    assert all(r["long_build"] == (0 if side == "lds" else 1) for r in records), records
    truth = np.array([sc.sawtooth_truth(x, names) for _, x in cases])
    worst = {}
    bad = sc.compare_sawtooth(names, got, truth, [label for label, _ in cases], worst=worst, what="hip")
    print("\nworst relative error:", {k[0]: "%.2g" % v for k, v in worst.items() if k[1] == "var"})
    assert max(len(x) for _, x in cases) == (max(sc.SAW_LENGTHS) if side == "lds" else rc.LAST_IN_LDS["SORT"] + 5)
    assert not bad, "%d cells, first: %s" % (len(bad), bad[:8])
