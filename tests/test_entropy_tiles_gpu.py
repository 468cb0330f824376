"""The tiled route of sample_entropy / approximate_entropy with m = 2 (tsfresh_amd/csrc/tsfa_entropy_tiles.hip, plan option
ent_tiles, launch record variant 5): the ordered-pair sweep of a series cut into tiles of 256 sorted rows by C columns and
spread over the chip.  Its per-row results are integer counts and its tail is the pair sweep's own, so every cell must equal
the one-workgroup pair sweep of the long-series build (variant 0) with ==; the brute force of the definition holds both to
the float bar of tests/parity.py."""
import json
import os

import numpy as np
import pytest

import parity
import route_cases as rc
from engines import hip_engine

pytestmark = pytest.mark.gpu

C = 2048   # tsfa_entropy_tiles.hip: ENT_C, the columns of a tile
ROWS = (2, 3, 63, 64, 65, 255, 256, 257, 513, C - 1, C, C + 1, 2 * C + 1)   # n - 1: templates of length 2
PLANS = {"four": {"sample_entropy": None, "approximate_entropy": [{"m": 2, "r": r} for r in (0.1, 0.5, 0.9)]},
         "ten": {"sample_entropy": None, "approximate_entropy": [{"m": 2, "r": round(0.1 * k, 1)} for k in range(1, 10)]}}
PAIR_SWEEP = {"ent_tiles": 0, "entropy_route": 1, "force_long": 1}   # one workgroup per series from HBM scratch: variant 0


def _counts(x, m, tols):
    """C[k, i]: the templates j of length m within Chebyshev distance tols[k] of template i, over all pairs (i, j)."""
    t = np.lib.stride_tricks.sliding_window_view(x, m)
    out = np.zeros((len(tols), len(t)))
    for i0 in range(0, len(t), 256):
        d = np.abs(t[i0:i0 + 256, None, :] - t[None, :, :]).max(axis=2)
        for k, r in enumerate(tols):
            out[k, i0:i0 + 256] = (d <= r).sum(axis=1)
    return out


def _definition(names, x):
    """-log(A / B) and |phi(2) - phi(3)| of one float64 series from the brute-force counts."""
    n, sd = len(x), np.std(x)
    tols = [0.2 * sd if "sample_entropy" in c else parity._param(c, "r") * sd for c in names]
    c2, c3 = _counts(x, 2, tols), _counts(x, 3, tols)
    with np.errstate(all="ignore"):
        return np.array([-np.log((c3[k].sum() - (n - 2)) / (c2[k].sum() - (n - 1))) if "sample_entropy" in c
                         else 0.0 if n <= 3 else abs(np.log(c2[k] / (n - 1)).mean() - np.log(c3[k] / (n - 2)).mean())
                         for k, c in enumerate(names)])


def _edge_series():
    kinds = ("iid", "walk", "ints", "const")
    return [np.full(r + 1, 0.25, dtype=np.float32) if kinds[i % 4] == "const" else rc.series_at(r + 1, kinds[i % 4], 3)
            for i, r in enumerate(ROWS)]


def _run(params, values, offsets, options, variant):
    records = []
    names, got = hip_engine(params, values, offsets, options=options, launches=records)
    rec = rc.record_of(records, "ENTROPY")
    assert rec["variant"] == variant and rec["long_build"] == 1, records
    return names, np.array(got)


_reference = {}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_tile_edges(gpu, plan, dtype):
    """A single row, a partly filled wavefront, a row block and a column chunk just filled and just exceeded; noise, ties,
    windows that span every column (the integers 0 .. 3) and tolerance 0 (a constant series).  The plan of ten tolerances
    crosses the batch of eight once."""
    xs = _edge_series()
    values = np.concatenate(xs).astype(dtype)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    names, got = _run(PLANS[plan], values, offsets, {"ent_tiles": 1}, 5)
    _, want = _run(PLANS[plan], values, offsets, PAIR_SWEEP, 0)
    diff = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert len(diff) == 0, (len(diff), [(int(s), names[c], got[s, c], want[s, c]) for s, c in diff[:6]])
    if plan not in _reference:   # (the series are float32 values: one brute force serves both sample types)
        _reference[plan] = np.array([_definition(names, x.astype(np.float64)) for x in xs])
    ref = _reference[plan]
    assert all(len(xs[s]) <= 4 for s, _ in np.argwhere(~np.isfinite(ref))), np.argwhere(~np.isfinite(ref))
    bad = [(len(xs[s]), names[c], got[s, c], ref[s, c]) for s, c in np.argwhere(np.isfinite(ref))
           if not abs(got[s, c] - ref[s, c]) <= parity.RTOL * abs(ref[s, c]) + parity.atol_for(names[c], xs[s])]
    assert not bad, (len(bad), bad[:8])


def test_auto_takes_the_tiles_for_one_long_series(gpu):
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_route_entropy.json")))
    n = 17409   # the first length beyond the bit-matrix sweeps (TSFA_ENTH_MAXN + 1)
    x = rc.series_at(n, doc["kind"], doc["seed"]).astype(np.float64)
    offsets = np.array([0, n], dtype=np.int64)
    names, got = _run(PLANS["four"], x, offsets, None, 5)
    _, want = _run(PLANS["four"], x, offsets, {"ent_tiles": 0}, 0)
    assert np.array_equal(got, want) and np.all(np.isfinite(got)), (got, want)
    stored = float(doc["sample_entropy"][str(n)])
    assert abs(got[0, names.index("value__sample_entropy")] - stored) <= 1e-9 * abs(stored), (got, stored)


@pytest.mark.parametrize("n_series,variant", [(8, 5), (512, 0)], ids=["few", "a_chip_full"])
def test_auto_leaves_a_group_that_fills_the_chip_to_one_workgroup_per_series(gpu, n_series, variant):
    """Auto counts the series of the group against the device's CUs (256 on the MI355X): short series forced onto the
    long-series build take the tiles as a handful and stay on the pair sweep as 512."""
    values = np.tile(rc.series_at(48, "iid", 4), n_series)
    offsets = np.arange(n_series + 1, dtype=np.int64) * 48
    _, got = _run(PLANS["four"], values, offsets, {"force_long": 1}, variant)
    assert np.all(np.isfinite(got)) and np.all(got == got[0]), got[:3]


def test_ent_tiles_takes_auto_never_and_always(gpu):
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    plan = _native.Plan(compile_fc_parameters(PLANS["four"]).native_specs(_native.calc_id), device=0)
    try:
        for v in (-1, 0, 1):
            plan.set_option("ent_tiles", v)
        for v in (2, 0.5, -2):
            with pytest.raises(Exception):
                plan.set_option("ent_tiles", v)
    finally:
        plan.close()
