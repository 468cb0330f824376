"""The AR family runs one 64-lane wavefront per series for every launch group up to 2048 samples (fam_ar.h: packed
normal matrix, lag products generated in place, no workgroup barrier).  Checks its columns against the oracle at the
lengths around the old workgroup-size boundary (256) and the launch boundary (2048), on noise, random walks, a large
offset (the raw-design gate) and stuck-sensor designs (the condition estimate), and that a series gives the same bits
alone and inside batches of other longest lengths."""
import numpy as np
import pytest

from engines import hip_engine, oracle_engine
from parity import compare

LENGTHS = (3, 20, 255, 256, 257, 1000, 1024, 2047, 2048)

AR_PARAMS = {
    "agg_autocorrelation": [{"f_agg": s, "maxlag": 40} for s in ("mean", "median", "var")],
    "partial_autocorrelation": [{"lag": lag} for lag in range(10)],
    "ar_coefficient": [{"coeff": c, "k": 10} for c in range(5)] + [{"coeff": c, "k": 16} for c in (0, 8, 16)],
    "augmented_dickey_fuller": [{"attr": a} for a in ("teststat", "pvalue", "usedlag")],
}


def _series(rng, n, kind):
    if kind == "noise":
        return rng.standard_normal(n)
    if kind == "walk":
        return np.cumsum(rng.standard_normal(n))
    if kind == "offset":
        return 1e6 + rng.standard_normal(n)
    # stuck sensor: a noisy start, then a constant level
    head = min(n, 12)
    return np.concatenate([rng.standard_normal(head), np.full(n - head, 3.25)])


def _batch(series):
    offsets = np.zeros(len(series) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(s) for s in series])
    return np.concatenate(series).astype(np.float64), offsets


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noise", "walk", "offset", "stuck"])
def test_ar_columns_match_oracle_across_lengths(kind):
    rng = np.random.default_rng(2048 + len(kind))
    series = [_series(rng, n, kind) for n in LENGTHS for _ in range(2)]
    values, offsets = _batch(series)
    names, got = hip_engine(AR_PARAMS, values, offsets)
    onames, want = oracle_engine(AR_PARAMS, values, offsets)
    assert names == onames
    bad = compare(names, got, want, series)
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_ar_columns_do_not_depend_on_the_batch():
    rng = np.random.default_rng(7)
    probes = [rng.standard_normal(n) for n in (20, 255, 256, 257, 300)] + [np.cumsum(rng.standard_normal(280))]
    alone = []
    for x in probes:
        values, offsets = _batch([x])
        alone.append(hip_engine(AR_PARAMS, values, offsets)[1][0])
    for maxn in (300, 2000):
        fill = [rng.standard_normal(maxn)] + [rng.standard_normal(int(m)) for m in rng.integers(30, maxn, 5)]
        values, offsets = _batch(fill[:3] + probes + fill[3:])
        got = hip_engine(AR_PARAMS, values, offsets)[1]
        for i, want in enumerate(alone):
            np.testing.assert_array_equal(got[3 + i], want, err_msg="probe %d in a batch of maxn %d" % (i, maxn))
