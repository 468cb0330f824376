"""linear_trend_timewise on a series of ONE sample: scipy's linregress raises nothing there and returns rvalue 0.0 next to four
NaN (the variance of one sample is zero, which it tests before it divides), and so does the kernel -- a ragged tensor batch
with `times=` meets such series (tests/test_tensor_times_gpu.py).  Series of two and three samples ride along."""
import numpy as np
import pytest

from engines import emul_engine, hip_engine, oracle_engine
from parity import compare

PARAMS = {"linear_trend_timewise": [{"attr": a} for a in ["pvalue", "rvalue", "intercept", "slope", "stderr"]]}
LENGTHS = np.array([1, 2, 3, 1, 5])
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
VALUES = np.random.default_rng(2).standard_normal(int(LENGTHS.sum()))
HOURS = np.concatenate([np.cumsum(np.random.default_rng(3 + i).uniform(0.1, 2.0, size=L)) for i, L in enumerate(LENGTHS)])
HOURS -= np.repeat(HOURS[OFFSETS[:-1]], LENGTHS)


def _check(engine):
    names, want = oracle_engine(PARAMS, VALUES, OFFSETS, times=HOURS)
    got_names, got = engine(PARAMS, VALUES, OFFSETS, times=HOURS)
    assert got_names == names
    rvalue = names.index('value__linear_trend_timewise__attr_"rvalue"')
    for row in (0, 3):
        assert want[row, rvalue] == 0.0 and got[row, rvalue] == 0.0
        assert np.isnan(np.delete(want[row], rvalue)).all() and np.isnan(np.delete(got[row], rvalue)).all()
    bad = compare(names, got, want, [VALUES[OFFSETS[i]:OFFSETS[i + 1]] for i in range(len(LENGTHS))])
    assert not bad, bad


def test_emulation_matches_the_oracle():
    _check(emul_engine)


@pytest.mark.gpu
def test_hip_matches_the_oracle(gpu):
    _check(hip_engine)
