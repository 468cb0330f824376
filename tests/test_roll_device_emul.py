"""The window builder's kernel bodies (csrc/roll_device.h: per-series count, the packer's scan, the fill), emulated with one
thread per workgroup (tests/emul/emul_roll.cpp), against `roll_views` on the same lengths plus a phantom series of `steps`
samples whose windows are dropped -- what `extract_rolled_features` computes on the host.  Equality of
(series, frm, until, ts) is exact; no case is skipped.

The bodies are grid-stride loops over series / windows: they use no LDS, no ballots and no DPP, so the emulation sees all
of their arithmetic.  What it does not see is the 1024-thread form of the scan they share with the packer (`pk_blk_excl_sum`
runs with one lane here); tests/test_roll_device_gpu.py checks the windows on the device."""
import numpy as np
import pytest

import emul_roll_lib
from tsfresh_amd import _native
from tsfresh_amd.utilities.dataframe_functions import roll_views

FIXED = [1, 2, 5, 33, 64, 65, 130]
RANDOM = np.random.default_rng(1).integers(1, 41, size=30).tolist()
DIRECTIONS = (1, -1, 3, -2)


def _want(lengths, direction, mts, mn, steps):
    gi, frm, until, ts = roll_views(np.concatenate([np.asarray(lengths, dtype=np.int64), [steps]]), direction, mts, mn)
    keep = gi < len(lengths)
    return gi[keep], frm[keep], until[keep], ts[keep]


def _check(lengths, direction, mts, mn, steps):
    got = emul_roll_lib.roll(lengths, direction, mts, mn, steps)
    assert not isinstance(got, int), "refused: %r" % ((direction, mts, mn, steps),)
    want = _want(lengths, direction, mts, mn, steps)
    for g, w, what in zip(got, want, ("series", "frm", "until", "ts")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, direction, mts, mn, steps)
    return len(want[0])


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("lengths", [FIXED, RANDOM], ids=["fixed", "random"])
def test_windows_equal_roll_views(lengths, direction):
    longest = max(lengths)
    counts = {}
    for steps in (longest, longest + 16):
        for mts in (None, 7, longest + 5):
            for mn in (0, 2, (mts or steps) + 1):
                counts[(steps, mts, mn)] = _check(lengths, direction, mts, mn, steps)
    assert all(n == 0 for (steps, mts, mn), n in counts.items() if mn == (mts or steps) + 1)   # min_timeshift > max_timeshift
    assert all(n > 0 for (steps, mts, mn), n in counts.items() if mn == 0)


def test_steps_above_the_longest_series_change_the_congruence():
    """Another kind owns the longest series: with direction 3 the shifts are those congruent to 47, not to 31, modulo 3."""
    lengths = [31, 20, 4, 31, 7]
    for mts, mn in ((None, 0), (12, 2), (7, 0)):
        _check(lengths, 3, mts, mn, 47)
        _check(lengths, -3, mts, mn, 47)
    a = emul_roll_lib.roll(lengths, 3, None, 0, 47)
    b = emul_roll_lib.roll(lengths, 3, None, 0, 31)
    assert set(a[3] % 3) == {47 % 3} and set(b[3] % 3) == {31 % 3} and 47 % 3 != 31 % 3


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_series_without_windows_between_series_with_some(direction):
    lengths = [10, 1, 1, 12, 2, 9, 3, 3, 40, 1]
    n = _check(lengths, direction, None, 4, 40)   # series of fewer than 5 samples have no window
    assert n > 0
    got = emul_roll_lib.roll(lengths, direction, None, 4, 40)
    assert set(got[0].tolist()) <= {0, 3, 5, 8}
    _check([1, 1, 6, 1], direction, 3, 2, 6)        # leading and trailing empty series


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_many_short_series(direction):
    """5 000 series of 1 .. 3 samples: the scan of the counts runs over more than one 4096-element step."""
    lengths = np.random.default_rng(2).integers(1, 4, size=5000)
    assert _check(lengths, direction, None, 0, 3) > 0
    _check(lengths, direction, 1, 1, 5)


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_more_than_4096_windows(direction):
    n = _check([64] * 70, direction, 20, 0, 64)
    if abs(direction) == 1:
        assert n == 70 * 64 > 4096


def test_argument_errors():
    lengths = [5, 9, 3]
    inv = _native.TSFA_ERR_INVALID
    assert emul_roll_lib.roll(lengths, 0, None, 0, 9) == inv      # direction 0
    assert emul_roll_lib.roll(lengths, 1, None, -1, 9) == inv     # negative min_timeshift
    assert emul_roll_lib.roll(lengths, 1, -2, 0, 9) == inv        # negative max_timeshift (0 means none)
    assert emul_roll_lib.roll(lengths, 1, None, 0, 8) == inv      # steps below the longest series
    assert emul_roll_lib.roll(lengths, -2, None, 0, 8) == inv
    assert not isinstance(emul_roll_lib.roll(lengths, 1, None, 0, 9), int)


@pytest.mark.parametrize("dtype", ["int64", "float64", "datetime64[ns]", "int32"])
def test_shift_values_name_the_window(dtype):
    lengths = np.array(RANDOM)
    total = int(lengths.sum())
    sort = np.random.default_rng(3).integers(0, 10 ** 6, size=total).astype(dtype)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for direction in DIRECTIONS:
        series, frm, until, ts, sv = emul_roll_lib.roll(lengths, direction, 7, 1, 40, sort=sort)
        row = offsets[series] + (until - 1 if direction > 0 else frm)
        assert np.array_equal(sv.view(sort.dtype), sort[row])
