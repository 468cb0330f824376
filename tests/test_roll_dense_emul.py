"""tsfa_roll_count / tsfa_roll_fill without the device (tests/emul/emul_roll_dense.cpp: the host checks the driver shares with
it through csrc/roll_device.h, and the kernel bodies with one thread per workgroup over three workgroups), against
`roll_views` on the same lengths plus a phantom series of `steps` samples whose windows are dropped -- what
`extract_rolled_features` computes on the host.  Equality of (starts, ends, series, timeshifts) is exact; no case is skipped.

The bodies are grid-stride loops without LDS traffic, ballots or DPP (rl_count_body's one LDS word aside), so the emulation
sees all of their arithmetic, the division of the uniform route included.  What it does not see: the 1024-thread form of the
scan (`pk_blk_excl_sum` runs with one lane here), the streams, and the two-word read-back of the extent; those are
tests/test_roll_dense_gpu.py's."""
import itertools
import subprocess

import numpy as np
import pytest

import emul_roll_dense_lib as erd
from tsfresh_amd import _native
from tsfresh_amd.utilities.dataframe_functions import roll_views

DIRECTIONS = (1, -1, 2, -2, 3, -3)
MAX_TIMESHIFTS = (None, 1, 2, 4, 100)
MIN_TIMESHIFTS = (0, 1, 3, 7, 20)
SIZES = (1, 2, 3, 5, 8, 13)
# multisets of the six lengths: every single length, every pair (with itself too), and longer mixes in several orders
MULTISETS = [[a] for a in SIZES] + [list(c) for c in itertools.combinations_with_replacement(SIZES, 2)] + [
    [1, 2, 3, 5, 8, 13], [13, 8, 5, 3, 2, 1], [1, 1, 13, 1, 2, 2, 8, 1], [5, 5, 1, 13, 13, 3], [3] * 7, [13] * 4, [1] * 5]


def want(lengths, direction, mts, mn, steps, base=0):
    """(starts, ends, series, timeshifts) of the host route of extract_rolled_features."""
    lengths = np.asarray(lengths, dtype=np.int64)
    gi, frm, until, ts = roll_views(np.concatenate([lengths, [steps]]), direction, mts, mn)
    keep = gi < len(lengths)
    gi, frm, until, ts = gi[keep], frm[keep], until[keep], ts[keep]
    offsets = base + np.concatenate([[0], np.cumsum(lengths)])
    return offsets[gi] + frm, offsets[gi] + until, gi, ts


def _check(lengths, direction, mts, mn, steps, uniform=False, base=0, grid=3):
    got = erd.windows(lengths, direction, mts, mn, steps, uniform=uniform, base=base, grid=grid)
    assert not isinstance(got, int), "refused with %r: %r" % (got, (lengths, direction, mts, mn, steps, uniform))
    for g, w, what in zip(got, want(lengths, direction, mts, mn, steps, base), ("starts", "ends", "series", "timeshifts")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, lengths, direction, mts, mn, steps, uniform)
    return got


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_grid_equals_roll_views_on_both_routes(direction):
    n_cases = n_empty = 0
    for lengths in MULTISETS:
        same = len(set(lengths)) == 1
        for mts in MAX_TIMESHIFTS:
            for mn in MIN_TIMESHIFTS:
                ragged = _check(lengths, direction, mts, mn, max(lengths))
                n_cases += 1
                n_empty += len(ragged[0]) == 0
                if same:
                    # on uniform lengths the closed-form route equals the ragged route in all four arrays
                    uniform = _check(lengths, direction, mts, mn, max(lengths), uniform=True)
                    assert all(np.array_equal(u, r) for u, r in zip(uniform, ragged))
    assert n_cases == len(MULTISETS) * 25 and 0 < n_empty < n_cases


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_steps_above_the_longest_series(direction):
    """Another kind, or a longer batch, owns the longest series: the congruence class of the shifts follows `steps`."""
    for lengths in ([1, 2, 3, 5, 8, 13], [5, 5, 1, 13, 13, 3], [8] * 3, [13], [2] * 6):
        same = len(set(lengths)) == 1
        for steps in (max(lengths) + 1, max(lengths) + 2, max(lengths) + 16):
            for mts in MAX_TIMESHIFTS:
                for mn in MIN_TIMESHIFTS:
                    ragged = _check(lengths, direction, mts, mn, steps, base=11)
                    if same:
                        uniform = _check(lengths, direction, mts, mn, steps, uniform=True, base=11)
                        assert all(np.array_equal(u, r) for u, r in zip(uniform, ragged))


def test_no_window_writes_nothing():
    for uniform in (False, True):
        for direction in (1, -2):
            got = erd.windows([5, 5, 5], direction, 3, 4, 5, uniform=uniform)   # min_timeshift above max_timeshift
            assert all(len(a) == 0 for a in got)
            got = erd.windows([5, 5, 5], direction, None, 5, 5, uniform=uniform)  # min_timeshift at the length
            assert all(len(a) == 0 for a in got)
    # the fill itself: n_windows == 0 returns before a pointer is looked at
    offsets = np.arange(4, dtype=np.int64) * 5
    out = np.full((4, 8), erd.SENTINEL, dtype=np.int64)
    assert erd.fill(offsets, 3, 0, out, 1, None, 5, 5, series_len=5) == _native.TSFA_OK
    assert erd.fill(offsets, 3, 0, out, 1, None, 5, 5, scanned=np.zeros(3, dtype=np.uint32)) == _native.TSFA_OK
    assert (out == erd.SENTINEL).all()


@pytest.mark.parametrize("direction", (1, -1, 2, -3))
def test_many_short_series_cross_a_step_of_the_scan(direction):
    """5 000 series of 1 .. 3 samples: more than the 4 096 elements one step of the single-workgroup scan takes."""
    lengths = np.random.default_rng(2).integers(1, 4, size=5000)
    assert len(_check(lengths, direction, None, 0, 3, grid=7)[0]) > 4096 // abs(direction)
    _check(lengths, direction, 1, 1, 5, grid=7)


def test_uniform_route_with_more_windows_than_one_pass_of_the_grid():
    for direction in (1, -1, 3):
        got = _check([64] * 70, direction, 20, 0, 64, uniform=True, grid=2)
        if abs(direction) == 1:
            assert len(got[0]) == 70 * 64
        assert len(got[0]) % 70 == 0   # every series has the same windows


def test_refusals():
    inv, too_long, ok = _native.TSFA_ERR_INVALID, _native.TSFA_ERR_TOO_LONG, _native.TSFA_OK
    lengths = [5, 9, 3]
    for uniform_lengths, uniform in ((lengths, False), ([9, 9, 9], True)):
        assert erd.windows(uniform_lengths, 0, None, 0, 9, uniform=uniform) == inv      # direction 0
        assert erd.windows(uniform_lengths, 1, None, -1, 9, uniform=uniform) == inv     # negative min_timeshift
        assert erd.windows(uniform_lengths, 1, -2, 0, 9, uniform=uniform) == inv        # negative max_timeshift (0 means none)
        assert erd.windows(uniform_lengths, 1, None, 0, 8, uniform=uniform) == inv      # steps below the longest series
        assert erd.windows(uniform_lengths, -2, None, 0, 8, uniform=uniform) == inv
        assert not isinstance(erd.windows(uniform_lengths, 1, None, 0, 9, uniform=uniform), int)
    # 2^32 samples: an offsets array that only claims such an extent (nothing but its two ends is read before the refusal)
    scanned = np.zeros(1, dtype=np.uint32)
    claims = np.array([3, 3 + 2 ** 32], dtype=np.int64)
    assert erd.count(claims, 1, 1, None, 0, 2 ** 32, scanned=scanned) == (too_long, 0)
    claims[1] -= 1
    rc, n = erd.count(claims, 1, 1, 7, 7, 2 ** 32, scanned=scanned)                   # one sample fewer is taken
    assert rc == ok and n == 2 ** 32 - 1 - 7
    assert erd.count(claims[::-1].copy(), 1, 1, None, 0, 5, scanned=scanned) == (inv, 0)   # descending
    # the uniform route: n_series * series_len, without forming a product that could overflow
    assert erd.count(None, 2 ** 16, 1, None, 0, 2 ** 16, series_len=2 ** 16) == (too_long, 0)
    assert erd.count(None, 2 ** 40, 1, None, 0, 2 ** 40, series_len=2 ** 40) == (too_long, 0)
    assert erd.count(None, 65535, 1, None, 0, 65537, series_len=65537) == (ok, 65535 * 65537)
    assert erd.count(None, 3, 1, None, 0, 4, series_len=0) == (inv, 0)
    assert erd.count(None, -1, 1, None, 0, 4, series_len=4) == (inv, 0)
    # a window count that is not the batch's own is refused by the uniform fill
    offsets = np.arange(4, dtype=np.int64) * 5
    out = np.full((4, 32), erd.SENTINEL, dtype=np.int64)
    assert erd.fill(offsets, 3, 14, out, 1, None, 0, 5, series_len=5) == inv
    assert erd.fill(offsets, 3, 15, out, 1, None, 0, 5, series_len=5) == ok
    assert (out[:, 15:] == erd.SENTINEL).all() and (out[:, :15] != erd.SENTINEL).all()


def test_the_real_entries_without_a_device_are_an_error_not_a_cpu_route():
    if _native.device_count() > 0:
        # (a HIP device is present: direction 0 is refused before anything is launched)
        with pytest.raises(_native.NativeError) as ei:
            _native.roll_count(None, 3, rolling_direction=0, steps=5, series_len=5)
        assert ei.value.code == _native.TSFA_ERR_INVALID
        return
    for call in (lambda: _native.roll_count(None, 3, steps=5, series_len=5),
                 lambda: _native.roll_fill(None, 3, 0, None, None, None, None, steps=5, series_len=5)):
        with pytest.raises(_native.NativeError) as ei:
            call()
        assert ei.value.code == _native.TSFA_ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """The same source with its own main, built with AddressSanitizer and UBSan: one pass of the grid into heap blocks of
    exactly n_windows cells.  A process of its own; nothing sanitised is loaded into python."""
    exe = str(tmp_path / "emul_roll_dense_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DTSFA_EMUL", "-DRL_EMUL_MAIN",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", erd.SRC, "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0 and done.stdout.strip().endswith(", 0 failed") and done.stderr == "", (done.stdout, done.stderr)
