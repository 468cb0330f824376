"""tsfa_roll_count / tsfa_roll_fill on the device against their emulation (tests/emul/emul_roll_dense.cpp, itself checked against
`roll_views` by tests/test_roll_dense_emul.py): starts, ends, series and timeshifts are compared exactly, on both routes.  The
output buffers are torch allocations pre-filled with a sentinel and longer than n_windows: nothing beyond the last window
may be written.  What only the device shows: the 1024-thread scan and its carry, the second trip of the grid-stride loops, the
two-word read-back of the extent, a caller's stream."""
import numpy as np
import pytest
import torch

import emul_roll_dense_lib as erd
from tsfresh_amd import _native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCAN_SENTINEL = 0x5A5A5A5A


def _device_windows(lengths, direction, mts, mn, steps, uniform, base=0, stream=None):
    lengths = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    offsets = torch.from_numpy(base + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(DEV)
    kw = dict(rolling_direction=direction, max_timeshift=mts, min_timeshift=mn, steps=steps, device=0,
              stream=None if stream is None else stream.cuda_stream)
    scanned = None
    if uniform:
        kw["series_len"] = int(lengths[0])
    else:
        scanned = torch.full((B + erd.GUARD,), SCAN_SENTINEL, dtype=torch.int32, device=DEV)
        kw["scanned_ptr"] = scanned.data_ptr()
    torch.cuda.synchronize()
    n = _native.roll_count(offsets.data_ptr(), B, **kw)
    out = torch.full((4, n + erd.GUARD), erd.SENTINEL, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    _native.roll_fill(offsets.data_ptr(), B, n, *(out[k].data_ptr() for k in range(4)), **kw)
    if stream is not None:
        stream.synchronize()
    host = out.cpu().numpy()
    assert (host[:, n:] == erd.SENTINEL).all(), "a cell after the last window was written"
    if scanned is not None:
        assert (scanned[B:].cpu().numpy() == SCAN_SENTINEL).all(), "a cell after the last count was written"
    return tuple(host[k, :n] for k in range(4))


def _check(lengths, direction, mts, mn, steps, uniform, base=0, stream=None):
    want = erd.windows(lengths, direction, mts, mn, steps, uniform=uniform, base=base)
    assert not isinstance(want, int)
    got = _device_windows(lengths, direction, mts, mn, steps, uniform, base=base, stream=stream)
    for g, w, what in zip(got, want, ("starts", "ends", "series", "timeshifts")):
        assert np.array_equal(g, w), (what, list(lengths)[:8], direction, mts, mn, steps, uniform)
    return len(want[0])


def _subset(uniform):
    """60 cases of the CPU grid (tests/test_roll_dense_emul.py), every value of every axis among them."""
    from test_roll_dense_emul import DIRECTIONS, MAX_TIMESHIFTS, MIN_TIMESHIFTS, MULTISETS
    sets = [m for m in MULTISETS if (len(set(m)) == 1) == uniform]
    cases = []
    for k in range(60):
        lengths = sets[k % len(sets)]
        steps = max(lengths) + (0 if k % 4 else 5)
        cases.append((lengths, DIRECTIONS[k % 6], MAX_TIMESHIFTS[(k // 6 + k) % 5], MIN_TIMESHIFTS[(k // 2) % 5], steps))
    return cases


@pytest.mark.parametrize("uniform", (False, True), ids=("ragged", "uniform"))
def test_subset_of_the_grid_equals_the_emulation(gpu, uniform):
    cases = _subset(uniform)
    assert len(cases) == 60
    counts = [_check(*case, uniform=uniform, base=3) for case in cases]
    assert any(c == 0 for c in counts) and any(c > 0 for c in counts)


@pytest.mark.parametrize("direction", (1, -1, 2))
def test_many_short_series_cross_the_scans_carry(gpu, direction):
    lengths = np.random.default_rng(2).integers(1, 4, size=5000)
    assert _check(lengths, direction, None, 0, 3, uniform=False) > 4096 // abs(direction)


def test_more_windows_than_threads_in_the_grid(gpu):
    """600 x 1024 at min_timeshift 0: 614 400 windows, more than the 2048 x 256 threads of the largest grid, so the
    grid-stride loops of both fills take a second trip."""
    assert _check([1024] * 600, 1, None, 0, 1024, uniform=True) == 600 * 1024 > 2048 * 256
    assert _check([1024] * 600, -1, 100, 0, 1024, uniform=True) == 600 * 1024
    lengths = np.random.default_rng(5).integers(1, 1025, size=600)
    lengths[0], lengths[-1] = 1, 1024
    assert _check(lengths, 1, None, 0, 1024, uniform=False) == int(lengths.sum())
    assert _check([1024] * 600, 1, None, 0, 1024, uniform=False) == 600 * 1024 > 2048 * 256


@pytest.mark.parametrize("uniform", (False, True), ids=("ragged", "uniform"))
def test_on_a_callers_stream(gpu, uniform):
    stream = torch.cuda.Stream(device=0)
    lengths = [40] * 9 if uniform else [40, 3, 17, 1, 40, 22, 8, 8, 39]
    assert _check(lengths, 2, 12, 2, 40, uniform=uniform, stream=stream) > 0


def test_refusals_on_the_device(gpu):
    offsets = torch.tensor([0, 2 ** 32], dtype=torch.int64, device=DEV)   # only claims its extent: one uint32 of counts exists
    scanned = torch.full((1 + erd.GUARD,), SCAN_SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(_native.NativeError) as ei:
        _native.roll_count(offsets.data_ptr(), 1, steps=2 ** 32, scanned_ptr=scanned.data_ptr())
    assert ei.value.code == _native.TSFA_ERR_TOO_LONG
    assert (scanned.cpu().numpy() == SCAN_SENTINEL).all()   # refused before anything was launched
    with pytest.raises(_native.NativeError) as ei:
        _native.roll_count(None, 2 ** 16, steps=2 ** 16, series_len=2 ** 16)
    assert ei.value.code == _native.TSFA_ERR_TOO_LONG
    offsets = torch.tensor([0, 5, 14, 17], dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    for kw in (dict(rolling_direction=0, steps=9), dict(min_timeshift=-1, steps=9), dict(max_timeshift=-2, steps=9), dict(steps=8)):
        with pytest.raises(_native.NativeError) as ei:
            _native.roll_count(offsets.data_ptr(), 3, scanned_ptr=scanned.data_ptr(), **kw)
        assert ei.value.code == _native.TSFA_ERR_INVALID
    assert "below the batch's longest series (9 samples)" in str(ei.value)
