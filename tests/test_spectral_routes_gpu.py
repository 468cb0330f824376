"""Every rfft route of k_spectral against an exact DFT, at offsets too: the HIP kernels.  Truth, inputs and the derivation of
every bar: tests/spectral_truth.py; the same grid through the g++ build of the kernel sources, with the same forced
options: tests/test_spectral_routes_emul.py.  That both files pass with the same route table (spectral_truth.route_of) is
the evidence that the emulation and the device take the same route for every length of the grid: a series on another
route misses that route's bar by orders of magnitude at 2^30 (radix-2 against the centred routes) or takes bars a thousand
times apart (chirp-z against the sweeps).

One ragged batch per (dtype, build): "lds" holds the lengths a CU's LDS holds, "long" runs from the long-series build.  A
batch holds every length at every level of the dtype once (N(0,1) and the walk alternating): 140 / 84 series of at most
8197 samples, 40 / 24 of at most 65 536."""
import numpy as np
import pytest

import spectral_truth as st
from engines import hip_engine


def _run(cases, mode, dtype_name):
    values, offsets = st.pack(cases, np.dtype(dtype_name))
    return hip_engine(st.params(cases), values, offsets, options=st.MODE_OPTIONS[mode])


def _cases(dtype_name, build, mode):
    cases = st.batch(dtype_name, build)
    if mode != "default":   # a forced mode changes nothing for lengths with one route: only those with two run again
        cases = [c for c in cases if len({st.route_of(c.n, m) for m in st.MODES}) > 1]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("mode", st.MODES)
@pytest.mark.parametrize("build", ["lds", "long"])
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_every_route_meets_its_bar_at_every_level_on_the_device(gpu, dtype_name, build, mode):
    """default options; "bluestein": 0, so that the sweep is reached above the crossover on the same series; "bluestein_min":
    257, so that the chirp-z transform is reached below it.  The radix-2 bar is level-proportional by design (sum|x|, not
    sum|x - mean|): centring that route would change the bits of the headline path and is out of scope."""
    cases = _cases(dtype_name, build, mode)
    names, got = _run(cases, mode, dtype_name)
    worst = {}
    bad = st.check(names, got, cases, mode, worst=worst, what="device")
    print("\n" + st.worst_table([worst], ["device %s %s %s" % (dtype_name, build, mode)]))
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:8])
    assert {(r, lv) for (r, lv, _) in worst} == {(st.route_of(c.n, mode), c.level) for c in cases}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_a_series_gives_the_same_bits_alone_and_inside_the_batch(gpu, dtype_name):
    """One length per route (direct, radix-2, Goertzel, chirp-z in LDS; chirp-z and Reinsch from the long build), at the
    dtype's highest level: extracted alone -- a batch whose longest series it is, so the launch group is sized for it -- and
    inside the batch of its build."""
    for build, lengths in (("lds", (100, 1024, 896, 2053)), ("long", (32767, 32769))):
        cases = st.batch(dtype_name, build)
        names, got = _run(cases, "default", dtype_name)
        level = st.LEVELS[dtype_name][-1]
        picked = [i for i, c in enumerate(cases) if c.n in lengths and c.level == level]
        assert len(picked) == len(lengths)
        for i in picked:
            c = cases[i]
            # (the workgroup size follows the longest series of a launch group: beyond 2048 samples 512 threads, and the
            #  strided sums depend on it in the last bit -- alone means with the same company of longer series or none)
            if build == "lds" and c.n <= 2048:
                mates = [cases[i], next(m for m in cases if m.n == 8197 and m.level == level)]
            else:
                mates = [cases[i]]
            n2, alone = hip_engine(st.params(cases), *st.pack(mates, np.dtype(dtype_name)))
            assert n2 == names
            assert np.array_equal(alone[0], got[i], equal_nan=True), (c.label, np.flatnonzero(alone[0] != got[i])[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_welch_density_against_scipy_on_the_centred_base_on_the_device(gpu, dtype_name):
    """spkt_welch_density bins 2, 5, 8 on both sides of the 256-sample segment (blk_rfft's direct route below it, the batched
    128-point transform from it on) at level 0 and 2^24 (float32: the dtype's highest level takes its place)."""
    cases = st.welch_cases(dtype_name)
    values, offsets = st.pack(cases, np.dtype(dtype_name))
    names, got = hip_engine(st.WELCH_PARAMS, values, offsets)
    worst = {}
    bad = st.check_welch(names, got, cases, what="device", worst=worst)
    print("\nwelch, worst error / bar per level:", worst)
    assert not bad, bad[:8]
