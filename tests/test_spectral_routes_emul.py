"""Every rfft route of k_spectral against an exact DFT, at offsets too: the g++ build of the kernel sources (tests/emul).
Truth, inputs and the derivation of every bar: tests/spectral_truth.py.  The device twin, same grid, same bars, same forced
options: tests/test_spectral_routes_gpu.py.

The whole grid runs here, the two Reinsch lengths (32 769, 32 770) included: none is left to the GPU file.  Where a length
has two routes it takes both: mode "bluestein_off" (TSFA_EMUL_BLUESTEIN=0) sends the chirp-z lengths down the Goertzel
sweep, mode "bluestein_min_257" (TSFA_EMUL_BLUESTEIN_MIN=257) the Goertzel lengths down the chirp-z transform.  The
emulation reads float64; a float32 case hands it the float32 values, which is what the device's float32 kernels see."""
import numpy as np
import pytest

import spectral_truth as st
from engines import emul_engine


def _run(cases, mode, monkeypatch):
    for k in ("TSFA_EMUL_BLUESTEIN", "TSFA_EMUL_BLUESTEIN_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in st.MODE_ENV[mode].items():
        monkeypatch.setenv(k, v)
    values, offsets = st.pack(cases, np.float64)
    return emul_engine(st.params(cases), values, offsets)


def _cases(dtype_name, build, mode):
    cases = st.batch(dtype_name, build)
    if mode != "default":   # a forced mode changes nothing for lengths with one route: only those with two run again
        cases = [c for c in cases if len({st.route_of(c.n, m) for m in st.MODES}) > 1]
    return cases


def test_truth_is_an_exact_dft():
    """dft_bins against a series whose DFT is known in closed form (a cosine of an exact bin: n / 2 there, 0 elsewhere; bin 0 of
    a constant: n times it) and against numpy on small well-conditioned input."""
    n = 1000
    j = np.arange(n)
    x = np.cos(2 * np.pi * 7 * j / n)
    re, im = st.dft_bins(x, [0, 1, 7, 50, 500])
    assert np.max(np.abs(np.array(re, dtype=np.float64) - [0, 0, n / 2, 0, 0])) < 1e-12    # (x itself is rounded to 1e-16 per sample)
    assert np.max(np.abs(np.array(im, dtype=np.float64))) < 1e-12
    x = np.random.default_rng(1).standard_normal(257).astype(np.float32)
    re, im = st.dft_bins(x, range(129))
    X = np.fft.rfft(x.astype(np.float64))
    assert np.max(np.abs(np.array(re, dtype=np.float64) - X.real)) < 1e-12 and np.max(np.abs(np.array(im, dtype=np.float64) - X.imag)) < 1e-12
    with pytest.raises(AssertionError):
        st.dft_bins(x.astype(np.float16), [0])


def test_route_table_has_every_route_on_both_sides_of_every_decision():
    r = {n: st.route_of(n) for b in st.LENGTHS for n in st.LENGTHS[b]}
    assert [r[n] for n in (255, 256, 257, 896, 897, 898, 1279, 1280, 1281, 1282)] == \
        ["direct", "radix2", "goertzel", "goertzel", "goertzel", "chirpz", "goertzel", "chirpz", "chirpz", "chirpz"]   # (1280: even, past 897)
    assert [r[n] for n in (32766, 32767, 32768, 65536, 32769, 32770)] == ["chirpz", "chirpz", "radix2", "radix2", "reinsch", "reinsch"]
    assert st.route_of(8197, "bluestein_off") == "goertzel" and st.route_of(257, "bluestein_min_257") == "chirpz"
    assert st.route_of(255, "bluestein_min_257") == "direct" and st.route_of(32769, "bluestein_min_257") == "reinsch"


@pytest.mark.parametrize("route,length", [("goertzel", 257), ("goertzel", 898), ("goertzel", 1282), ("reinsch", 32769)])
def test_restatement_constants_are_the_measured_ones(route, length):
    """The constants of the sweep bars come from the float64 numpy restatements of the recurrences, not from the kernel:
    re-measured here on a few lengths, they must be the figures written in spectral_truth.RESTATEMENT_WORST."""
    worst = (0.0, 0.0)   # (bins >= 1, bin 0)
    for dtype_name in ("float64", "float32"):
        for c in st.batch(dtype_name, "long" if length > 8197 else "lds"):
            if c.n == length:
                worst = tuple(max(w, r) for w, r in zip(worst, st.restatement_ratio(route, c)))
    assert all(abs(w - r) <= 0.01 * w for w, r in zip(worst, st.RESTATEMENT_WORST[route][length])), worst


@pytest.mark.parametrize("mode", st.MODES)
@pytest.mark.parametrize("build", ["lds", "long"])
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_every_route_meets_its_bar_at_every_level(dtype_name, build, mode, monkeypatch):
    cases = _cases(dtype_name, build, mode)
    names, got = _run(cases, mode, monkeypatch)
    worst = {}
    bad = st.check(names, got, cases, mode, worst=worst, what="emulation")
    print("\n" + st.worst_table([worst], ["emulation %s %s %s" % (dtype_name, build, mode)]))
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[:8])
    # every route the mode can reach was reached at every level
    assert {(r, lv) for (r, lv, _) in worst} == {(st.route_of(c.n, mode), c.level) for c in cases}


def test_welch_reference_is_level_free_and_the_bar_is_wide_enough_for_it():
    """The bar of the Welch test (1e-12 relative + 1e-13 max(pxx)) must hold between scipy's welch on the centred base and on x
    at level 0 -- where they are the same series: a bar the reference misses against itself would be wrong, not the kernel."""
    for c in st.welch_cases():
        if c.level == 0.0:
            assert np.array_equal(c.x, c.b)
            a, b = st.welch_reference(c.b), st.welch_reference(c.x)
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a) + 1e-13 * np.max(a))


def test_welch_density_against_scipy_on_the_centred_base():
    cases = st.welch_cases()
    values, offsets = st.pack(cases, np.float64)
    names, got = emul_engine(st.WELCH_PARAMS, values, offsets)
    worst = {}
    bad = st.check_welch(names, got, cases, what="emulation", worst=worst)
    print("\nwelch, worst error / bar per level:", worst)
    assert not bad, bad[:8]
    # constant detrend: the density does not move with the level (both levels of a base were held to ONE truth above)
    for i in range(0, len(cases), 2):
        assert np.array_equal(cases[i].b, cases[i + 1].b) and cases[i].level == 0.0 and cases[i + 1].level == 2.0 ** 24
