"""matrix_profile with an explicit window on the CPU: the brute force of the definition (tests/mprofile_ref.py) against the
reference's pinned value, and the g++ build of k_mprofile's body (tests/emul/emul_mprofile.cpp) against the brute force."""
import numpy as np

import emul_mprofile_lib
import mprofile_cases as cases
import mprofile_ref

PINNED_MIN = 2.825786727580335   # tests/units/feature_extraction/test_feature_calculations.py:2060 of the reference


def test_pinned_min_of_the_references_unit_test():
    """The reference's own assertAlmostEqual (7 places) on its unit-test input with windows = 36, for both evaluations.
    Measured here: the brute force gives 2.8257867275803306 (4.4e-15 from the pinned value), the emulated kernel body
    2.8257867275803337 (1.3e-15 from it)."""
    x = mprofile_ref.reference_unit_test_input()
    brute = mprofile_ref.feature(mprofile_ref.profile(x, 36), "min")
    emul = emul_mprofile_lib.emul_mprofile([(36, "min")], x, [0, len(x)])[0, 0]
    print("brute force %r (%.1e off), emulation %r (%.1e off)" % (brute, abs(brute - PINNED_MIN), emul, abs(emul - PINNED_MIN)))
    assert round(abs(brute - PINNED_MIN), 7) == 0
    assert round(abs(emul - PINNED_MIN), 7) == 0


def test_brute_force_agrees_with_a_pairwise_evaluation_of_the_definition():
    """The helper itself, against np.corrcoef pair by pair on a series small enough for that."""
    rng = np.random.default_rng(5)
    x = np.round(rng.standard_normal(40), 1)
    x[20:26] = 1.5   # flat windows for w = 4, 5
    for w in (4, 5, 8):
        L, e = len(x) - w + 1, mprofile_ref.exclusion(w)
        want = np.full(L, np.nan)
        for i in range(L):
            a = x[i:i + w]
            if a.max() == a.min():
                continue
            best = -np.inf
            for j in range(L):
                b = x[j:j + w]
                if abs(i - j) > e and b.max() != b.min():
                    best = max(best, min(np.corrcoef(a, b)[0, 1], 1.0))
            if best > -np.inf:
                want[i] = np.sqrt(2 * w * (1 - best))
        got = mprofile_ref.profile(x, w)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=0, atol=1e-6)


def test_emulated_kernel_against_the_brute_force():
    """All six features, w in {4, 5, 8, 36, 64, 65}, on the edge lengths (no pair, one pair, two diagonals), the general
    lengths and every series kind.  No cell is skipped: every one is compared, NaN must meet NaN."""
    values, offsets = cases.small_batch()
    cols = cases.columns()
    got = emul_mprofile_lib.emul_mprofile(cols, values, offsets)
    want = cases.small_reference()
    assert not np.any(got == -12345.0)   # every cell written
    bad = cases.mismatches(got, want, cols, offsets)
    assert not bad, (len(bad), bad[:8])
    # the cases hold what they are there for
    assert np.isnan(want).any() and (want[~np.isnan(want)] < 1e-5).any()
    n_nan_rows = int(np.isnan(want).all(axis=1).sum())
    assert n_nan_rows >= 1   # the constant series


def test_edge_lengths_have_no_pair_then_one():
    cols = [(w, "max") for w in cases.WINDOWS]
    rng = np.random.default_rng(3)
    for c, (w, _) in enumerate(cols):
        e = mprofile_ref.exclusion(w)
        for extra, finite in ((1, False), (2, True)):
            x = rng.standard_normal(e + extra + w - 1)
            got = emul_mprofile_lib.emul_mprofile(cols, x, [0, len(x)])[0, c]
            assert np.isfinite(got) == finite, (w, extra, got)
        x = rng.standard_normal(w - 1)   # w > n
        assert np.isnan(emul_mprofile_lib.emul_mprofile(cols, x, [0, len(x)])[0, c])


def test_emulated_kernel_on_float32_input():
    values, offsets = cases.small_batch_f32()
    assert values.dtype == np.float32
    cols = cases.columns()
    got = emul_mprofile_lib.emul_mprofile(cols, values, offsets)
    bad = cases.mismatches(got, cases.small_reference_f32(), cols, offsets)
    assert not bad, (len(bad), bad[:8])
    # float32 samples are read as the float64 they convert to, exactly
    again = emul_mprofile_lib.emul_mprofile(cols, values.astype(np.float64), offsets)
    assert np.array_equal(got, again, equal_nan=True)


def test_a_series_gives_the_same_bits_alone_and_in_a_batch_and_whatever_the_column_order():
    values, offsets = cases.small_batch()
    cols = cases.columns()
    got = emul_mprofile_lib.emul_mprofile(cols, values, offsets)
    for s in (0, 7, len(offsets) - 2):
        x = values[offsets[s]:offsets[s + 1]]
        alone = emul_mprofile_lib.emul_mprofile(cols, x, [0, len(x)])
        assert np.array_equal(alone[0], got[s], equal_nan=True)
    order = np.random.default_rng(1).permutation(len(cols))
    shuffled = emul_mprofile_lib.emul_mprofile([cols[i] for i in order], values, offsets)
    assert np.array_equal(shuffled, got[:, order], equal_nan=True)


def test_error_of_rho_does_not_grow_with_the_length():
    """Bounded drift: a diagonal's covariance is recomputed every TSFA_MP_RESTART rows, so a planted exact repeat deep inside
    a long series (many updates after the diagonal's first cell) still gives P within the floor of 1e-12 in rho."""
    stride = emul_mprofile_lib.restart_stride()
    assert stride >= 64 and stride & (stride - 1) == 0
    rng = np.random.default_rng(11)
    n, w = 12 * stride, 16
    x = np.cumsum(rng.standard_normal(n)) * 100.0 + 1e4   # a drifting level: the hard case for a recurrence
    x[n - 3 * w:n - w] = x[n - 40 * w:n - 38 * w]          # the repeat ends near the last rows of its diagonal
    got = emul_mprofile_lib.emul_mprofile([(w, "min")], x, [0, n])[0, 0]
    want = mprofile_ref.feature(mprofile_ref.profile(x, w), "min")
    print("min of the profile: kernel body %.3e, brute force %.3e, floor %.3e" % (got, want, mprofile_ref.tolerance(w)[1]))
    assert mprofile_ref.close(got, want, w)
    assert got <= mprofile_ref.tolerance(w)[1]


def test_lds_threshold_is_between_the_lengths_the_device_tests_use():
    """The layout (tsfa_layout.h: MpLds) holds float64 series up to 3 332 samples and float32 up to 3 636 in a workgroup's
    160 KB; the device tests run 2048 (LDS) and 4096 / 21 000 (HBM scratch)."""
    assert emul_mprofile_lib.longest_in_lds(8) == 3332
    assert emul_mprofile_lib.longest_in_lds(4) == 3636
