"""number_cwt_peaks links ridge lines column by column for widths up to 5 (fam_cwt.h: cwt_link_columns); the general linker
(cwt_link_general: scipy's _identify_ridge_lines restated in parallel for any width) stays for wider plans and as the plan
option cwt_links = 0.  Both run here on the CPU through the device's LDS layout (tests/emul/emul_cwt_links.cpp), fed
relative-maximum masks directly, and must give the same entries (end column, end row) and the same row-0 marks: on random
non-adjacent masks at every width 1 .. 5 and length 3 .. 40, and on the constructed cases where the one row with link
distance 1 (row 3 under a start row 4) matters.  The entries are also held against scipy's own linker on the same mask."""
import numpy as np
import pytest

import emul_cwt_links_lib as ecl

DENSITIES = (0.05, 0.2, 0.35, 0.5, 0.8)


def _random_mask(rng, W, n, density):
    """Relative maxima are strict: never two neighbours in a row, never an end column.  Whole rows are emptied at random, so
    that the start row (the highest row with a maximum) lies below W - 1 and rows in between are gaps."""
    m = np.zeros((W, n), dtype=bool)
    for r in range(W):
        if rng.random() < 0.2:
            continue
        last = -2
        for c in range(1, n - 1):
            if c > last + 1 and rng.random() < density:
                m[r, c] = True
                last = c
    return m


def _scipy_entries(mask):
    """(end column, end row) of scipy's ridge lines of length >= ceil(W / 4) on a matrix whose relative maxima are `mask`."""
    from scipy.signal._peak_finding import _identify_ridge_lines
    W = mask.shape[0]
    if not mask.any():
        return []
    widths = np.arange(1, W + 1)
    lines = _identify_ridge_lines(mask.astype(np.float64), widths / 4.0, np.ceil(widths[0]))
    min_length = int(np.ceil(W / 4))
    return sorted((int(ln[1][0]), int(ln[0][0])) for ln in lines if len(ln[0]) >= min_length)


def _check(mask, scipy_too=True):
    W = mask.shape[0]
    for derive_w1 in (False, True):
        gen = ecl.links(mask, W, 0, derive_w1)
        col = ecl.links(mask, W, 1, derive_w1)
        assert not gen[2] and not col[2], (mask.astype(int), gen, col)   # three lines per column fit
        assert col[0] == gen[0], (derive_w1, mask.astype(int), col[0], gen[0])
        assert col[1] == gen[1], (derive_w1, mask.astype(int), col[1], gen[1])
        if derive_w1:   # the marked columns are the lines that end on row 0, and those are not listed
            assert all(r > 0 for _, r in col[0])
        else:
            assert col[1] == []
            plain = col[0]
    marked = ecl.links(mask, W, 1, True)
    assert sorted(marked[0] + [(c, 0) for c in marked[1]]) == plain
    if scipy_too:
        assert plain == _scipy_entries(mask), (mask.astype(int), plain)
    return plain


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
def test_random_masks_link_alike(W):
    rng = np.random.default_rng([20261021, W])
    seen_low_start = seen_start4 = 0
    for n in range(3, 41):
        for density in DENSITIES:
            for _ in range(6):
                mask = _random_mask(rng, W, n, density)
                _check(mask)
                rows = np.nonzero(mask.any(axis=1))[0]
                if len(rows) and rows[-1] < W - 1:
                    seen_low_start += 1
                if len(rows) and rows[-1] == 4:
                    seen_start4 += 1
    assert W == 1 or seen_low_start > 20
    assert W < 5 or seen_start4 > 200


@pytest.mark.parametrize("n", [5, 8, 9, 16, 17, 40])
@pytest.mark.parametrize("shift", [-1, 1])
def test_alternating_columns_that_shift_by_one_between_rows_4_and_3(n, shift):
    """Every line of row 4 sees a maximum on either side at row 3: p - 1 and p + 1 both choose p (the double chooser), the
    line grows by two and moves to p + 1; at the ends only one of them exists."""
    for low in range(8):   # every filling of rows 2 .. 0 with the row-3 pattern or nothing
        mask = np.zeros((5, n), dtype=bool)
        first = 1 if shift == 1 else 2
        mask[4, first:n - 1:2] = True
        mask[3, first + shift:n - 1:2] = True
        if shift == -1:
            mask[3, 0] = False
        for r in range(3):
            if (low >> r) & 1:
                mask[r] = mask[3]
        _check(mask)


@pytest.mark.parametrize("n", [5, 6, 7, 12, 33])
def test_a_maximum_between_two_lines_joins_the_left_one(n):
    """Lines in columns p - 2 and p, a row-3 maximum at p - 1 between them: a distance tie, the earlier line (the smaller
    column) wins, and the line at p goes without unless p + 1 is a maximum too."""
    for p in range(3, n - 1):
        for right in (False, True):
            for row3_self in (False, True):   # ... and with the left line's own column taken at row 3 there is no tie at all
                mask = np.zeros((5, n), dtype=bool)
                mask[4, p - 2] = mask[4, p] = True
                mask[3, p - 1] = True
                if right and p + 1 < n - 1:
                    mask[3, p + 1] = True
                if row3_self and p - 3 >= 1:
                    mask[3, p - 3] = True
                for low in range(8):
                    m2 = mask.copy()
                    for r in range(3):
                        if (low >> r) & 1:
                            m2[r, p - 1] = True
                    _check(m2)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 40])
def test_maxima_next_to_the_ends(W, n):
    """Columns 1 and n - 2 (the outermost a strict maximum can take): the neighbourhood reads of row 3 run off the series."""
    rng = np.random.default_rng([1, W, n])
    for _ in range(40):
        mask = np.zeros((W, n), dtype=bool)
        for r in range(W):
            for c in (1, n - 2, 2, n - 3):   # ... and the second column from either end, where its neighbours are free
                if 1 <= c <= n - 2 and not mask[r, c - 1] and not mask[r, c + 1] and rng.random() < 0.6:
                    mask[r, c] = True
        _check(mask)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5])
def test_an_empty_mask_has_no_lines(W):
    for n in (1, 2, 3, 17, 40):
        assert _check(np.zeros((W, n), dtype=bool)) == []


def test_two_entries_in_one_column():
    """A column can end two qualifying lines: one that retired and a later one.  Both are listed."""
    n = 40
    mask = np.zeros((4, n), dtype=bool)
    mask[3, 1:n - 1:2] = True     # lines of length 1 that retire on row 1 ...
    mask[0, 1:n - 1:2] = True     # ... and new ones in the same columns on row 0
    plain = _check(mask)
    assert len(plain) == 2 * len(range(1, n - 1, 2))
