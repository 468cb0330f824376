"""The exact Kolmogorov-Smirnov tail of the selection (tsfresh_amd/csrc/rel_ks.h), without a GPU: the g++ -DTSFA_EMUL build of
the bodies (tests/emul/emul_rel_ks.cpp, lanes looped) against a Python port of tsfa_ks_outer_prob's row walk, against scipy's
lattice function and against the Python text of ks_2samp_pvalue.  Every lattice point is one float64 expression of its two
predecessors, so the walk by anti-diagonals must give the row walk's value bit for bit: all comparisons are `==`."""
import math

import numpy as np
import pytest

import emul_rel_ks_lib as K
import emul_rel_tails_lib as E


def _limits(m, n, g, h, i):
    """minj(i), maxj(i) of tsfa_ks_outer_prob (m >= n), in exact integers."""
    mg, ng = m // g, n // g
    minj = min(max((ng * i - h) // mg + 1, 0), n)
    maxj = min(-((-(ng * i + h)) // mg), n + 1)
    return minj, maxj


def _width(m, n, h):
    """Columns of the widest row of the band."""
    if m < n:
        m, n = n, m
    g = math.gcd(m, n)
    return max(b - a for a, b in (_limits(m, n, g, h, i) for i in range(m + 1)))


def _row_walk(m, n, g, h):
    """tsfa_ks_outer_prob, line by line."""
    if m < n:
        m, n = n, m
    minj, maxj = _limits(m, n, g, h, 0)
    curlen = maxj - minj
    A = [1.0] * (n + 4)
    for j in range(minj, maxj):
        A[j] = 0.0
    for i in range(1, m + 1):
        lastminj, lastlen = minj, curlen
        minj, maxj = _limits(m, n, g, h, i)
        if maxj <= minj:
            return 1.0
        val = 0.0 if minj == 0 else 1.0
        for jj in range(maxj - minj):
            j = jj + minj
            val = (A[jj + minj - lastminj] * float(i) + val * float(j)) / float(i + j)
            A[jj] = val
        curlen = maxj - minj
        if lastlen > curlen:
            for q in range(maxj - minj, maxj - minj + (lastlen - curlen)):
                A[q] = 1.0
    return A[maxj - minj - 1]


def _scipy_walk(m, n, g, h):
    from scipy.stats._stats_py import _compute_outer_prob_inside_method
    if m < n:
        m, n = n, m
    return float(_compute_outer_prob_inside_method(m, n, g, h))


def _horner(n, h):
    """The n1 == n2 branch of ks_2samp_pvalue before its range check."""
    prob, k = 0.0, n // h
    while k >= 0:
        p1 = 1.0
        for j in range(h):
            p1 = (n - k * h - j) * p1 / (n + k * h + j + 1)
        prob = p1 * (1.0 - prob)
        k -= 1
    return 2.0 * prob


# (m, n, h, columns of the widest row): the chunk seams of the walk, 64 columns a chunk
WIDTHS = [(145, 67, 73, 1), (131, 130, 85, 2), (131, 130, 4117, 63), (131, 130, 4159, 64), (131, 130, 4243, 65),
          (131, 130, 8317, 127), (131, 130, 8359, 128), (138, 130, 4423, 129), (131, 130, 8485, 130)]


@pytest.mark.parametrize("m,n,h,width", WIDTHS)
def test_lattice_equals_the_row_walk_across_the_chunk_seams(m, n, h, width):
    assert _width(m, n, h) == width
    g = math.gcd(m, n)
    want = _row_walk(m, n, g, h)
    assert all(b > a for a, b in (_limits(m, n, g, h, i) for i in range(m + 1)))   # the walk runs: no empty row
    assert 0.0 < want <= 1.0
    assert _scipy_walk(m, n, g, h) == want
    for storage in (K.ANY, K.LDS, K.SCRATCH):
        assert K.lattice(m, n, g, h, storage) == want
    assert K.lattice(n, m, g, h) == want   # the swap of m < n


@pytest.mark.parametrize("m,n,h,order", [(129, 65, 129 * 65, 1e-53), (250, 100, 450, 1e-63), (200, 3, 300, None)])
def test_lattice_tiny_tails_and_a_three_row_sample(m, n, h, order):
    g = math.gcd(m, n)
    want = _row_walk(m, n, g, h)
    if order is not None:
        assert order < want < 100 * order
    assert _scipy_walk(m, n, g, h) == want
    for storage in (K.ANY, K.SCRATCH):
        assert K.lattice(m, n, g, h, storage) == want
        assert K.lattice(n, m, g, h, storage) == want


def test_lattice_empty_band_is_one():
    m, n, h = 97, 89, 1
    assert any(b <= a for a, b in (_limits(m, n, 1, h, i) for i in range(1, m + 1)))
    assert _row_walk(m, n, 1, h) == 1.0 and _scipy_walk(m, n, 1, h) == 1.0
    assert K.lattice(m, n, 1, h) == 1.0 and K.lattice(n, m, 1, h, K.SCRATCH) == 1.0


def test_lattice_on_both_sides_of_the_lds_to_scratch_crossover():
    """The ring needs (floor(2 h / (mg + ng)) + 1) // 64 + 2 chunks; the LDS slice holds lds_chunks() of them.  (1030, 1029):
    h = 987290 is the last that fits, 987291 the first that does not."""
    m, n = 1030, 1029
    lds = K.lds_chunks()
    for h, chunks in ((987290, lds), (987291, lds + 1)):
        assert K.ring_chunks(m, n, 1, h) == chunks == ((2 * h) // (m + n) + 1) // 64 + 2
        want = _scipy_walk(m, n, 1, h)
        assert K.lattice(m, n, 1, h, K.ANY) == want
        assert K.lattice(m, n, 1, h, K.SCRATCH) == want
        # the LDS-sized ring is refused, not overrun, where the driver would not choose it
        assert (K.lattice(m, n, 1, h, K.LDS) == want) if chunks <= lds else (K.lattice(m, n, 1, h, K.LDS) == -1.0)
    # the row walk itself at a band of about 1 000 columns, once
    assert _row_walk(m, n, 1, 987291) == _scipy_walk(m, n, 1, 987291)
    # the widest lattice the rule admits needs fewer chunks than the scratch slice holds
    assert K.ring_chunks(10000, 9999, 1, 10000 * 9999) <= 256


def test_horner_form_equals_the_python_text_for_every_h():
    from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue
    ns, hs = [], []
    for n in range(1, 131):
        for h in range(1, n + 1):
            ns.append(n)
            hs.append(h)
    ns, hs = np.array(ns), np.array(hs)
    d = hs / ns
    assert (np.rint(d * ns) == hs).all()
    p, route, left = K.ks_tails(ns, ns, d)
    want = np.array([_horner(int(n), int(h)) for n, h in zip(ns, hs)])
    served = (want >= 0.0) & (want <= 1.0)
    assert (route[served] == K.KS_EXACT).all() and (route[~served] == K.HOST_KS).all()
    assert (p[served] == want[served]).all() and np.isnan(p[~served]).all()
    assert left == int((~served).sum()) and left > 0
    # rounding pushes (5, 5, h = 1) an ulp past 1: the Python text falls through to kstwo, the cell stays with the host
    q = int(np.nonzero((ns == 5) & (hs == 1))[0][0])
    assert want[q] == 1.0000000000000002 and route[q] == K.HOST_KS
    for q in np.nonzero(served)[0][::97]:
        assert ks_2samp_pvalue(ns[q], ns[q], d[q]) == p[q]


def test_route_rule():
    n1 = [10000, 10001, 3, 10001, 40, 7, 0, 5, 12, 12]
    n2 = [3, 3, 10000, 10001, 60, 7, 4, 0, 30, 30]
    d = [0.5, 0.5, 0.5, 0.1, 0.004, 0.07, 0.5, 0.5, float("nan"), 1.5]
    p, route, left = K.ks_tails(n1, n2, d)
    want = [K.KS_EXACT, K.HOST_KS, K.KS_EXACT, K.HOST_KS, K.KS_EXACT, K.KS_EXACT, K.HOST_KS, K.HOST_KS, K.HOST_KS, K.HOST_KS]
    assert route.tolist() == want and left == want.count(K.HOST_KS)
    assert np.isnan(p[np.array(want) == K.HOST_KS]).all()
    # max(n1, n2) == 10 000 is served, on either side; 10 001 is not
    assert p[0] == p[2] == _scipy_walk(10000, 3, 1, int(round(0.5 * 30000)))
    # h == 0: round(0.004 * 120) and round(0.07 * 7)
    assert p[4] == 1.0 and p[5] == 1.0


def test_the_stage_serves_only_the_flagged_cells_of_the_tables():
    """Class tables under 'smir' and the table of a real target: rel_tails.h flags, the Kolmogorov-Smirnov stage fills in."""
    from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue
    # three columns (constant, two-valued, real) x three classes of 40 / 25 / 35 rows
    class_n = np.array([40, 25, 35])
    n_unique = np.array([1, 2, 50])
    ks_d = np.array([[0.0, 0.0, 0.0], [0.3, 0.2, 0.1], [0.25, 0.6, 0.013]])
    hi = np.array([[0, 0, 0], [20, 10, 5], [0, 0, 0]])
    p, route, typ, n_host = E.tails_classes(n_unique, np.zeros(3), np.zeros((3, 3)), hi, class_n, with_ks=True)
    assert n_host == 3 and route[2].tolist() == [E.HOST_KS] * 3
    before = p.copy()
    assert K.ks_stage_classes(class_n, ks_d, p, route) == 3
    assert route[2].tolist() == [K.KS_EXACT] * 3 and route[:2].tolist() == [[E.NONE] * 3, [E.FISHER] * 3]
    assert [p[2, k] for k in range(3)] == [ks_2samp_pvalue(class_n[k], 100 - class_n[k], ks_d[2, k]) for k in range(3)]
    assert np.array_equal(p[:2], before[:2], equal_nan=True)
    # real target, 100 rows: constant, two-valued (30 / 70), real, two-valued (50 / 50, the fall-through of n = 50, h = 1 if any)
    cols = np.zeros(4, dtype=E.REAL_COL_DTYPE)
    cols["n_unique"] = [1, 2, 80, 2]
    cols["n_hi"] = [0, 30, 0, 50]
    cols["ks_d"] = [0.0, 0.31, 0.0, 0.12]
    cols["xtie"], cols["dis"] = 10, 2000
    p, route, typ, n_host = E.tails_real(cols, 100, 0, 0.0, 0.0)
    assert n_host == 2 and route.tolist() == [E.NONE, E.HOST_KS, E.KENDALL, E.HOST_KS]
    kendall = p[2]
    assert K.ks_stage_real(cols, 100, p, route) == 2
    assert route.tolist() == [E.NONE, K.KS_EXACT, E.KENDALL, K.KS_EXACT]
    assert p[1] == ks_2samp_pvalue(30, 70, 0.31) and p[3] == ks_2samp_pvalue(50, 50, 0.12) and p[2] == kendall
