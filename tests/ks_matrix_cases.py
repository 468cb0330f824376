"""Test helper: the one table of (n1, n2, d) triples behind tests/test_select_ks_matrix_gpu.py and
tests/test_select_ks_matrix_emul.py, and the accuracy bar of profiles/pvalue_floor.md that both hold tsfa_ks_matrix_tails to.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import numpy as np

from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue

HOST_KS, KS_MATRIX = 5, 9


def _last(n, nxsq):
    """The largest d with (n * d) * d <= nxsq, in float64 as kstwo.sf forms it; the next double is on the other side."""
    d = np.sqrt(nxsq / n)
    while (n * d) * d > nxsq:
        d = np.nextafter(d, 0.0)
    while (n * np.nextafter(d, 1.0)) * np.nextafter(d, 1.0) <= nxsq:
        d = np.nextafter(d, 1.0)
    return float(d)


def _up(d):
    return float(np.nextafter(d, 1.0))


def _small(n):
    """(10001, k) with rint(10001 k / (10001 + k)) == n."""
    k = next(k for k in range(n, n + 4) if np.rint(10001.0 * k / (10001.0 + k)) == n)
    return (10001, k)


_N5000, _N100K = (15000, 7500), (200000, 200000)
_D15 = (1.4 / 5000.0) ** (2.0 / 3.0)           # n d^1.5 == 1.4 at n = 5000, to an ulp or two
while 5000.0 * _D15 ** 1.5 > 1.4:
    _D15 = float(np.nextafter(_D15, 0.0))
while 5000.0 * _up(_D15) ** 1.5 <= 1.4:
    _D15 = _up(_D15)
_DMAX = (1.4 / 1e5) ** (2.0 / 3.0) * (1.0 - 1e-9)   # k = 59, m = 117: the largest matrix
EXACT, BAR = "exact", "bar"

# (n1, n2), d, route, kind.  Not reachable, so not here: m = 1 and floor(n d) = 0 (n d <= 1 is a closed branch), and a cell on
# either side of n d^2 == 2.2 with n d^1.5 <= 1.4 (for n >= 141 the second implies n d^2 < 0.72)
CASES = [
    # the serve rule
    (_small(1), 0.3, KS_MATRIX, EXACT), (_small(1), 0.8, KS_MATRIX, BAR), (_small(2), 0.7, KS_MATRIX, BAR),
    (_small(3), 0.55, KS_MATRIX, BAR),
    (_small(140), 0.3, KS_MATRIX, BAR),
    (_small(141), 0.3, HOST_KS, None),                       # the large stage's
    (_small(141), _last(141.0, 2.2), HOST_KS, None), (_small(141), _up(_last(141.0, 2.2)), HOST_KS, None),
    ((10000, 10000), 0.3, HOST_KS, None), ((10000, 20), 0.3, HOST_KS, None),
    (_N100K, _DMAX, KS_MATRIX, BAR),
    ((200002, 200002), _DMAX, HOST_KS, None),                # n = 100 001
    (_N5000, _D15, KS_MATRIX, BAR), (_N5000, _up(_D15), HOST_KS, None),
    # the closed branches
    (_small(20), 0.0, KS_MATRIX, EXACT), (_small(20), 1.0, KS_MATRIX, EXACT), (_small(20), 0.4 / 20.0, KS_MATRIX, EXACT),
    (_small(20), 0.75 / 20.0, KS_MATRIX, BAR), (_small(140), 1.0 / 140.0, KS_MATRIX, BAR),
    (_small(20), 1.0 - 0.5 / 20.0, KS_MATRIX, BAR),
    (_small(12), 0.5, KS_MATRIX, BAR), (_small(12), float(np.nextafter(0.5, 0.0)), KS_MATRIX, BAR),   # the sum | Pomeranz
] + [(_small(n), d, KS_MATRIX, BAR) for n in (20, 140) for v in (0.754693, 4.0) for d in (_last(float(n), v), _up(_last(float(n), v)))] + [
    # Durbin, small: m = 3; h = 0; h < 0.5; h > 0.5 (the largest k, 11, is the seam above)
    (_small(100), 0.015, KS_MATRIX, BAR), (_small(100), 0.05, KS_MATRIX, BAR), (_small(100), 0.047, KS_MATRIX, BAR),
    (_small(100), 0.042, KS_MATRIX, BAR),
    # Durbin, large: m = 15 | 17, 31 | 33; the cell ks_large_cases pins as a host cell; m = 3
    (_N5000, 7.5 / 5000.0, KS_MATRIX, BAR), (_N5000, 8.5 / 5000.0, KS_MATRIX, BAR), (_N5000, 15.5 / 5000.0, KS_MATRIX, BAR),
    (_N5000, 16.5 / 5000.0, KS_MATRIX, BAR), (_N5000, float(np.sqrt(0.05 / 5000.0)), KS_MATRIX, BAR),
    (_small(141), 1.5 / 141.0, KS_MATRIX, BAR),
    # Pomeranz: the fractional part of n d is 0, 0.5, below, above; n = 4 with floor(n d) = 1 (the widest row is the seam above)
    (_small(64), 0.125, KS_MATRIX, BAR), (_small(100), 0.125, KS_MATRIX, BAR), (_small(100), 0.122, KS_MATRIX, BAR),
    (_small(100), 0.128, KS_MATRIX, BAR), (_small(4), 0.45, KS_MATRIX, BAR),
]
N1 = np.array([c[0][0] for c in CASES], dtype=np.int64)
N2 = np.array([c[0][1] for c in CASES], dtype=np.int64)
D = np.array([c[1] for c in CASES], dtype=np.float64)
WANT = np.array([ks_2samp_pvalue(a, b, d) if route == KS_MATRIX else np.nan for (a, b), d, route, _ in CASES])


def check(p, route, skip=lambda case: False):
    """Route bytes, and the bar: 1e-6 relative wherever the host's value is a normal double, equal where it is the 0.0 or 1.0 of
    a cut.  skip(case): the served cases an emulation does not hold."""
    worst = 0.0
    for i, case in enumerate(CASES):
        (a, b), d, r, kind = case
        what = "case %d: n1 %d n2 %d d %r: got p %r route %d, host %r" % (i, a, b, d, p[i], route[i], WANT[i])
        if r == HOST_KS or skip(case):
            assert route[i] == HOST_KS and np.isnan(p[i]), what
            continue
        assert route[i] == r, what
        if kind == EXACT:
            assert WANT[i] in (0.0, 1.0) and p[i] == WANT[i], what
        else:
            worst = max(worst, abs(p[i] - WANT[i]) / WANT[i])
            assert abs(p[i] - WANT[i]) / WANT[i] <= 1e-6, what
    print("largest relative error over the normal values: %.3g" % worst)
