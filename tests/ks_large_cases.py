"""Test helper: the one table of (n1, n2, d) triples behind tests/test_select_ks_large_emul.py and
tests/test_select_ks_large_gpu.py, and the accuracy bar both hold tsfa_ks_large_tails to.

TEST INFRASTRUCTURE ONLY.  The product never imports this.
"""
import numpy as np

from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue

HOST_KS, KS_KOLMOGN = 5, 8
RUN = 16   # KSL_RUN of csrc/rel_ks_large.h: the emulation test compares it


def _seam(n, nxsq):
    """The smallest d with (n * d) * d >= nxsq, in float64 as kstwo.sf forms it."""
    d = np.sqrt(nxsq / n)
    while (n * d) * d >= nxsq:
        d = np.nextafter(d, 0.0)
    while (n * d) * d < nxsq:
        d = np.nextafter(d, 1.0)
    return float(d)


def _terms(n, k):
    """A d for which the sum has k terms: floor(n (1 - d)) + 1 == k."""
    return 1.0 - (k - 0.5) / n


def _below(d):
    return float(np.nextafter(d, 0.0))


# the rounded n = n1 n2 / (n1 + n2) of the pairs below
_N141, _N1100, _N5000, _N10K, _N20K, _N500K, _N1M = (10001, 143), (10001, 1236), (15000, 7500), (20000, 20000), (40000, 40000), \
    (10 ** 6, 10 ** 6), (2 * 10 ** 6, 2 * 10 ** 6)
EXACT, BAR = "exact", "bar"   # the host's 0.0 / 1.0 of a cut is met exactly; everything else to the relative bar

# (n1, n2, d, route, kind)
CASES = [
    # the serve rule
    ((10001, 142), 0.3, HOST_KS, None),                      # n = 140
    (_N141, 0.3, KS_KOLMOGN, BAR),                           # n = 141: the sum
    ((10000, 10000), 0.3, HOST_KS, None),                    # at most 10 000 rows: not this entry's
    (_N1M, float(np.sqrt(50.0 / 1e6)), KS_KOLMOGN, BAR),     # n at the cap
    ((2000002, 2000002), float(np.sqrt(50.0 / 1e6)), HOST_KS, None),   # n = 1 000 001
    (_N5000, float(np.sqrt(0.05 / 5000.0)), HOST_KS, None),  # Durbin's matrix
    # the closed branches
    (_N10K, 0.0, KS_KOLMOGN, EXACT),
    (_N10K, 1.0, KS_KOLMOGN, EXACT),
    (_N10K, 0.4 / 10000.0, KS_KOLMOGN, EXACT),               # t <= 0.5
    (_N10K, 0.75 / 10000.0, KS_KOLMOGN, BAR),                # t in (0.5, 1]
    (_N10K, 0.98 / 10000.0, KS_KOLMOGN, BAR),
    (_N141, 1.0 - 0.5 / 141.0, KS_KOLMOGN, BAR),             # t >= n - 1
    (_N10K, float(np.sqrt(0.3 / 1e4)), KS_KOLMOGN, BAR),     # Pelz-Good
    (_N10K, float(np.sqrt(1.0 / 1e4)), KS_KOLMOGN, BAR),
    (_N10K, float(np.sqrt(2.19 / 1e4)), KS_KOLMOGN, BAR),
    (_N500K, float(np.sqrt(0.05 / 5e5)), KS_KOLMOGN, BAR),   # Pelz-Good where n <= 100 000 would take Durbin's matrix
    # the seams
    (_N10K, _seam(1e4, 2.2), KS_KOLMOGN, BAR),               # the sum
    (_N10K, _below(_seam(1e4, 2.2)), KS_KOLMOGN, BAR),       # Pelz-Good
    (_N10K, _seam(1e4, 370.0), KS_KOLMOGN, EXACT),           # the cut
    (_N10K, _below(_seam(1e4, 370.0)), KS_KOLMOGN, BAR),     # the sum, a subnormal value
    (_N141, 0.5, KS_KOLMOGN, BAR),                           # x >= 0.5
    (_N141, _below(0.5), KS_KOLMOGN, BAR),
    (_N10K, 0.5, KS_KOLMOGN, BAR),                           # x >= 0.5 comes before the cut: 5 001 terms that underflow
    (_N10K, _below(0.5), KS_KOLMOGN, EXACT),
    (_N20K, float(np.sqrt(360.0 / 2e4)), KS_KOLMOGN, BAR),   # a subnormal value
] + [(_N141, _terms(141.0, k), KS_KOLMOGN, BAR) for k in (RUN - 1, RUN, RUN + 1, 63, 64, 65)] \
  + [(_N1100, _terms(1100.0, k), KS_KOLMOGN, BAR) for k in (64 * RUN - 1, 64 * RUN, 64 * RUN + 1)] \
  + [(pair, float(np.sqrt(-np.log(p / 2.0) / 2.0 / n)), KS_KOLMOGN, BAR)   # p near 1e-16, 1e-175, 1e-297
     for pair, n in ((_N20K, 2e4), (_N1M, 1e6)) for p in (1e-16, 1e-175, 1e-297)]

N1 = np.array([c[0][0] for c in CASES], dtype=np.int64)
N2 = np.array([c[0][1] for c in CASES], dtype=np.int64)
D = np.array([c[1] for c in CASES], dtype=np.float64)

_want = None


def host_values():
    """ks_2samp_pvalue of every served case (NaN for the others), computed once."""
    global _want
    if _want is None:
        _want = np.array([ks_2samp_pvalue(a, b, d) if route == KS_KOLMOGN else np.nan for (a, b), d, route, _ in CASES])
    return _want


def check(p, route):
    """Route bytes, and the bar of profiles/pvalue_floor.md: 1e-6 relative wherever the host's value is a normal double, equal
    where it is the 0.0 or 1.0 of a cut, inside [0, 2**-1021) where it is subnormal or has underflowed."""
    want = host_values()
    worst = 0.0
    for i, ((a, b), d, r, kind) in enumerate(CASES):
        what = "case %d: n1 %d n2 %d d %r: got p %r route %d, host %r" % (i, a, b, d, p[i], route[i], want[i])
        assert route[i] == r, what
        if r == HOST_KS:
            assert np.isnan(p[i]), what
        elif kind == EXACT:
            assert want[i] in (0.0, 1.0) and p[i] == want[i], what
        elif want[i] < 2.0 ** -1022:
            assert 0.0 <= p[i] < 2.0 ** -1021, what
        else:
            rel = abs(p[i] - want[i]) / want[i]
            worst = max(worst, rel)
            assert rel <= 1e-6, what
    print("largest relative error over the normal values: %.3g" % worst)
