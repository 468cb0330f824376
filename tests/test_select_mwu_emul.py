"""The exact Mann-Whitney tail of the selection (tsfresh_amd/csrc/rel_mwu.h), without a GPU: the g++ -DTSFA_EMUL build of the
bodies (tests/emul/emul_rel_mwu.cpp, the threads of a phase looped) against `mannwhitney_pvalue`.  The counts are exact
integers and the quotient is the correctly rounded one, so every comparison is `==`.  p starts as NaN and the emulated buffers
as a garbage pattern: a word that was never written would show."""
import functools

import numpy as np
import pytest

import emul_rel_mwu_lib as M
from tsfresh_amd import _native
from tsfresh_amd.feature_selection.significance_tests import _mwu_exact_sf, mannwhitney_pvalue

HOST_MWU, MWU_EXACT, NORMAL = _native.TSFA_ROUTE_HOST_MWU_EXACT, _native.TSFA_ROUTE_MWU_EXACT, _native.TSFA_ROUTE_MWU_NORMAL
MAX_TOP = _native.TSFA_MWU_EXACT_MAX_TOP

# (m, n): one coefficient, chunks shorter than the stride, 65 and 73 coefficients on 512 threads, several coefficients a
# thread, both sides of the LDS-to-scratch crossover, counts beyond 2^64
TABLES = [(1, 1), (1, 9), (2, 3), (8, 8), (8, 9), (3, 2000), (8, 319), (8, 320), (5, 20000)]


def statistics(top, seed):
    """The k of a table: the ends, the middle, and eight draws."""
    return [0, 1, -(-top // 2), max(top - 1, 0), top, top + 1] + np.random.default_rng(seed).integers(0, top + 2, 8).tolist()


@functools.lru_cache(maxsize=None)
def want(k, n1, n2):
    """The host's p of the statistic k: through mannwhitney_pvalue where k can be its max(u1, u2), else by its two lines."""
    if 2 * k >= n1 * n2:
        return mannwhitney_pvalue(k + n1 * (n1 + 1) / 2.0, n1, n2, 0)
    return min(max(2.0 * _mwu_exact_sf(k, n1, n2), 0.0), 1.0)


def test_the_crossover_pair_straddles_the_lds_limit():
    assert 8 * 319 + 1 <= M.lds_elems() < 8 * 320 + 1


@pytest.mark.parametrize("m,n", TABLES)
def test_tails_equal_the_host_function(m, n):
    ks = statistics(m * n, [m, n])
    # table 0 is (m, n), table 1 (n, m); the last cell carries another route byte
    table = np.array([0, 1] * len(ks) + [0], dtype=np.int32)
    u = np.array([float(k) for k in ks for _ in (0, 1)] + [1.0])
    p = np.full(len(u), np.nan)
    route = np.full(len(u), HOST_MWU, dtype=np.uint8)
    route[-1] = NORMAL
    served = M.mwu_tails([m, n], [n, m], table, u, p, route)
    assert served == len(u) - 1
    assert (route[:-1] == MWU_EXACT).all() and route[-1] == NORMAL and np.isnan(p[-1])
    for q, k in enumerate(ks):
        assert p[2 * q] == want(k, m, n), (k, p[2 * q], want(k, m, n))
        assert p[2 * q + 1] == want(k, n, m), (k, p[2 * q + 1], want(k, n, m))
    assert p[2 * ks.index(m * n + 1)] == 0.0 and p[0] == 1.0


def test_the_cap_and_cells_left_alone():
    assert M.served(1, MAX_TOP) and M.served(8, MAX_TOP // 8) and not M.served(8, MAX_TOP // 8 + 1)
    assert not M.served(9, 9) and not M.served(0, 5)
    n1, n2 = [1, 8, 9], [MAX_TOP, MAX_TOP // 8 + 1, 100]
    table = np.array([0, 0, 1, 2, 3, -1], dtype=np.int32)   # the last two: no such table
    u = np.array([MAX_TOP - 3.0, float(MAX_TOP), 5.0, 500.0, 1.0, 1.0])
    p = np.full(6, np.nan)
    route = np.full(6, HOST_MWU, dtype=np.uint8)
    assert M.mwu_tails(n1, n2, table, u, p, route) == 2
    assert route.tolist() == [MWU_EXACT, MWU_EXACT] + [HOST_MWU] * 4 and np.isnan(p[2:]).all()
    assert p[0] == want(MAX_TOP - 3, 1, MAX_TOP) and p[1] == 2.0 * (1 / (MAX_TOP + 1))


def test_class_tables_from_rank_sums():
    """The stage as the chain runs it: table = cell mod classes, u from the rank sum; three classes of 4, 9 and 27 rows, so
    class 0 is served as (4, 36), class 1 is a normal-route class and class 2's complement has more than 8 rows too."""
    rng = np.random.default_rng(3)
    y = rng.permutation(np.repeat([0, 1, 2], [4, 9, 27]))
    X = rng.standard_normal((40, 6)) + 0.8 * (y == 0)[:, None]
    ranks = np.argsort(np.argsort(X, axis=0), axis=0) + 1.0
    rank_sums = np.stack([ranks[y == c].sum(axis=0) for c in range(3)], axis=1)
    route = np.tile(np.array([HOST_MWU, NORMAL, NORMAL], dtype=np.uint8), (6, 1))
    route[5, 0] = _native.TSFA_ROUTE_FISHER
    p = np.full((6, 3), np.nan)
    assert M.mwu_stage_classes([4, 9, 27], rank_sums, p, route) == 5
    assert (route[:5, 0] == MWU_EXACT).all() and route[5, 0] == _native.TSFA_ROUTE_FISHER and (route[:, 1:] == NORMAL).all()
    assert np.isnan(p[:, 1:]).all() and np.isnan(p[5, 0])
    for j in range(5):
        assert p[j, 0] == mannwhitney_pvalue(rank_sums[j, 0], 4, 36, 0)
