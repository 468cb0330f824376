"""The exact Mann-Whitney tail on the device (`mwu_tail="device"`, tsfresh_amd/csrc/rel_mwu.h): `tsfa_mwu_tails` on tables and
statistics against `mannwhitney_pvalue`, and the tensor selection with mwu_tail="device" against mwu_tail="host".

Every comparison of p-values is `==`: the counts are exact integers and the quotient is the correctly rounded float64 of the
rational, which is what the host's `int / int` gives.  What the emulation (test_select_mwu_emul.py) cannot see is here: the
device's carries as compiled, the LDS and HBM layouts, the barriers between the passes."""
import functools
import warnings
from itertools import accumulate

import numpy as np
import pytest
import torch   # before the native library: one HIP runtime in the process, the one torch brings

from test_select_mwu_emul import TABLES, statistics, want
from tsfresh_amd import _native
from tsfresh_amd.feature_selection.significance_tests import _mwu_exact_sf
from tsfresh_amd.tensor_selection import (calculate_relevance_tensor, extract_relevant_features_tensor,
                                          select_features_tensor)

pytestmark = pytest.mark.gpu

HOST_MWU, MWU_EXACT = _native.TSFA_ROUTE_HOST_MWU_EXACT, _native.TSFA_ROUTE_MWU_EXACT
NORMAL, FISHER = _native.TSFA_ROUTE_MWU_NORMAL, _native.TSFA_ROUTE_FISHER
CAP = (8, _native.TSFA_MWU_EXACT_MAX_TOP // 8)   # total is about 2^128.7: the third limb carries


@functools.lru_cache(maxsize=None)
def tail_counts(m, n):
    """S_0 .. S_top of _mwu_exact_sf in exact integers, the stride-i sums by accumulate over slices instead of the index loop."""
    c = [1] + [0] * (m * n)
    for i in range(1, m + 1):
        c[n + i:] = [x - y for x, y in zip(c[n + i:], c)]
        for r in range(i):
            c[r::i] = accumulate(c[r::i])
    return list(accumulate(reversed(c)))[::-1]


def test_the_slice_form_of_the_reference_is_the_host_function():
    S = tail_counts(3, 2000)
    assert all(S[k] / S[0] == _mwu_exact_sf(k, 3, 2000) for k in statistics(6000, 0) if k <= 6000)


def _tails(n1, n2, table, u, route):
    dev = torch.cuda.current_device()
    table = torch.tensor(table, dtype=torch.int32, device="cuda")
    u = torch.tensor(u, dtype=torch.float64, device="cuda")
    p = torch.full((len(u),), float("nan"), dtype=torch.float64, device="cuda")
    route = torch.tensor(route, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    served = _native.mwu_tails(n1, n2, table.data_ptr(), u.data_ptr(), len(u), p.data_ptr(), route.data_ptr(), device=dev)
    return served, p.cpu().numpy(), route.cpu().numpy()


def test_mwu_tails_equal_the_host_function_on_every_table():
    """One call: every table in both orders of its samples (2 t: (m, n), 2 t + 1: (n, m)), then the table at the cap, a table
    beyond it, and a cell with another route byte.  The tables in LDS form and in scratch form are built by one launch."""
    n1 = [x for m, n in TABLES for x in (m, n)] + [CAP[0], 8]
    n2 = [x for m, n in TABLES for x in (n, m)] + [CAP[1], CAP[1] + 1]
    cells = [(2 * t + o, k) for t, (m, n) in enumerate(TABLES) for k in statistics(m * n, [m, n]) for o in (0, 1)]
    cells += [(2 * len(TABLES), k) for k in statistics(CAP[0] * CAP[1], 0)[:6]]
    left = [(2 * len(TABLES) + 1, 7), (0, 1)]
    route = [HOST_MWU] * (len(cells) + 1) + [NORMAL]
    served, p, got_route = _tails(n1, n2, [t for t, _ in cells + left], [float(k) for _, k in cells + left], route)
    assert served == len(cells)
    assert got_route.tolist() == [MWU_EXACT] * len(cells) + [HOST_MWU, NORMAL] and np.isnan(p[len(cells):]).all()
    S = tail_counts(*CAP)
    for q, (t, k) in enumerate(cells):
        expect = want(k, n1[t], n2[t]) if t < 2 * len(TABLES) else (min(2.0 * (S[k] / S[0]), 1.0) if k < len(S) else 0.0)
        assert p[q] == expect, (n1[t], n2[t], k, p[q], expect)


NAMES = ["normal%d" % j for j in range(1, 7)] + ["round%d" % j for j in range(1, 4)] + ["bin%d" % j for j in range(1, 4)]
UNTIED, TIED, TWO = list(range(6)), list(range(6, 9)), list(range(9, 12))
CHAIN = [(40, (37, 3)), (300, (292, 8)), (2049, (2044, 5)), (300, (150, 146, 4))]   # rows, rows of every class


@functools.lru_cache(maxsize=None)
def _case(n, class_n):
    rng = np.random.default_rng([n, len(class_n), 2])
    y = rng.permutation(np.repeat(np.arange(len(class_n)), class_n)).astype(np.int64)
    s = (y == len(class_n) - 1).astype(float)   # the small class
    cols = [rng.standard_normal(n) + 0.9 * j * s for j in range(1, 7)]
    cols += [np.round(rng.standard_normal(n) + j * s) for j in range(1, 4)]
    cols += [(j * s + rng.standard_normal(n) > 0.5).astype(float) for j in range(1, 4)]
    X = np.ascontiguousarray(np.stack(cols, axis=1))
    assert all(len(np.unique(X[:, j])) == n for j in UNTIED) and all(len(np.unique(X[:, j])) == 2 for j in TWO)
    return X, y


def _run(n, class_n, fn=calculate_relevance_tensor, **options):
    X, y = _case(n, class_n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return fn(torch.from_numpy(X).cuda(), y, columns=NAMES, multiclass=len(class_n) > 2, **options)


@pytest.mark.parametrize("n,class_n", CHAIN)
def test_device_tail_equals_host_tail_through_the_chain(n, class_n):
    host, dev = _run(n, class_n, mwu_tail="host"), _run(n, class_n, mwu_tail="device")
    hr, dr = host.routes.cpu().numpy(), dev.routes.cpu().numpy()
    # the exact cells: the untied columns in the tables of a class that has, or leaves, at most 8 rows
    small = [k for k, c in enumerate(class_n) if c <= 8 or n - c <= 8]
    exact = np.zeros_like(hr, dtype=bool)
    exact[np.ix_(UNTIED, small)] = True
    assert len(small) == (2 if len(class_n) == 2 else 1)
    assert (hr[exact] == HOST_MWU).all() and (dr[exact] == MWU_EXACT).all() and (dr[~exact] == hr[~exact]).all()
    assert (hr[TIED] == NORMAL).all() and (hr[TWO] == FISHER).all()
    assert host.host_cells == exact.sum() and dev.host_cells == 0
    hp, dp = host.p_values.cpu().numpy(), dev.p_values.cpu().numpy()
    assert not np.isnan(hp).any() and np.array_equal(hp, dp), np.argwhere(hp != dp)
    for field in ("types", "relevant_per_table", "relevant", "n_significant", "p_value"):
        assert torch.equal(getattr(host, field), getattr(dev, field)), field
    hs, ds = _run(n, class_n, select_features_tensor, mwu_tail="host"), _run(n, class_n, select_features_tensor, mwu_tail="device")
    assert hs[1] == ds[1] and len(ds[1]) > 0
    assert torch.equal(hs[0], ds[0]) and torch.equal(hs[2], ds[2])


def test_the_default_is_the_host_tail_and_a_bad_value_is_refused():
    n, class_n = 300, (292, 8)
    default, host = _run(n, class_n), _run(n, class_n, mwu_tail="host")
    assert torch.equal(default.routes, host.routes) and default.host_cells == host.host_cells == 2 * len(UNTIED)
    assert (default.routes[UNTIED] == HOST_MWU).all() and not (default.routes == MWU_EXACT).any()
    assert torch.equal(default.p_values, host.p_values)
    X, y = _case(n, class_n)
    for fn in (calculate_relevance_tensor, select_features_tensor):
        with pytest.raises(ValueError, match="mwu_tail"):
            fn(torch.from_numpy(X).cuda(), y, mwu_tail="gpu")
    with pytest.raises(ValueError, match="mwu_tail"):
        extract_relevant_features_tensor(torch.zeros((4, 8), dtype=torch.float64), np.array([0, 0, 1, 1]), mwu_tail=None)
