"""ks_tail="device_matrix" on the GPU: tsfa_ks_matrix_tails (csrc/rel_ks_matrix.h) on the table of tests/ks_matrix_cases.py, and the
whole chain against ks_tail="host", where every Kolmogorov-Smirnov cell has n = 60 beyond 10 000 rows."""
import warnings

import numpy as np
import pytest
import torch   # before the native library: one HIP runtime in the process, the one torch brings

import ks_matrix_cases as cases
from tsfresh_amd import _native
from tsfresh_amd.tensor_selection import calculate_relevance_tensor, select_features_tensor

pytestmark = pytest.mark.gpu

N_ROWS, N_RARE = 10200, 60   # n = round(60 * 10140 / 10200) = 60


def _tails(index):
    k = len(index)
    n1, n2, d = (torch.from_numpy(a[index]).cuda() for a in (cases.N1, cases.N2, cases.D))
    p = torch.full((k,), -1.0, dtype=torch.float64, device="cuda")
    route = torch.full((k,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _native.ks_matrix_tails(n1.data_ptr(), n2.data_ptr(), d.data_ptr(), k, p.data_ptr(), route.data_ptr(),
                            device=torch.cuda.current_device())
    return p.cpu().numpy(), route.cpu().numpy()


def test_ks_matrix_tails_meet_the_bar_on_triples_wherever_a_cell_stands():
    p, route = _tails(np.arange(len(cases.CASES)))
    cases.check(p, route)
    order = np.random.default_rng(5).permutation(len(cases.CASES))
    shuffled, _ = _tails(order)
    assert np.array_equal(shuffled.view(np.int64), p[order].view(np.int64))
    for i in np.flatnonzero(route == cases.KS_MATRIX)[[0, 3, -1, -9, -12]]:   # alone: a closed cell and one of every kernel
        assert _tails(np.array([i]))[0].view(np.int64)[0] == p.view(np.int64)[i]


def _chain_case(kind):
    """Six seeded columns; the host's p-values of the Kolmogorov-Smirnov cells are below 1e-6 or above 0.2 (the FDR thresholds
    of six columns lie between 0.0083 and 0.05)."""
    rng = np.random.default_rng(3)
    if kind == "smir":
        y = np.zeros(N_ROWS, dtype=np.int64)
        y[rng.choice(N_ROWS, N_RARE, replace=False)] = 1
        X = rng.standard_normal((N_ROWS, 6))
        X[y == 1, :3] += 1.0
        return X, y, dict(test_for_binary_target_real_feature="smir"), 12
    y = rng.standard_normal(N_ROWS)
    X = rng.standard_normal((N_ROWS, 6))
    X[:, 0] += y
    X[:, 1] -= 0.5 * y
    for col, shift in ((4, 1.0), (5, 0.0)):   # the two two-valued columns: one that moves the target, one that does not
        hi = rng.choice(N_ROWS, N_RARE, replace=False)
        X[:, col] = 0.0
        X[hi, col] = 1.0
        y[hi] += shift
    return X, y, {}, 2


@pytest.mark.parametrize("kind", ["smir", "real"])
def test_device_matrix_tail_matches_host_tail_through_the_chain(kind):
    X, y, options, ks_cells = _chain_case(kind)
    Xd = torch.from_numpy(X).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        host = calculate_relevance_tensor(Xd, y, ks_tail="host", **options)
        dev = calculate_relevance_tensor(Xd, y, ks_tail="device_matrix", **options)
        kept = select_features_tensor(Xd, y, ks_tail="device_matrix", **options)
    assert host.host_cells == ks_cells and dev.host_cells == 0
    was_ks = host.routes == _native.TSFA_ROUTE_HOST_KS
    assert int(was_ks.sum()) == ks_cells and bool((dev.routes[was_ks] == _native.TSFA_ROUTE_KS_MATRIX).all())
    assert torch.equal(dev.routes[~was_ks], host.routes[~was_ks])
    hp, dp, ks = host.p_values.cpu().numpy(), dev.p_values.cpu().numpy(), was_ks.cpu().numpy()
    assert np.array_equal(dp[~ks], hp[~ks], equal_nan=True)
    rel = np.abs(dp[ks] - hp[ks]) / hp[ks]
    print("largest relative error: %.3g" % rel.max(), "host p:", np.sort(hp[ks]))
    assert (hp[ks] >= 2.0 ** -1022).all() and (rel <= 1e-6).all()
    assert torch.equal(dev.relevant, host.relevant) and torch.equal(dev.relevant_per_table, host.relevant_per_table)
    assert 0 < int(host.relevant.sum()) < 6
    assert kept[1] == torch.nonzero(host.relevant).view(-1).tolist()
