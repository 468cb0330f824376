"""ks_tail="device_large" on the GPU: tsfa_ks_large_tails (csrc/rel_ks_large.h) on the table of tests/ks_large_cases.py, and the
whole chain against ks_tail="host", where every Kolmogorov-Smirnov cell lies beyond 10 000 rows."""
import warnings

import numpy as np
import pytest
import torch   # before the native library: one HIP runtime in the process, the one torch brings

import ks_large_cases as cases
from tsfresh_amd import _native
from tsfresh_amd.tensor_selection import calculate_relevance_tensor, select_features_tensor

pytestmark = pytest.mark.gpu

# 10 400 rows: a class (or a column value) of 200 rows against 10 200 gives n = round(200 * 10200 / 10400) = 196; below 10 144
# rows no split has a sample beyond 10 000 rows and n >= 141
N_ROWS, N_RARE = 10400, 200


def test_ks_large_tails_meet_the_bar_on_triples():
    k = len(cases.CASES)
    n1, n2, d = (torch.from_numpy(a).cuda() for a in (cases.N1, cases.N2, cases.D))
    p = torch.full((k,), -1.0, dtype=torch.float64, device="cuda")
    route = torch.full((k,), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _native.ks_large_tails(n1.data_ptr(), n2.data_ptr(), d.data_ptr(), k, p.data_ptr(), route.data_ptr(),
                           device=torch.cuda.current_device())
    cases.check(p.cpu().numpy(), route.cpu().numpy())


def _chain_case(kind):
    """Six seeded columns; the p-values of the Kolmogorov-Smirnov cells are below 1e-24 or above 0.14, none is a Durbin cell."""
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
def test_device_large_tail_matches_host_tail_through_the_chain(kind):
    X, y, options, ks_cells = _chain_case(kind)
    Xd = torch.from_numpy(X).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        host = calculate_relevance_tensor(Xd, y, ks_tail="host", **options)
        dev = calculate_relevance_tensor(Xd, y, ks_tail="device_large", **options)
        kept = select_features_tensor(Xd, y, ks_tail="device_large", **options)
    assert host.host_cells == ks_cells and dev.host_cells == 0
    was_ks = host.routes == _native.TSFA_ROUTE_HOST_KS
    assert int(was_ks.sum()) == ks_cells and bool((dev.routes[was_ks] == _native.TSFA_ROUTE_KS_KOLMOGN).all())
    assert torch.equal(dev.routes[~was_ks], host.routes[~was_ks])
    hp, dp, ks = host.p_values.cpu().numpy(), dev.p_values.cpu().numpy(), was_ks.cpu().numpy()
    assert np.array_equal(dp[~ks], hp[~ks], equal_nan=True)
    rel = np.abs(dp[ks] - hp[ks]) / hp[ks]
    print("largest relative error: %.3g" % rel.max())
    assert (hp[ks] >= 2.0 ** -1022).all() and (rel <= 1e-6).all()
    assert torch.equal(dev.relevant, host.relevant) and torch.equal(dev.relevant_per_table, host.relevant_per_table)
    assert 0 < int(host.relevant.sum()) < 6
    assert kept[1] == torch.nonzero(host.relevant).view(-1).tolist()


def test_device_large_is_a_value_of_ks_tail_only():
    X, y = torch.zeros((4, 2), dtype=torch.float64), np.arange(4.0)
    with pytest.raises(ValueError, match="mwu_tail"):
        calculate_relevance_tensor(X, y, mwu_tail="device_large")
    with pytest.raises(ValueError, match="ks_tail"):
        calculate_relevance_tensor(X, y, ks_tail="device_huge")
