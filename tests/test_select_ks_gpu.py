"""The exact Kolmogorov-Smirnov tail on the device (`ks_tail="device"`, tsfresh_amd/csrc/rel_ks.h): `tsfa_ks_tails` on triples
against `ks_2samp_pvalue`, and the tensor selection with ks_tail="device" against ks_tail="host".

Every comparison of p-values is `==`: the Horner form and every lattice point are the host's float64 expressions, operand for
operand, so the device owes the host's bits.  The matrix of the chain tests is the 24-column recipe of test_select_tensor_gpu.py
(8 shifted normals, 4 rounded ones, 6 two-valued columns, one column with a single 1, a constant, 4 noise columns)."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch   # before the native library: one HIP runtime in the process, the one torch brings

from tsfresh_amd import _native
from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue
from tsfresh_amd.tensor_selection import (calculate_relevance_tensor, extract_relevant_features_tensor,
                                          select_features_tensor)

pytestmark = pytest.mark.gpu

HOST_KS, KS_EXACT = _native.TSFA_ROUTE_HOST_KS, _native.TSFA_ROUTE_KS_EXACT


def _exact(n1, n2, d):
    """The exact branch of ks_2samp_pvalue before its range check, by the host functions; None beyond 10 000 rows."""
    n1, n2 = int(n1), int(n2)
    if max(n1, n2) > 10000:
        return None
    g = math.gcd(n1, n2)
    h = int(round(d * ((n1 // g) * n2)))
    if h == 0:
        return 1.0
    if n1 != n2:
        return _native.ks_outer_prob(n1, n2, g, h)
    prob, k = 0.0, n1 // h
    while k >= 0:
        p1 = 1.0
        for j in range(h):
            p1 = (n1 - k * h - j) * p1 / (n1 + k * h + j + 1)
        prob = p1 * (1.0 - prob)
        k -= 1
    return 2.0 * prob


def _served(n1, n2, d):
    v = _exact(n1, n2, d)
    return v is not None and 0.0 <= v <= 1.0


def _from_h(m, n, h):
    lcm = (m // math.gcd(m, n)) * n
    d = h / lcm
    assert int(round(d * lcm)) == h
    return m, n, d


# band widths 1 .. 130 (the chunk seams), tiny tails, three rows, an empty band, both sides of the LDS-to-scratch crossover
# (rings of 16 and 17 chunks), wide bands in scratch, a band of about 400 columns at the largest samples the rule admits,
# either order of the samples; the Horner form with its fall-through (5, 5, h = 1); h == 0; beyond the rule
TRIPLES = [_from_h(*t) for t in [
    (145, 67, 73), (131, 130, 85), (131, 130, 4117), (131, 130, 4159), (131, 130, 4243), (131, 130, 8317), (131, 130, 8359),
    (131, 130, 8485), (138, 130, 4423), (129, 65, 129 * 65), (250, 100, 450), (200, 3, 300), (3, 200, 300), (97, 89, 1),
    (1030, 1029, 987290), (1030, 1029, 987291), (1029, 1030, 1030 * 1029), (5, 5, 1), (5, 5, 3), (130, 130, 7), (64, 64, 64),
    (1, 1, 1), (2000, 2000, 90)]] + [
    (10000, 9999, 0.02), (9999, 10000, 0.3), (40, 60, 0.004), (7, 7, 0.07), (10000, 3, 0.5), (10001, 3, 0.5), (3, 10001, 0.5),
    (10001, 10001, 0.1)]


def test_ks_tails_equal_the_host_function_on_triples():
    n1 = torch.tensor([t[0] for t in TRIPLES], dtype=torch.int64, device="cuda")
    n2 = torch.tensor([t[1] for t in TRIPLES], dtype=torch.int64, device="cuda")
    d = torch.tensor([t[2] for t in TRIPLES], dtype=torch.float64, device="cuda")
    p = torch.full((len(TRIPLES),), -1.0, dtype=torch.float64, device="cuda")
    route = torch.full((len(TRIPLES),), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _native.ks_tails(n1.data_ptr(), n2.data_ptr(), d.data_ptr(), len(TRIPLES), p.data_ptr(), route.data_ptr(),
                     device=torch.cuda.current_device())
    p, route = p.cpu().numpy(), route.cpu().numpy()
    want_route = [KS_EXACT if _served(*t) else HOST_KS for t in TRIPLES]
    assert route.tolist() == want_route
    assert want_route.count(HOST_KS) == 4   # (5, 5, h = 1) and the three beyond 10 000 rows
    for q, t in enumerate(TRIPLES):
        if want_route[q] == KS_EXACT:
            assert p[q] == ks_2samp_pvalue(*t), (t, p[q], ks_2samp_pvalue(*t))
        else:
            assert np.isnan(p[q]), t
    assert p[TRIPLES.index(_from_h(97, 89, 1))] == 1.0                  # the empty band
    assert 1e-53 < p[TRIPLES.index(_from_h(129, 65, 129 * 65))] < 1e-51
    assert p[TRIPLES.index((40, 60, 0.004))] == 1.0                     # h == 0


NAMES = ["shift%d" % j for j in range(1, 9)] + ["round%d" % j for j in range(1, 5)] + ["bin%d" % j for j in range(1, 7)] + [
    "single", "const", "noise1", "noise2", "noise3", "noise4"]
BINARY = [NAMES.index(f) for f in NAMES if f.startswith("bin") or f == "single"]
CONST = NAMES.index("const")
CHAIN = [(n, c) for n in (40, 300, 2049) for c in (0, 2, 3)]   # classes = 0: the regression


@functools.lru_cache(maxsize=None)
def _case(n, classes):
    rng = np.random.default_rng([n, classes, 1])
    if classes:
        y = rng.permutation(np.arange(n) % classes).astype(np.int64)
        s = (y == 0).astype(float) - (y == classes - 1).astype(float)
    else:
        y = np.round(rng.standard_normal(n), 1)
        s = (y - y.mean()) / y.std()
    cols = [rng.standard_normal(n) + 0.15 * j * s for j in range(1, 9)]
    cols += [np.round(rng.standard_normal(n) + 0.3 * j * s) for j in range(1, 5)]
    cols += [(0.4 * j * s + rng.standard_normal(n) > 0).astype(float) for j in range(1, 7)]
    single = np.zeros(n)
    single[int(rng.integers(n))] = 1.0
    cols += [single, np.full(n, 2.5)] + [rng.standard_normal(n) for _ in range(4)]
    X = np.ascontiguousarray(np.stack(cols, axis=1))
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _options(classes):
    return dict(test_for_binary_target_real_feature="smir", multiclass=classes > 2) if classes else {}


def _ks_cells(n, classes):
    """The Kolmogorov-Smirnov cells of the case and their triples, from the statistics sweep: {(column, table): (n1, n2, d)}."""
    X, y = _case(n, classes)
    if classes:
        stats = _native.relevance_classes(X, y.astype(np.int32), classes, device=torch.cuda.current_device(), with_ks=True)
        n_unique, ks_d = stats[0], stats[-1]
        class_n = np.bincount(y, minlength=classes)
        return {(j, k): (int(class_n[k]), int(n - class_n[k]), float(ks_d[j, k]))
                for j in range(len(NAMES)) if n_unique[j] > 2 for k in range(classes)}
    rec, _ = _native.relevance_real(X, y, device=torch.cuda.current_device())
    return {(j, 0): (int(rec["n_hi"][j]), int(n - rec["n_hi"][j]), float(rec["ks_d"][j]))
            for j in range(len(NAMES)) if rec["n_unique"][j] == 2}


def _run(n, classes, ks_tail, fn=calculate_relevance_tensor):
    X, y = _case(n, classes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # the constant column
        return fn(torch.from_numpy(X).cuda(), y, columns=NAMES, ks_tail=ks_tail, **_options(classes))


@pytest.mark.parametrize("n,classes", CHAIN)
def test_device_tail_equals_host_tail_through_the_chain(n, classes):
    host, dev = _run(n, classes, "host"), _run(n, classes, "device")
    cells = _ks_cells(n, classes)
    # the cells are the two-valued columns of the regression, the real columns of every class table under "smir"
    columns = sorted({j for j, _ in cells})
    assert columns == (BINARY if not classes else [j for j in range(len(NAMES)) if j not in BINARY and j != CONST])
    left = {cell for cell, t in cells.items() if not _served(*t)}   # the fall-through to kstwo, from the host function
    hr, dr = host.routes.cpu().numpy(), dev.routes.cpu().numpy()
    for (j, k), t in cells.items():
        assert hr[j, k] == HOST_KS
        assert dr[j, k] == (HOST_KS if (j, k) in left else KS_EXACT), (NAMES[j], k, t)
    other = np.ones_like(hr, dtype=bool)
    other[tuple(np.array(sorted(cells)).T)] = False
    assert (dr[other] == hr[other]).all()
    assert host.host_cells == len(cells) and dev.host_cells == len(left)
    # p-values with ==, NaN (the constant column) matching NaN
    hp, dp = host.p_values.cpu().numpy(), dev.p_values.cpu().numpy()
    assert np.array_equal(hp, dp, equal_nan=True), np.argwhere(~((hp == dp) | (np.isnan(hp) & np.isnan(dp))))
    for (j, k), t in cells.items():
        assert dp[j, k] == ks_2samp_pvalue(*t)
    for field in ("types", "relevant_per_table", "relevant", "n_significant"):
        assert torch.equal(getattr(host, field), getattr(dev, field)), field
    assert np.array_equal(host.p_value.cpu().numpy(), dev.p_value.cpu().numpy(), equal_nan=True)
    # the selection: the same columns, the same cells
    hs, ds = _run(n, classes, "host", select_features_tensor), _run(n, classes, "device", select_features_tensor)
    assert hs[1] == ds[1] and len(ds[1]) > 0
    assert torch.equal(hs[0], ds[0]) and torch.equal(hs[2], ds[2])


def test_fall_through_cells_stay_with_the_host():
    """Two classes of 5 rows each and a column whose distance is 1 / 5: the exact value is 1.0000000000000002, ks_2samp_pvalue
    falls through to kstwo, and the device leaves exactly that cell (both tables of it) to the host."""
    assert _exact(5, 5, 0.2) == 1.0000000000000002
    y = np.array([0, 1] * 5)
    far = np.arange(10.0) + 100.0 * y                      # d = 1
    near = np.array([0, 1, 2, 3, 4, 5, 7, 6, 8, 9.0])       # one swap of neighbours: d = 1 / 5
    X = torch.from_numpy(np.stack([far, near], axis=1)).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        host = calculate_relevance_tensor(X, y, test_for_binary_target_real_feature="smir", ks_tail="host")
        dev = calculate_relevance_tensor(X, y, test_for_binary_target_real_feature="smir", ks_tail="device")
    assert dev.routes.cpu().tolist() == [[KS_EXACT, KS_EXACT], [HOST_KS, HOST_KS]]
    assert dev.host_cells == 2 and host.host_cells == 4
    hp, dp = host.p_values.cpu().numpy(), dev.p_values.cpu().numpy()
    assert np.array_equal(hp, dp)
    assert dp[1, 0] == ks_2samp_pvalue(5, 5, 0.2) and dp[0, 0] == ks_2samp_pvalue(5, 5, 1.0)


def test_beyond_ten_thousand_rows_the_cell_stays_with_the_host():
    n = 10002
    rng = np.random.default_rng(5)
    y = rng.standard_normal(n)
    two = np.zeros(n)
    two[int(np.argmax(y))] = 1.0                            # 10 001 rows against 1
    served = (y > 0.3).astype(float)                        # both samples below the rule
    X = torch.from_numpy(np.stack([two, served, y + rng.standard_normal(n)], axis=1)).cuda()
    dev = calculate_relevance_tensor(X, y, ks_tail="device")
    host = calculate_relevance_tensor(X, y, ks_tail="host")
    assert dev.routes.cpu().view(-1).tolist() == [HOST_KS, KS_EXACT, _native.TSFA_ROUTE_KENDALL]
    assert host.routes.cpu().view(-1).tolist() == [HOST_KS, HOST_KS, _native.TSFA_ROUTE_KENDALL]
    assert dev.host_cells == 1 and host.host_cells == 2
    dp = dev.p_values.cpu().numpy()
    assert np.array_equal(dp, host.p_values.cpu().numpy())
    assert dp[0, 0] == ks_2samp_pvalue(1, 10001, 1.0)


def test_the_default_is_the_host_tail_and_a_bad_value_is_refused():
    n, classes = 300, 0
    X, y = _case(n, classes)
    Xd = torch.from_numpy(X).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        default = calculate_relevance_tensor(Xd, y, columns=NAMES)
    host = _run(n, classes, "host")
    assert torch.equal(default.routes, host.routes) and default.host_cells == host.host_cells == len(BINARY)
    assert (default.routes.cpu().numpy()[BINARY, 0] == HOST_KS).all() and not (default.routes == KS_EXACT).any()
    assert np.array_equal(default.p_values.cpu().numpy(), host.p_values.cpu().numpy(), equal_nan=True)
    for fn in (calculate_relevance_tensor, select_features_tensor):
        with pytest.raises(ValueError, match="ks_tail"):
            fn(Xd, y, ks_tail="gpu")
    with pytest.raises(ValueError, match="ks_tail"):
        extract_relevant_features_tensor(torch.zeros((4, 8), dtype=torch.float64), np.arange(4.0), ks_tail=None)
