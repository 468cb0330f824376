#!/usr/bin/env python
"""Timing of the Kolmogorov-Smirnov tail beyond 10 000 rows of the tensor selection, host against device, in one process: writes
profiles/select_ks_large_timing.md.

  selection  --rows x --cols real columns, --classes classes, "smir" (every class against the rest: all cells lie beyond
             10 000 rows); every tenth column `normal + c_j s` with c_j graded from 0 to 0.2 (s: +1 on the first class, -1 on the
             last), the rest noise
    host          `select_features_tensor(..., ks_tail="host")` on the first --host-cols columns only: one `kstwo.sf` call per
                  cell, so the leg is capped at a column count that finishes in about a minute
    device_large  `select_features_tensor(..., ks_tail="device_large")` on the same columns, and on all of them
    flag / serve  the statistics sweep with the tails kernels on its own, cells only flagged / served: the difference is the stage
  kernels    `tsfa_ks_large_tails` on triples that all take one branch: the one-sided sum at n = 4 000, 100 000 and 1 000 000
             (n d^2 graded from 2.2 to 340), and Pelz-Good cells of the same count, whose time is the entry without `k_ksl_smirnov`
             (`k_ks_init`, `k_ksl_route`, the read-back); the difference is `k_ksl_smirnov` alone.  A sample of each batch is
             compared with `ks_2samp_pvalue`: the largest relative error per branch.
Host clock around calls that end synchronised, one warm-up round, then --runs rounds with the legs alternating; median and range.

    python profiles/select_ks_large_timing.py [--runs 5] [--rows 20000] [--cols 7880] [--host-cols 800]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_classification(torch, n, m, classes, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(20000 + m + classes)
    y = torch.randperm(n, generator=g, device=dev) % classes
    s = (y == 0).double() - (y == classes - 1).double()
    X = torch.randn((n, m), generator=g, device=dev, dtype=torch.float64)
    dep = torch.arange(m, device=dev) % 10 == 0
    coef = torch.zeros(m, dtype=torch.float64, device=dev)
    coef[dep] = torch.linspace(0.0, 0.2, int(dep.sum().item()), dtype=torch.float64, device=dev)
    X += s[:, None] * coef[None, :]
    return X, y.cpu().numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--cols", type=int, default=7880)
    ap.add_argument("--host-cols", type=int, default=800)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_ks_large_timing.md"))
    args = ap.parse_args()
    import torch

    from tsfresh_amd import _native, calculate_relevance_tensor, select_features_tensor
    from tsfresh_amd.feature_selection.significance_tests import ks_2samp_pvalue
    if _native.device_count() < 1:
        raise SystemExit("select_ks_large_timing.py needs a HIP device: nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    n, m, mh, C = args.rows, args.cols, args.host_cols, args.classes
    opts = dict(test_for_binary_target_real_feature="smir")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def rounds(title, legs):
        times, results = {name: [] for name, _ in legs}, {}
        for rnd in range(args.runs + 1):   # round 0 warms up
            for name, fn in legs:
                dt, results[name] = clock(fn)
                if rnd:
                    times[name].append(dt)
                print("%s round %d %s %.4f s" % (title, rnd, name, dt), flush=True)
        return times, results

    def cell(t):
        return "%.4f (%.4f .. %.4f)" % (statistics.median(t), min(t), max(t))

    with open(_native.LIB_PATH, "rb") as f:
        build_id = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["# The Kolmogorov-Smirnov tail beyond 10 000 rows of the tensor selection: host against device", "",
             "Written by `profiles/select_ks_large_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`." % (torch.cuda.get_device_name(0), build_id), "",
             "Host clock around calls that end synchronised, one warm-up round, %d timed rounds with the legs alternating; seconds, "
             "median (min .. max)." % args.runs, ""]

    # ---- the selection ----
    X, y = build_classification(torch, n, m, C, dev)
    Xh = X[:, :mh]   # a row-strided view: the host leg's columns
    codes = np.searchsorted(np.unique(y), y).astype(np.int32)
    p = torch.empty((m, C), dtype=torch.float64, device=dev)
    routes = torch.empty((m, C), dtype=torch.uint8, device=dev)
    types = torch.empty(m, dtype=torch.uint8, device=dev)

    def tails(ks_tail):
        return _native.relevance_tails_classes(X.data_ptr(), n, m, m, codes, C, p.data_ptr(), routes.data_ptr(), types.data_ptr(),
                                               with_ks=True, ks_tail=ks_tail)

    times, results = rounds("selection", [
        ("host", lambda: select_features_tensor(Xh, y, check_nan=False, ks_tail="host", **opts)),
        ("large", lambda: select_features_tensor(Xh, y, check_nan=False, ks_tail="device_large", **opts)),
        ("large_all", lambda: select_features_tensor(X, y, check_nan=False, ks_tail="device_large", **opts)),
        ("flag", lambda: tails("host")), ("serve", lambda: tails("device_large"))])
    res_h = calculate_relevance_tensor(Xh, y, check_nan=False, ks_tail="host", **opts)
    res_d = calculate_relevance_tensor(Xh, y, check_nan=False, ks_tail="device_large", **opts)
    res_a = calculate_relevance_tensor(X, y, check_nan=False, ks_tail="device_large", **opts)
    hp, dp = res_h.p_values.cpu().numpy(), res_d.p_values.cpu().numpy()
    big = hp >= 2.0 ** -1022
    rel = float((np.abs(dp[big] - hp[big]) / hp[big]).max())
    med = {k: statistics.median(v) for k, v in times.items()}
    lines += ["## Selection", "",
              "%d rows x %d real columns, %d classes, \"smir\": %d Kolmogorov-Smirnov cells, %d served on the device "
              "(`TSFA_ROUTE_KS_KOLMOGN`), %d left to the host.  The host leg and the leg beside it run on the first %d columns "
              "(%d cells, %d left to the host by `device_large`), a cap that keeps the host leg near a minute." % (
                  n, m, C, m * C, int((res_a.routes == _native.TSFA_ROUTE_KS_KOLMOGN).sum().item()), res_a.host_cells, mh, mh * C,
                  res_d.host_cells), "",
              "| leg | columns | seconds |", "|---|---|---|",
              "| `select_features_tensor(ks_tail=\"host\")` | %d | %s |" % (mh, cell(times["host"])),
              "| `select_features_tensor(ks_tail=\"device_large\")` | %d | %s |" % (mh, cell(times["large"])),
              "| `select_features_tensor(ks_tail=\"device_large\")` | %d | %s |" % (m, cell(times["large_all"])),
              "| flag: sweep + tails kernels, cells flagged | %d | %s |" % (m, cell(times["flag"])),
              "| serve: sweep + tails kernels, cells served | %d | %s |" % (m, cell(times["serve"])),
              "| the stage (serve minus flag) | %d | %.4f |" % (m, med["serve"] - med["flag"]), "",
              "On the %d columns the host leg takes %.2f ms a cell; the device leg is %.0f x faster there.  Largest relative "
              "difference of the p-values (host values that are normal doubles): %.3g; selection %s." % (
                  mh, 1e3 * med["host"] / (mh * C), med["host"] / med["large"], rel,
                  "equal" if results["host"][1] == results["large"][1] else "DIFFERENT"), ""]

    # ---- the kernels ----
    lines += ["## `tsfa_ks_large_tails` by branch", "",
              "| cells | n | branch | seconds | largest relative error (sample of 24 cells) |", "|---|---|---|---|---|"]
    rng = np.random.default_rng(1)
    for k, n1, n2, nn in ((39400, 20000, 5000, 4000.0), (4096, 200000, 200000, 100000.0), (512, 2000000, 2000000, 1000000.0)):
        a = torch.full((k,), n1, dtype=torch.int64, device=dev)
        b = torch.full((k,), n2, dtype=torch.int64, device=dev)
        pk = torch.empty(k, dtype=torch.float64, device=dev)
        rk = torch.empty(k, dtype=torch.uint8, device=dev)
        batches = [("the sum", np.sqrt(np.linspace(2.2001, 340.0, k) / nn)), ("Pelz-Good", np.sqrt(rng.uniform(0.3, 2.19, k) / nn))]
        legs, held = [], {}
        for name, dd in batches:
            held[name] = torch.from_numpy(dd).to(dev)
            legs.append((name, lambda t=held[name]: _native.ks_large_tails(a.data_ptr(), b.data_ptr(), t.data_ptr(), k, pk.data_ptr(),
                                                                           rk.data_ptr())))
        times, _ = rounds("n = %d" % nn, legs)
        for (name, dd), (_, fn) in zip(batches, legs):
            fn()
            torch.cuda.synchronize()
            assert bool((rk == _native.TSFA_ROUTE_KS_KOLMOGN).all().item())
            got, pick = pk.cpu().numpy(), np.linspace(0, k - 1, 24).astype(int)
            want = np.array([ks_2samp_pvalue(n1, n2, dd[i]) for i in pick])
            lines.append("| %d | %d | %s | %s | %.3g |" % (k, nn, name, cell(times[name]), (np.abs(got[pick] - want) / want).max()))
        lines.append("| %d | %d | `k_ksl_smirnov` alone (the sum minus Pelz-Good) | %.4f | |" % (
            k, nn, statistics.median(times["the sum"]) - statistics.median(times["Pelz-Good"])))
    lines.append("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
