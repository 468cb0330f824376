#!/usr/bin/env python
"""Timing of the exact Kolmogorov-Smirnov tail of the tensor selection, host against device, in one process: writes
profiles/select_ks_timing.md.

Two shapes, both below the 10 000-row rule of the exact tail:
  regression      8 000 rows x 2 000 columns, a real target; a quarter of the columns two-valued, `(c_j s + normal > 0)` with
                  c_j graded from 0 to 0.6 over them (s: the standardised target), the rest `normal + 0.1 s`
  classification  8 000 rows x 2 000 real columns, five classes, "smir"; every tenth column `normal + c_j s` with c_j graded
                  from 0 to 0.5 (s: +1 on the first class, -1 on the last), the rest noise
  host    `select_features_tensor(..., ks_tail="host")`: the flagged cells one at a time through `ks_2samp_pvalue`
  device  `select_features_tensor(..., ks_tail="device")`
Host clock around calls that end synchronised, one warm-up round, then --runs rounds with the two legs alternating; the document
holds the median and the range of each leg, and the share of the tails kernels: the statistics sweep with the tails kernels is
timed on its own with the cells only flagged (`ks_tail="host"`, nothing copied) and with the cells served; the difference is the
Kolmogorov-Smirnov stage.

    python profiles/select_ks_timing.py [--runs 5] [--rows 8000] [--cols 2000] [--shape both] [--out profiles/select_ks_timing.md]
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


def build_regression(torch, n, m, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(8000 + m)
    y = torch.round(torch.randn(n, generator=g, device=dev, dtype=torch.float64), decimals=2)
    s = (y - y.mean()) / y.std()
    X = torch.randn((n, m), generator=g, device=dev, dtype=torch.float64)
    two = torch.arange(m, device=dev) % 4 == 0
    k = int(two.sum().item())
    coef = torch.full((m,), 0.1, dtype=torch.float64, device=dev)
    coef[two] = torch.linspace(0.0, 0.6, k, dtype=torch.float64, device=dev)
    X += s[:, None] * coef[None, :]
    X[:, two] = (X[:, two] > 0).double()
    return X, y.cpu().numpy()


def build_classification(torch, n, m, classes, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(8000 + m + classes)
    y = torch.randperm(n, generator=g, device=dev) % classes
    s = (y == 0).double() - (y == classes - 1).double()
    X = torch.randn((n, m), generator=g, device=dev, dtype=torch.float64)
    dep = torch.arange(m, device=dev) % 10 == 0
    coef = torch.zeros(m, dtype=torch.float64, device=dev)
    coef[dep] = torch.linspace(0.0, 0.5, int(dep.sum().item()), dtype=torch.float64, device=dev)
    X += s[:, None] * coef[None, :]
    return X, y.cpu().numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8000)
    ap.add_argument("--cols", type=int, default=2000)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--shape", choices=["regression", "classification", "both"], default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_ks_timing.md"))
    args = ap.parse_args()
    import torch

    from tsfresh_amd import _native, calculate_relevance_tensor, select_features_tensor
    from tsfresh_amd.feature_selection.significance_tests import target_tie_statistics
    if _native.device_count() < 1:
        raise SystemExit("select_ks_timing.py needs a HIP device: nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    n, m, C = args.rows, args.cols, args.classes

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with open(_native.LIB_PATH, "rb") as f:
        build_id = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["# The exact Kolmogorov-Smirnov tail of the tensor selection: host against device", "",
             "Written by `profiles/select_ks_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`." % (torch.cuda.get_device_name(0), build_id), "",
             "Host clock around calls that end synchronised, one warm-up round, %d timed rounds with the legs alternating; seconds, "
             "median (min .. max).  `flag` / `serve`: the statistics sweep with the tails kernels on its own "
             "(`tsfa_relevance_tails_*`), the Kolmogorov-Smirnov cells only flagged, or served on the device; their difference is the "
             "Kolmogorov-Smirnov stage (`k_ks_closed`, `k_ks_lattice` and their two read-backs of counters)." % args.runs, ""]

    shapes = []
    if args.shape in ("regression", "both"):
        X, y = build_regression(torch, n, m, dev)
        shapes.append(("Regression", "%d rows x %d columns, a real target, every fourth column two-valued" % (n, m), X, y, {}))
    if args.shape in ("classification", "both"):
        X, y = build_classification(torch, n, m, C, dev)
        shapes.append(("Classification", "%d rows x %d real columns, %d classes, \"smir\"" % (n, m, C), X, y,
                       dict(test_for_binary_target_real_feature="smir")))
    for title, what, X, y, opts in shapes:
        T = 1 if not opts else C
        p = torch.empty((m, T), dtype=torch.float64, device=dev)
        routes = torch.empty((m, T), dtype=torch.uint8, device=dev)
        types = torch.empty(m, dtype=torch.uint8, device=dev)
        codes = None if not opts else np.searchsorted(np.unique(y), y).astype(np.int32)

        def tails(ks_tail):
            if opts:
                return _native.relevance_tails_classes(X.data_ptr(), n, m, m, codes, T, p.data_ptr(), routes.data_ptr(),
                                                       types.data_ptr(), with_ks=True, ks_tail=ks_tail)
            return _native.relevance_tails_real(X.data_ptr(), n, m, m, y, target_tie_statistics, p.data_ptr(), routes.data_ptr(),
                                                types.data_ptr(), ks_tail=ks_tail)

        legs = [("host", lambda: select_features_tensor(X, y, check_nan=False, ks_tail="host", **opts)),
                ("device", lambda: select_features_tensor(X, y, check_nan=False, ks_tail="device", **opts)),
                ("flag", lambda: tails("host")), ("serve", lambda: tails("device"))]
        times = {name: [] for name, _ in legs}
        results = {}
        for rnd in range(args.runs + 1):   # round 0 warms every shape up
            for name, fn in legs:
                dt, out = clock(fn)
                results[name] = out
                if rnd:
                    times[name].append(dt)
                print("%s round %d %s %.4f s" % (title, rnd, name, dt), flush=True)
        res_h = calculate_relevance_tensor(X, y, check_nan=False, ks_tail="host", **opts)
        res_d = calculate_relevance_tensor(X, y, check_nan=False, ks_tail="device", **opts)
        same_p = bool(((res_h.p_values == res_d.p_values) | (res_h.p_values.isnan() & res_d.p_values.isnan())).all().item())
        same_sel = results["host"][1] == results["device"][1] and torch.equal(results["host"][0], results["device"][0])
        served = int((res_d.routes == _native.TSFA_ROUTE_KS_EXACT).sum().item())

        def cell(name):
            t = times[name]
            return "%.4f (%.4f .. %.4f)" % (statistics.median(t), min(t), max(t))

        med = {k: statistics.median(v) for k, v in times.items()}
        lines += ["## %s" % title, "",
                  "%s; %d Kolmogorov-Smirnov cells, %d served on the device, %d left to the host; %d columns selected." % (
                      what, res_h.host_cells, served, res_d.host_cells, len(results["device"][1])), "",
                  "| leg | seconds |", "|---|---|",
                  "| `select_features_tensor(ks_tail=\"host\")` | %s |" % cell("host"),
                  "| `select_features_tensor(ks_tail=\"device\")` | %s |" % cell("device"),
                  "| flag: sweep + tails kernels, cells flagged | %s |" % cell("flag"),
                  "| serve: sweep + tails kernels, cells served | %s |" % cell("serve"),
                  "| the Kolmogorov-Smirnov stage (serve minus flag) | %.4f |" % (med["serve"] - med["flag"]), "",
                  "The device leg is %.1f x %s the host leg; the tails kernels with the Kolmogorov-Smirnov stage are %.0f %% of it.  "
                  "p-values %s, selection %s." % (
                      max(med["host"], med["device"]) / min(med["host"], med["device"]),
                      "faster than" if med["device"] < med["host"] else "SLOWER than",
                      100.0 * (med["serve"] - med["flag"]) / med["device"],
                      "equal (`==`)" if same_p else "DIFFERENT", "equal" if same_sel else "DIFFERENT"), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
