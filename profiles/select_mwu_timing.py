#!/usr/bin/env python
"""Timing of the exact Mann-Whitney tail of the tensor selection, host against device, in one process: writes
profiles/select_mwu_timing.md.

The rare-event shape: --rows x --cols untied normal columns, a binary target with 5 positives, then with 8; a tenth of the
columns shifted on the positives.  Every cell of both class tables is an exact Mann-Whitney cell.
  host    `select_features_tensor(..., mwu_tail="host")`: the flagged cells one at a time through `mannwhitney_pvalue`, which
          rebuilds the arrangement counts per cell.  The leg runs on the first --host-cols columns only: all of them would take
          minutes a round.
  device  `select_features_tensor(..., mwu_tail="device")`, on the same column subset and on all columns
Host clock around calls that end synchronised, one warm-up round, then --runs rounds with the legs alternating; the document holds
the median and the range of each leg.  The statistics sweep with the tails kernels is timed on its own with the cells only
flagged and with the cells served; the difference is the Mann-Whitney stage.  `tsfa_mwu_tails` on one cell times a table build.

    python profiles/select_mwu_timing.py [--runs 3] [--rows 20000] [--cols 2000] [--host-cols 50] [--out profiles/select_mwu_timing.md]
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


def build(torch, n, m, positives, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(20000 + m + positives)
    y = torch.zeros(n, dtype=torch.int64, device=dev)
    y[torch.randperm(n, generator=g, device=dev)[:positives]] = 1
    X = torch.randn((n, m), generator=g, device=dev, dtype=torch.float64)
    coef = torch.zeros(m, dtype=torch.float64, device=dev)
    dep = torch.arange(m, device=dev) % 10 == 0
    coef[dep] = torch.linspace(0.0, 4.0, int(dep.sum().item()), dtype=torch.float64, device=dev)
    X += y.double()[:, None] * coef[None, :]
    return X, y.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--cols", type=int, default=2000)
    ap.add_argument("--host-cols", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_mwu_timing.md"))
    args = ap.parse_args()
    import torch

    from tsfresh_amd import _native, calculate_relevance_tensor, select_features_tensor
    if _native.device_count() < 1:
        raise SystemExit("select_mwu_timing.py needs a HIP device: nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    n, m, mh = args.rows, args.cols, min(args.host_cols, args.cols)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with open(_native.LIB_PATH, "rb") as f:
        build_id = hashlib.sha256(f.read()).hexdigest()[:16]
    lines = ["# The exact Mann-Whitney tail of the tensor selection: host against device", "",
             "Written by `profiles/select_mwu_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`." % (torch.cuda.get_device_name(0), build_id), "",
             "Host clock around calls that end synchronised, one warm-up round, %d timed rounds with the legs alternating; seconds, "
             "median (min .. max).  The host leg runs on the first %d columns only (all %d would take minutes a round); the device "
             "leg runs on that subset and on all columns.  `flag` / `serve`: the statistics sweep with the tails kernels on its own "
             "(`tsfa_relevance_tails_classes`), all columns, the exact cells only flagged, or served on the device; their difference "
             "is the Mann-Whitney stage (`k_mwu_build`, `k_mwu_cells`, the allocations and one read-back of a counter).  `table`: "
             "`tsfa_mwu_tails` on one cell, i.e. one table build, one cell and the call's allocations." % (args.runs, mh, m), ""]

    for positives in (5, 8):
        X, y = build(torch, n, m, positives, dev)
        Xh = X[:, :mh].contiguous()
        codes = y.astype(np.int32)
        p = torch.empty((m, 2), dtype=torch.float64, device=dev)
        routes = torch.empty((m, 2), dtype=torch.uint8, device=dev)
        types = torch.empty(m, dtype=torch.uint8, device=dev)
        one_table = torch.zeros(1, dtype=torch.int32, device=dev)
        one_u = torch.full((1,), 0.75 * positives * (n - positives), dtype=torch.float64, device=dev)
        one_p = torch.empty(1, dtype=torch.float64, device=dev)

        def tails(mwu_tail):
            return _native.relevance_tails_classes(X.data_ptr(), n, m, m, codes, 2, p.data_ptr(), routes.data_ptr(), types.data_ptr(),
                                                   mwu_tail=mwu_tail)

        def table():
            one_route = torch.full((1,), _native.TSFA_ROUTE_HOST_MWU_EXACT, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            return _native.mwu_tails([positives], [n - positives], one_table.data_ptr(), one_u.data_ptr(), 1, one_p.data_ptr(),
                                     one_route.data_ptr())

        legs = [("host", lambda: select_features_tensor(Xh, y, check_nan=False, mwu_tail="host")),
                ("device", lambda: select_features_tensor(Xh, y, check_nan=False, mwu_tail="device")),
                ("device_all", lambda: select_features_tensor(X, y, check_nan=False, mwu_tail="device")),
                ("flag", lambda: tails("host")), ("serve", lambda: tails("device")), ("table", table)]
        times = {name: [] for name, _ in legs}
        results = {}
        for rnd in range(args.runs + 1):   # round 0 warms up
            for name, fn in legs:
                dt, out = clock(fn)
                results[name] = out
                if rnd:
                    times[name].append(dt)
                print("%d positives round %d %s %.4f s" % (positives, rnd, name, dt), flush=True)
        res_h = calculate_relevance_tensor(Xh, y, check_nan=False, mwu_tail="host")
        res_d = calculate_relevance_tensor(Xh, y, check_nan=False, mwu_tail="device")
        res_a = calculate_relevance_tensor(X, y, check_nan=False, mwu_tail="device")
        same_p = bool((res_h.p_values == res_d.p_values).all().item())
        same_sel = results["host"][1] == results["device"][1] and torch.equal(results["host"][0], results["device"][0])
        served = int((res_a.routes == _native.TSFA_ROUTE_MWU_EXACT).sum().item())

        def cell(name):
            t = times[name]
            return "%.4f (%.4f .. %.4f)" % (statistics.median(t), min(t), max(t))

        med = {k: statistics.median(v) for k, v in times.items()}
        top = positives * (n - positives)
        lines += ["## %d positives of %d rows" % (positives, n), "",
                  "%d untied columns, two class tables (%d, %d): %d coefficients of three limbs a table, both buffers in %s; "
                  "%d exact cells on the subset, %d on all columns, %d served on the device, %d left to the host; %d columns "
                  "selected of the subset, %d of all." % (
                      m, positives, n - positives, top + 1, "LDS" if top + 1 <= 2560 else "HBM scratch", res_h.host_cells, 2 * m,
                      served, res_a.host_cells, len(results["device"][1]), len(results["device_all"][1])), "",
                  "| leg | columns | seconds |", "|---|---|---|",
                  "| `select_features_tensor(mwu_tail=\"host\")` | %d | %s |" % (mh, cell("host")),
                  "| `select_features_tensor(mwu_tail=\"device\")` | %d | %s |" % (mh, cell("device")),
                  "| `select_features_tensor(mwu_tail=\"device\")` | %d | %s |" % (m, cell("device_all")),
                  "| flag: sweep + tails kernels, cells flagged | %d | %s |" % (m, cell("flag")),
                  "| serve: sweep + tails kernels, cells served | %d | %s |" % (m, cell("serve")),
                  "| the Mann-Whitney stage (serve minus flag) | %d | %.4f |" % (m, med["serve"] - med["flag"]),
                  "| table: `tsfa_mwu_tails`, one cell of (%d, %d) | | %s |" % (positives, n - positives, cell("table")), "",
                  "On the %d columns the device leg is %.1f x %s the host leg (%.4f s a host cell).  p-values %s, selection %s." % (
                      mh, max(med["host"], med["device"]) / min(med["host"], med["device"]),
                      "faster than" if med["device"] < med["host"] else "SLOWER than", med["host"] / max(res_h.host_cells, 1),
                      "equal (`==`)" if same_p else "DIFFERENT", "equal" if same_sel else "DIFFERENT"), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
