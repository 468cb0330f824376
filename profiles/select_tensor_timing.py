#!/usr/bin/env python
"""Timing of the selection step on one device, in one process: writes profiles/select_tensor_timing.md.

The matrix is 20 000 rows x 7 880 columns (ten kinds of ComprehensiveFCParameters), five classes, "mann": the 24 test columns of
tests/test_select_tensor_gpu.py tiled with fresh noise, built on the device with a seeded generator.
  before  the device-resident chain of `extract_relevant_features`: `_relevance_table` on a `DeviceMatrix` (statistics on the
          device, tails and FDR on the host, per cell in Python) + `to_host` of the selected columns;
  after   `select_features_tensor` on the same values: tails, FDR, mask and gather on the device, the selected matrix stays in HBM.
Host clock around calls that end synchronised, one warm-up round, then --runs rounds with the two legs alternating; the document
holds the median and the range of each leg, the split of each leg into its steps (each step timed on its own, same rounds), and the
build id of the library.

    python profiles/select_tensor_timing.py [--runs 5] [--rows 20000] [--cols 7880] [--out profiles/select_tensor_timing.md]
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


def build_matrix(torch, n, m, classes, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(20000 + m)
    y = torch.randperm(n, generator=g, device=dev) % classes
    s = (y == 0).double() - (y == classes - 1).double()
    kind = torch.arange(m, device=dev) % 24   # 0-7 shifted, 8-11 rounded, 12-17 binary, 18 single, 19 constant, 20-23 noise
    kf = kind.double()
    coef = torch.where(kind < 8, 0.15 * (kf + 1), torch.where(kind < 12, 0.3 * (kf - 7), torch.where(kind < 18, 0.4 * (kf - 11),
                                                                                               torch.zeros_like(kf))))
    X = torch.randn((n, m), generator=g, device=dev, dtype=torch.float64)
    X += s[:, None] * coef[None, :]
    rounded, binary = (kind >= 8) & (kind < 12), (kind >= 12) & (kind < 18)
    X[:, rounded] = torch.round(X[:, rounded])
    X[:, binary] = (X[:, binary] > 0).double()
    X[:, kind == 18] = 0.0
    X[int(torch.randint(n, (1,), generator=g, device=dev)), kind == 18] = 1.0
    X[:, kind == 19] = 2.5
    return X, y.cpu().numpy().astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--cols", type=int, default=7880)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_tensor_timing.md"))
    args = ap.parse_args()
    import ctypes

    import pandas as pd
    import torch

    from tsfresh_amd import _native, select_features_tensor
    from tsfresh_amd.feature_selection.relevance import _relevance_table
    if _native.device_count() < 1:
        raise SystemExit("select_tensor_timing.py needs a HIP device: nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda:0")
    n, m, C = args.rows, args.cols, args.classes
    X, y = build_matrix(torch, n, m, C, dev)
    names = ["f%d" % j for j in range(m)]
    y_series = pd.Series(y)
    dm = _native.DeviceMatrix(n, m, 0)
    host = X.cpu().numpy()
    lib = _native.load()
    _native._check(lib, lib.tsfa_device_copy(ctypes.c_void_p(dm.ptr), host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1, 0))
    del host
    codes = y.astype(np.int32)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def before():
        table = _relevance_table(dm, names, y_series, "auto", False, 1, False, "mann", 0.05, False, 0)
        relevant = list(table[table.relevant].feature)
        return relevant, dm.to_host([int(f[1:]) for f in relevant])

    def after():
        return select_features_tensor(X, y, check_nan=False)

    p = torch.empty((m, C), dtype=torch.float64, device=dev)
    routes = torch.empty((m, C), dtype=torch.uint8, device=dev)
    types = torch.empty(m, dtype=torch.uint8, device=dev)
    rel_t = torch.empty((m, C), dtype=torch.uint8, device=dev)
    rel = torch.empty(m, dtype=torch.uint8, device=dev)
    nsig = torch.empty(m, dtype=torch.int32, device=dev)
    pmin = torch.empty(m, dtype=torch.float64, device=dev)
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    state = {}

    def step_sweep():      # statistics sweep + its four copies to the host: the first step of the leg before
        return _native.relevance_classes(dm, codes, C, device=0)

    def step_tails():      # the same sweep + the tails kernels, nothing copied
        return _native.relevance_tails_classes(X.data_ptr(), n, m, m, codes, C, p.data_ptr(), routes.data_ptr(), types.data_ptr())

    def step_fdr():
        live = int((types != 0).sum().item())
        c_m = float(np.sum(1.0 / np.arange(1, live + 1)))
        _native.relevance_fdr(p.data_ptr(), types.data_ptr(), m, C, 0.05, c_m, 1, False, rel_t.data_ptr(), rel.data_ptr(),
                              nsig.data_ptr(), pmin.data_ptr())

    def step_gather():
        k = _native.compact_mask(rel.data_ptr(), m, idx.data_ptr())
        out = torch.empty((n, k), dtype=torch.float64, device=dev)
        _native.gather_columns_device(X.data_ptr(), n, m, idx.data_ptr(), k, out.data_ptr(), k)
        state["k"] = k
        return out

    def step_to_host():
        return dm.to_host(state["cols"])

    legs = [("before", before), ("after", after), ("sweep", step_sweep), ("tails", step_tails), ("fdr", step_fdr),
            ("gather", step_gather), ("to_host", step_to_host)]
    times = {name: [] for name, _ in legs}
    results = {}
    for rnd in range(args.runs + 1):   # round 0 warms every shape up
        for name, fn in legs:
            if name == "to_host" and "cols" not in state:
                state["cols"] = [int(f[1:]) for f in results["before"][0]]
            dt, out = clock(fn)
            results[name] = out
            if rnd:
                times[name].append(dt)
            print("round %d %s %.4f s" % (rnd, name, dt), flush=True)
    rel_before, block_before = results["before"]
    sel_after, cols_after, _ = results["after"]
    same = sorted(int(f[1:]) for f in rel_before) == cols_after
    order = np.argsort([int(f[1:]) for f in rel_before])
    same_cells = same and np.array_equal(block_before[:, order], sel_after.cpu().numpy())
    with open(_native.LIB_PATH, "rb") as f:
        build_id = hashlib.sha256(f.read()).hexdigest()[:16]

    def cell(name):
        t = times[name]
        return "%.4f (%.4f .. %.4f)" % (statistics.median(t), min(t), max(t))

    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["# Selection on tensors: timing", "",
             "Written by `profiles/select_tensor_timing.py` on %s, one process, one device; library build id "
             "(sha256(libtsfresh_amd.so)[:16]) `%s`." % (torch.cuda.get_device_name(0), build_id), "",
             "%d rows x %d columns float64 (%.2f GB), %d classes, \"mann\", Benjamini-Yekutieli at 0.05; %d columns selected.  Host clock "
             "around calls that end synchronised, one warm-up round, %d timed rounds with the legs alternating; seconds, median "
             "(min .. max)." % (n, m, n * m * 8 / 1e9, C, len(cols_after), args.runs), "",
             "| leg | seconds |", "|---|---|",
             "| before: `_relevance_table(DeviceMatrix)` + `to_host(selected)` | %s |" % cell("before"),
             "| after: `select_features_tensor` (selected matrix stays in HBM) | %s |" % cell("after"), "",
             "The steps, each timed on its own in the same rounds:", "",
             "| step | seconds |", "|---|---|",
             "| statistics sweep + copy of the statistics to the host (`tsfa_relevance_classes`) | %s |" % cell("sweep"),
             "| before: host tails, FDR and table (the leg minus sweep and `to_host`) | %.4f |" % (
                 med["before"] - med["sweep"] - med["to_host"]),
             "| before: `to_host` of the selected columns (`tsfa_gather_columns` + copy) | %s |" % cell("to_host"),
             "| after: statistics sweep + device tails (`tsfa_relevance_tails_classes`) | %s |" % cell("tails"),
             "| after: device tails alone (the row above minus the sweep row; the sweep row includes %.1f MB of copies) | %.4f |" % (
                 m * (32 + 16 * C) / 1e6, med["tails"] - med["sweep"]),
             "| after: FDR step-up and combination (`tsfa_relevance_fdr`, incl. the read of the column types) | %s |" % cell("fdr"),
             "| after: mask compaction + device gather (`tsfa_compact_mask`, `tsfa_gather_columns_device`) | %s |" % cell("gather"), "",
             "The two legs selected %s columns%s." % ("the same" if same else "DIFFERENT",
                                                     " with equal cells" if same_cells else (" but DIFFERENT cells" if same else "")), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
