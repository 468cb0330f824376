#!/usr/bin/env python
"""ks_tail="host" against ks_tail="device_matrix" where one class is rare: select_features_tensor on 20 000 rows under "smir" with
a class of 5, 60 and 140 rows, and tsfa_ks_matrix_tails alone on batches that all take one kernel.
    python profiles/select_ks_matrix_timing.py [rounds, default 5]
Alternating rounds, medians, device work closed by a synchronize; one JSON line per figure (profiles/select_ks_matrix_timing.md)."""
import json
import statistics
import sys
import time
import warnings

import numpy as np
import torch

from tsfresh_amd import _native
from tsfresh_amd.tensor_selection import select_features_tensor

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_ROWS, HOST_COLS, ALL_COLS = 20000, 800, 7880
warnings.simplefilter("ignore", RuntimeWarning)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def select(X, y, tail):
    return lambda: select_features_tensor(X, y, ks_tail=tail, test_for_binary_target_real_feature="smir")


rng = np.random.default_rng(11)
for rare in (5, 60, 140):
    y = np.zeros(N_ROWS, dtype=np.int64)
    y[rng.choice(N_ROWS, rare, replace=False)] = 1
    X = torch.from_numpy(rng.standard_normal((N_ROWS, ALL_COLS))).cuda()
    legs = {"host_800": select(X[:, :HOST_COLS].contiguous(), y, "host"),
            "device_matrix_800": select(X[:, :HOST_COLS].contiguous(), y, "device_matrix"),
            "device_matrix_7880": select(X, y, "device_matrix")}
    times = {k: [] for k in legs}
    legs["device_matrix_800"]()   # warm-up: module load, allocator
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    print(json.dumps({"rare_rows": rare, "rounds": ROUNDS, **{k + "_ms": round(statistics.median(v), 3) for k, v in times.items()}}))

# the stage alone: 7 880 cells of one kernel each
n = 7880
batches = {"durbin_small_n140": ((10001, 142), np.sqrt(rng.uniform(0.1, 0.75, n) / 140.0)),
           "pomeranz_n140": ((10001, 142), np.sqrt(rng.uniform(0.76, 4.0, n) / 140.0)),
           "durbin_large_m117": ((200000, 200000), np.full(n, (1.4 / 1e5) ** (2.0 / 3.0) * (1.0 - 1e-9)))}
for name, ((a, b), d) in batches.items():
    n1 = torch.full((n,), a, dtype=torch.int64, device="cuda")
    n2 = torch.full((n,), b, dtype=torch.int64, device="cuda")
    dd = torch.from_numpy(d).cuda()
    p = torch.empty(n, dtype=torch.float64, device="cuda")
    route = torch.empty(n, dtype=torch.uint8, device="cuda")
    run = lambda: _native.ks_matrix_tails(n1.data_ptr(), n2.data_ptr(), dd.data_ptr(), n, p.data_ptr(), route.data_ptr(),
                                          device=torch.cuda.current_device())
    run()
    ms = [timed(run) for _ in range(ROUNDS)]
    assert bool((route == _native.TSFA_ROUTE_KS_MATRIX).all())
    print(json.dumps({"batch": name, "cells": n, "median_ms": round(statistics.median(ms), 3), "us_per_cell": round(statistics.median(ms) * 1e3 / n, 3)}))
