#!/usr/bin/env python
"""DataFrame in -> DataFrame out of extract_features on frames whose rows are in TIME order (one row per (timestamp, id),
ids interleaved), packed on the host (pack="host": what the package did before the device packer) and on the device
(pack="device"), beside the id-ordered frame of the same size (the presorted fast path: the floor).

ComprehensiveFCParameters, float32 values, int64 id and time, 1024 stamps per id.  One process, warm (one untimed run per
configuration), then median and min - max of --runs timed runs.  Prints one JSON line per size and, with --md, the table
of profiles/pack_device_timing.md.
    python profiles/pack_device_timing.py [--rows 262144 1048576 4194304 16777216] [--runs 5] [--md out.md]
    python profiles/pack_device_timing.py --only-pack 16777216     (one DevicePack and nothing else: for rocprofv3)
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENGTH = 1024


def time_ordered_columns(rows, seed=42):
    n_ids = rows // LENGTH
    rng = np.random.default_rng(seed)
    ids = np.tile(np.arange(n_ids, dtype=np.int64), LENGTH)
    t = np.repeat(np.arange(LENGTH, dtype=np.int64), n_ids)
    v = rng.standard_normal(n_ids * LENGTH, dtype=np.float32)
    return ids, t, v


def timed(fn, runs):
    fn()   # warm
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 18, 1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--md", default=None)
    ap.add_argument("--only-pack", type=int, default=0)
    args = ap.parse_args()
    from tsfresh_amd import ComprehensiveFCParameters, _native, extract_features
    if args.only_pack:
        ids, t, v = time_ordered_columns(args.only_pack)
        cols = [_native.pack_column(a) for a in (ids, t, v)]
        for _ in range(2):
            pack = _native.DevicePack(cols[0], cols[1], cols[2])
            print(json.dumps({"rows": pack.n_rows, "n_series": pack.n_series, "passes": pack.n_passes}))
            pack.close()
        return
    params = ComprehensiveFCParameters()
    lines = []
    for rows in args.rows:
        ids, t, v = time_ordered_columns(rows)
        frame_t = pd.DataFrame({"id": ids, "time": t, "value": v})
        order = np.lexsort((t, ids))
        frame_id = pd.DataFrame({"id": ids[order], "time": t[order], "value": v[order]})
        kw = dict(column_id="id", column_sort="time", default_fc_parameters=params)
        res = {"rows": rows, "n_series": rows // LENGTH}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name, frame, mode in (("host", frame_t, "host"), ("device", frame_t, "device"), ("id_ordered", frame_id, "host")):
                ts = timed(lambda: extract_features(frame, pack=mode, **kw), args.runs)
                res[name] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}
        print(json.dumps(res), flush=True)
        lines.append(res)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| rows | series | pack=host median (min - max) s | pack=device median (min - max) s | "
                    "id-ordered frame median (min - max) s | host / device |\n|---|---|---|---|---|---|\n")
            for r in lines:
                cell = lambda d: "%.4f (%.4f - %.4f)" % (d["median_s"], d["min_s"], d["max_s"])  # noqa: E731
                f.write("| %d | %d | %s | %s | %s | %.1f |\n" % (r["rows"], r["n_series"], cell(r["host"]), cell(r["device"]),
                                                                 cell(r["id_ordered"]), r["host"]["median_s"] / r["device"]["median_s"]))


if __name__ == "__main__":
    main()
