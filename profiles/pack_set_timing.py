#!/usr/bin/env python
"""Wall clock of packing a frame of several kinds on the device: the per-kind route (what `pack_timeseries` did before the
pack set: host selection of every kind's rows, then one DevicePack per kind or value column) against the pack set (one sort
of the whole frame, `_native.DevicePackSet`), and a one-kind frame as the control.

2^22 rows by default, 1024 stamps per id, int64 id and time, float32 values:
  long      4 kinds, rows in (id, time) order with the kinds interleaved
  wide      4 value columns, rows in time order
  control   1 value column, rows in time order (one DevicePack on either route)
Best of --runs after one warm-up run, one JSON line per shape.  With TSFA_LIB pointing at a library that predates the set
only the per-kind legs and the control run (the "before" leg of profiles/pack_set_timing.md).
    python profiles/pack_set_timing.py [--rows 4194304] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LENGTH = 1024


def best(fn, runs):
    fn()   # warm
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        packed = fn()
        out.append(time.perf_counter() - t0)
        for pk in packed:
            if pk.device_pack is not None:
                pk.device_pack.close()
    return min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction import data
    has_set = hasattr(_native.load(), "tsfa_pack_set_create")
    rng = np.random.default_rng(42)
    rows, kinds_n = args.rows, 4

    # long: every (id, time) has its 4 kinds on consecutive rows
    n_ids = rows // (LENGTH * kinds_n)
    ids = np.repeat(np.arange(n_ids, dtype=np.int64), LENGTH * kinds_n)
    t = np.tile(np.repeat(np.arange(LENGTH, dtype=np.int64), kinds_n), n_ids)
    kinds = np.tile(np.array(["k0", "k1", "k2", "k3"], dtype=object), rows // kinds_n)
    long_ = pd.DataFrame({"id": ids, "time": t, "kind": kinds, "value": rng.standard_normal(rows, dtype=np.float32)})
    long_kw = dict(column_id="id", column_sort="time", column_kind="kind", column_value="value")
    # wide / control: one row per (time, id), ordered by time
    n_ids = rows // LENGTH
    wide = pd.DataFrame({"id": np.tile(np.arange(n_ids, dtype=np.int64), LENGTH),
                         "time": np.repeat(np.arange(LENGTH, dtype=np.int64), n_ids)})
    for c in "abcd":
        wide[c] = rng.standard_normal(rows, dtype=np.float32)
    wide_kw = dict(column_id="id", column_sort="time")

    def per_kind_long():   # pack_timeseries' long route before the set, with pack="device" for every kind
        kcodes, kuniq = pd.factorize(long_["kind"].to_numpy(), sort=True)
        ids_all, vals_all, sort_all = long_["id"].to_numpy(), long_["value"].to_numpy(), long_["time"].to_numpy()
        out = []
        for k, kind in enumerate(kuniq):
            sel = np.nonzero(kcodes == k)[0]
            out.append(data._pack(kind, ids_all[sel], vals_all[sel], sort_all[sel], pack="device"))
        return out

    def per_kind_wide():
        ids_all, sort_all = wide["id"].to_numpy(), wide["time"].to_numpy()
        return [data._pack(c, ids_all, wide[c].to_numpy(), sort_all, nan_name=c, pack="device") for c in "abcd"]

    legs = [("long", "per_kind", per_kind_long), ("wide", "per_kind", per_kind_wide),
            ("control", "one_pack", lambda: data.pack_timeseries(wide[["id", "time", "a"]], pack="device", **wide_kw)[0])]
    if has_set:
        legs += [("long", "set", lambda: data.pack_timeseries(long_, pack="device", **long_kw)[0]),
                 ("wide", "set", lambda: data.pack_timeseries(wide, pack="device", **wide_kw)[0])]
    for shape, route, fn in legs:
        packed = fn()
        passes = [pk.device_pack.n_passes if pk.device_pack is not None else None for pk in packed]
        for pk in packed:
            if pk.device_pack is not None:
                pk.device_pack.close()
        lo, hi = best(fn, args.runs)
        print(json.dumps({"lib": os.path.basename(_native.LIB_PATH), "shape": shape, "route": route, "rows": rows,
                          "best_s": round(lo, 5), "worst_s": round(hi, 5), "passes": passes}), flush=True)


if __name__ == "__main__":
    main()
