#!/usr/bin/env python
"""Wall clock of `extract_rolled_features` end to end on a time-ordered frame (the usual sensor log of a forecasting job):
n ids x n stamps, rows ordered by (time, id), int64 id and time, float32 values, max_timeshift=64, MinimalFCParameters.

    python profiles/roll_device_timing.py --pack host|device [--rows-log2 18 20 22] [--runs 5] [--package-root DIR]

--pack host runs on any commit (a package that predates the keyword is called without it: its only route is the host's);
--package-root: import tsfresh_amd from another checkout (the parent commit's "before" leg of profiles/roll_device_timing.md).
One JSON line per size: the median and the spread of --runs warm runs, and the phases of the LAST run -- pack (pack_timeseries),
windows (roll_views on the host route; tsfa_roll_windows + the host copies of series / timeshifts / shift values on the device
route), extract (the native call, on the host route with its uploads), assemble (everything else: the id tuples, the
ordering step, the DataFrame).
"""
import argparse
import hashlib
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(owner, name, bucket, phases):
    fn = getattr(owner, name)

    def wrapper(*a, **k):
        t0 = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            phases[bucket] = phases.get(bucket, 0.0) + time.perf_counter() - t0
    setattr(owner, name, wrapper)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pack", choices=("host", "device"), required=True)
    ap.add_argument("--rows-log2", type=int, nargs="+", default=[18, 20, 22])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    from tsfresh_amd import MinimalFCParameters, _native, extract_rolled_features
    from tsfresh_amd.feature_extraction import extraction
    from tsfresh_amd.utilities import dataframe_functions

    has_keyword = "pack" in inspect.signature(extract_rolled_features).parameters
    if args.pack == "device" and not has_keyword:
        raise SystemExit("this package has no device route for extract_rolled_features")
    kw = dict(pack=args.pack) if has_keyword else {}
    phases = {}
    _timed(extraction, "pack_timeseries", "pack", phases)
    _timed(dataframe_functions, "roll_views", "windows", phases)
    _timed(_native.Plan, "extract_windows_host", "extract", phases)
    if hasattr(_native, "DeviceWindows"):
        for name in ("__init__", "_copy", "shift_values"):
            _timed(_native.DeviceWindows, name, "windows", phases)
        _timed(_native.Plan, "extract_windows_pack", "extract", phases)
    with open(_native.LIB_PATH, "rb") as f:
        build = hashlib.sha256(f.read()).hexdigest()[:12]
    params = MinimalFCParameters()
    for lg in args.rows_log2:
        n = 1 << (lg // 2)
        m = (1 << lg) // n
        rng = np.random.default_rng(lg)
        df = pd.DataFrame({"id": np.tile(np.arange(n, dtype=np.int64), m), "time": np.repeat(np.arange(m, dtype=np.int64), n),
                           "value": rng.standard_normal(n * m, dtype=np.float32)})
        times = []
        for run in range(args.runs + 1):   # (the first run is the warm-up)
            phases.clear()
            t0 = time.perf_counter()
            out = extract_rolled_features(df, column_id="id", column_sort="time", max_timeshift=64,
                                          default_fc_parameters=params, **kw)
            times.append(time.perf_counter() - t0)
        rest = times[-1] - sum(phases.values())
        print(json.dumps({"package": os.path.abspath(args.package_root), "library_sha256": build, "pack": args.pack,
                          "rows": n * m, "ids": n, "stamps": m, "windows": len(out), "runs": args.runs,
                          "median_s": round(statistics.median(times[1:]), 4), "min_s": round(min(times[1:]), 4),
                          "max_s": round(max(times[1:]), 4),
                          "last_run_phases_s": dict({k: round(v, 4) for k, v in sorted(phases.items())}, assemble=round(rest, 4))}),
              flush=True)
        del df, out


if __name__ == "__main__":
    main()
