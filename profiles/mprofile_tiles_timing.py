#!/usr/bin/env python
"""matrix_profile: the tiled route (plan option mp_tiles = 1) against another build of the library, shape by shape.

    python profiles/mprofile_tiles_timing.py --parent-lib /path/to/the/parent/libtsfresh_amd.so [--trace] [--out-dir DIR]

Six columns of one window (w = 36), float32 input.  Per shape and library one child process (a library is loaded once per
process; the other build is given to the child through TSFA_LIB), the two alternating: the family's event timing
(tsfa_plan_set_profiling), four extracts, best of the last three.  The results of the two builds are compared bit for bit.
--trace: one more child per shape under `rocprofv3 --kernel-trace --stats` for the split between k_mpt_prologue, k_mpt_sweep
and k_mpt_epilogue (mean per launch).  Prints markdown table rows; every child runs under a time limit and the first failure
ends the script."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 36
ISSUE_BOUND = 5.8e11   # cell updates per second: profiles/mprofile_timing.md
SHAPES = ((1, 100000), (8, 32768), (1000, 4096), (1000, 3600), (10000, 1024))


def cells(n):
    nd = n - W + 1 - (W + 3) // 4 - 1
    return nd * (nd + 1) // 2


def child(args):
    import numpy as np
    sys.path.insert(0, ROOT)
    from tsfresh_amd import _native
    B, n = args.child
    values = np.random.default_rng(B * 1000003 + n).standard_normal(B * n).astype(np.float32)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    cid = _native.calc_id("matrix_profile")
    plan = _native.Plan([(cid, (float(W), float(k), 0.0, 0.0)) for k in range(6)])
    if args.tiles is not None:
        plan.set_option("mp_tiles", args.tiles)
    plan.set_profiling(True)
    ms = []
    for _ in range(args.runs):
        out = np.array(plan.extract_host(values, offsets))
        ms.append(dict(plan.last_timings())["k_mprofile"])
    rec = [r for r in plan.last_launches() if r["family"] == "MPROFILE"]
    plan.close()
    np.save(args.save, out)
    print("RESULT " + json.dumps({"ms": ms, "variant": sorted({r["variant"] for r in rec}), "long_build": sorted({r["long_build"] for r in rec})}))


def run_child(B, n, lib, tiles, save, runs=4, wrap=()):
    env = dict(os.environ)
    env.pop("TSFA_LIB", None)
    if lib:
        env["TSFA_LIB"] = lib
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", str(B), str(n), "--save", save, "--runs", str(runs)]
    if tiles is not None:
        cmd += ["--tiles", str(tiles)]
    res = subprocess.run(["timeout", "-k", "10", "400"] + cmd, env=env, capture_output=True, text=True)
    line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    if res.returncode != 0 or not line:
        sys.exit("child failed (%d): %s\n%s" % (res.returncode, " ".join(cmd), (res.stdout + res.stderr)[-3000:]))
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out-dir", help="where the result matrices and traces go (default: a new temporary directory)")
    ap.add_argument("--child", nargs=2, type=int)
    ap.add_argument("--tiles", type=float)
    ap.add_argument("--save")
    ap.add_argument("--runs", type=int, default=4)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import numpy as np
    if args.out_dir is None:
        import tempfile
        args.out_dir = tempfile.mkdtemp(prefix="mprofile_tiles_")
    os.makedirs(args.out_dir, exist_ok=True)
    print("| shape | cells | parent: route, ms (runs 2-4) | tiles: ms (runs 2-4) | tiles: cells / s | of the issue bound | parent / tiles | same bits |")
    print("|---|---|---|---|---|---|---|---|")
    for B, n in SHAPES:
        a_npy, b_npy = (os.path.join(args.out_dir, "mpt_%s_%dx%d.npy" % (k, B, n)) for k in ("parent", "tiles"))
        new = run_child(B, n, None, 1, b_npy)
        assert new["variant"] == [1], new
        old = run_child(B, n, args.parent_lib, None, a_npy) if args.parent_lib else None
        t_new = min(new["ms"][1:])
        same = "-"
        old_txt = "-"
        ratio = "-"
        if old:
            same = "yes" if np.array_equal(np.load(a_npy), np.load(b_npy), equal_nan=True) else "NO"
            t_old = min(old["ms"][1:])
            old_txt = "%s, %.2f (%s)" % ("HBM scratch" if old["long_build"] == [1] else "LDS", t_old, ", ".join("%.2f" % v for v in old["ms"][1:]))
            ratio = "%.2f" % (t_old / t_new)
        rate = B * cells(n) / (t_new * 1e-3)
        print("| %d x %d | %.3g | %s | %.2f (%s) | %.3g | %.0f %% | %s | %s |" % (
            B, n, B * cells(n), old_txt, t_new, ", ".join("%.2f" % v for v in new["ms"][1:]), rate, 100.0 * rate / ISSUE_BOUND, ratio, same), flush=True)
    if args.trace:
        print("\n| shape | k_mpt_prologue ms | k_mpt_sweep ms | k_mpt_epilogue ms |\n|---|---|---|---|")
        for B, n in SHAPES:
            d = os.path.join(args.out_dir, "mpt_trace_%dx%d" % (B, n))
            run_child(B, n, None, 1, os.path.join(args.out_dir, "mpt_trace.npy"), runs=3,
                      wrap=("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--"))
            mean = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    for k in ("k_mpt_prologue", "k_mpt_sweep", "k_mpt_epilogue"):
                        if k in row["Name"]:
                            mean[k] = float(row["AverageNs"]) * 1e-6
            print("| %d x %d | %s |" % (B, n, " | ".join("%.3f" % mean[k] if k in mean else "not measured" for k in
                                                          ("k_mpt_prologue", "k_mpt_sweep", "k_mpt_epilogue"))), flush=True)


if __name__ == "__main__":
    main()
