#!/usr/bin/env python
"""sample_entropy / approximate_entropy: the tiled route (plan option ent_tiles = 1) against another build of the library,
shape by shape.

    python profiles/entropy_tiles_timing.py --parent-lib /path/to/the/parent/libtsfresh_amd.so [--trace] [--out-dir DIR]
                                            [--shapes 1x20000,8x32768] [--skip-parent 1x1000000]

The six tolerances of ComprehensiveFCParameters (sample_entropy, approximate_entropy m = 2, r = 0.1 .. 0.9), float32 input.
Per shape and library one child process (a library is loaded once per process; the other build is given to the child through
TSFA_LIB), the two alternating: the family's event timing (tsfa_plan_set_profiling) and the wall time of the whole call, four
extracts, best of the last three.  The results of the two builds are compared bit for bit.  --trace: one more child per
shape under `rocprofv3 --kernel-trace --stats` for the split between the route's kernels (mean per launch).  Prints markdown
table rows; every child runs under a time limit and the first failure ends the script."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 20000), (1, 100000), (1, 1000000), (8, 32768), (64, 20000), (256, 20000), (2000, 20000))
KERNELS = ("k_ent_prologue", "k_ent_windows", "k_ent_scan", "k_ent_sweep", "k_ent_epilogue")
PARAMS = {"sample_entropy": None, "approximate_entropy": [{"m": 2, "r": r} for r in (0.1, 0.3, 0.5, 0.7, 0.9)]}


def child(args):
    import numpy as np
    sys.path.insert(0, ROOT)
    from tsfresh_amd import _native
    from tsfresh_amd.feature_extraction.plan import compile_fc_parameters
    B, n = args.child
    values = np.random.default_rng(B * 1000003 + n).standard_normal(B * n).astype(np.float32)
    offsets = np.arange(B + 1, dtype=np.int64) * n
    plan = _native.Plan(compile_fc_parameters(PARAMS).native_specs(_native.calc_id))
    if args.tiles is not None:
        plan.set_option("ent_tiles", args.tiles)
    plan.set_profiling(True)
    ms, wall = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out = np.array(plan.extract_host(values, offsets))
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(dict(plan.last_timings())["k_entropy"])
    rec = [r for r in plan.last_launches() if r["family"] == "ENTROPY"]
    plan.close()
    np.save(args.save, out)
    print("RESULT " + json.dumps({"ms": ms, "wall": wall, "variant": sorted({r["variant"] for r in rec})}))


def run_child(B, n, lib, tiles, save, runs=4, wrap=(), limit=400):
    env = dict(os.environ)
    env.pop("TSFA_LIB", None)
    if lib:
        env["TSFA_LIB"] = lib
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", str(B), str(n), "--save", save, "--runs", str(runs)]
    if tiles is not None:
        cmd += ["--tiles", str(tiles)]
    res = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env, capture_output=True, text=True)
    line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    if res.returncode != 0 or not line:
        sys.exit("child failed (%d): %s\n%s" % (res.returncode, " ".join(cmd), (res.stdout + res.stderr)[-3000:]))
    return json.loads(line[-1][7:])


def shape_list(text):
    return tuple(tuple(int(v) for v in s.split("x")) for s in text.split(",") if s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out-dir", help="where the result matrices and traces go (default: a new temporary directory)")
    ap.add_argument("--shapes", type=shape_list, default=SHAPES)
    ap.add_argument("--skip-parent", type=shape_list, default=(), help="shapes at which the other build is not run")
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
        args.out_dir = tempfile.mkdtemp(prefix="entropy_tiles_")
    os.makedirs(args.out_dir, exist_ok=True)
    best = lambda r, key: "%.2f (%s)" % (min(r[key][1:]), ", ".join("%.2f" % v for v in r[key][1:]))
    print("| shape | parent: variant | parent: k_entropy ms (runs 2-4) | parent: call ms | tiles: k_entropy ms (runs 2-4) | tiles: call ms | parent / tiles | same bits |")
    print("|---|---|---|---|---|---|---|---|")
    for B, n in args.shapes:
        a_npy, b_npy = (os.path.join(args.out_dir, "ent_%s_%dx%d.npy" % (k, B, n)) for k in ("parent", "tiles"))
        new = run_child(B, n, None, 1, b_npy, runs=args.runs)
        assert new["variant"] == [5], new
        old = run_child(B, n, args.parent_lib, None, a_npy, runs=args.runs) if args.parent_lib and (B, n) not in args.skip_parent else None
        cells = ["-"] * 3 + [best(new, "ms"), best(new, "wall"), "-", "-"]
        if old:
            same = np.array_equal(np.load(a_npy), np.load(b_npy), equal_nan=True)
            cells = [str(old["variant"]), best(old, "ms"), best(old, "wall")] + cells[3:5] + [
                "%.2f" % (min(old["ms"][1:]) / min(new["ms"][1:])), "yes" if same else "NO"]
        print("| %d x %d | %s |" % (B, n, " | ".join(cells)), flush=True)
    if args.trace:
        print("\n| shape | %s |\n|---|%s" % (" | ".join("`%s` ms" % k for k in KERNELS), "---|" * len(KERNELS)))
        for B, n in args.shapes:
            d = os.path.join(args.out_dir, "ent_trace_%dx%d" % (B, n))
            run_child(B, n, None, 1, os.path.join(args.out_dir, "ent_trace.npy"), runs=3,
                      wrap=("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--"))
            mean = {}
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    for k in KERNELS:
                        if k in row["Name"]:
                            mean[k] = float(row["AverageNs"]) * 1e-6
            print("| %d x %d | %s |" % (B, n, " | ".join("%.3f" % mean[k] if k in mean else "not measured" for k in KERNELS)), flush=True)


if __name__ == "__main__":
    main()
