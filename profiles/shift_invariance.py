#!/usr/bin/env python
"""The tables of profiles/shift_invariance.md: per invariant column group and level of tests/shift_cases.py, the worst
error / shift_bound of the reference's arithmetic (the oracle on the shifted series), of the g++ build of the kernel sources
and -- with --device -- of the HIP kernels; the share of cells the parity predicates skip; and the relative error of
change_quantiles(f_agg="var") on the jittered sawtooth against exact rational arithmetic.

    python profiles/shift_invariance.py [--device] [--cpu-cache FILE.npz]  > table.md

Tier-B groups are measured at every level here (the tests compare them at the two lower levels of a dtype only: the rows
above those levels show why).  --cpu-cache keeps the oracle's matrices between runs (minutes of O(n^2) entropies)."""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.simplefilter("ignore")
import shift_cases as sc  # noqa: E402
from engines import emul_engine, hip_engine, oracle_engine_parallel  # noqa: E402

DTYPES = ("float64", "float32")


def _fmt(v):
    return "-" if v is None else ("%.2g" % v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="add the HIP kernels' column (needs a GPU)")
    ap.add_argument("--cpu-cache", default="", help="npz file that keeps the oracle's matrices between runs")
    args = ap.parse_args()

    cases = {d: sc.cases(d) for d in DTYPES}
    every = [c for d in DTYPES for c in cases[d]]
    # the cache belongs to the inputs it was computed from: the digest of every base, shifted series and column parameter
    import hashlib
    digest = hashlib.sha1(b"".join(c.b.tobytes() + c.x.astype(np.float64).tobytes() for c in every)
                          + repr(sorted((k, repr(v)) for k, v in sc.params().items())).encode()).hexdigest()
    cache = dict(np.load(args.cpu_cache, allow_pickle=False)) if args.cpu_cache and os.path.exists(args.cpu_cache) else {}
    if "truth" in cache and str(cache.get("digest")) != digest:
        print("%s was computed from other inputs: recomputing" % args.cpu_cache, file=sys.stderr)
        cache = {}
    if "truth" in cache:
        names = [str(n) for n in cache["names"]]
        truth_all, ref_all = cache["truth"], cache["ref"]
    else:
        names, truth_all = sc.truth_of(every)
        rnames, ref_all = oracle_engine_parallel(sc.params(), *sc.pack([c.x for c in every]))
        assert rnames == names
        if args.cpu_cache:
            np.savez(args.cpu_cache, names=np.array(names), truth=truth_all, ref=ref_all, digest=np.array(digest))
    assert truth_all.shape == (len(every), len(names))

    worst = {}      # (engine, dtype) -> {(group, level): violation}
    skipped_share = {}
    for d in DTYPES:
        rows = [i for i, c in enumerate(every) if c.dtype_name == d]
        truth, ref = truth_all[rows], ref_all[rows]
        values, offsets = sc.pack([c.x for c in cases[d]])
        engines = {"reference": ref, "emulation": emul_engine(sc.params(), values, offsets)[1]}
        if args.device:
            engines["device"] = hip_engine(sc.params(), values.astype(np.dtype(d)), offsets)[1]
        for name, got in engines.items():
            w, skipped = {}, []
            sc.compare_shift(names, got, truth, cases[d], worst=w, skipped=skipped, every_level=True)
            worst[name, d] = w
        tier_skipped = []
        sc.compare_shift(names, ref, truth, cases[d], skipped=tier_skipped)
        skipped_share[d] = (len(tier_skipped), sc.n_invariant_cells(names, cases[d]),
                            sorted({sc.group_of(col) for _, col in tier_skipped}))

    tier = {}
    for col in names:
        if sc.tier_of(col):
            tier[sc.group_of(col)] = sc.tier_of(col)
    cols = ["reference", "emulation"] + (["device"] if args.device else [])
    print("worst error / shift_bound per column group and level: %s%s\n" % (" / ".join(cols), "" if args.device else
                                                                           "  (no device column: run with --device)"))
    for d in DTYPES:
        levels = sc.TIER_A_LEVELS[d]
        print("%s\n\n| tier | columns | %s |\n|---|---|%s" % (d, " | ".join("%+g" % lv for lv in levels), "---|" * len(levels)))
        for g in sorted(tier, key=lambda g: (tier[g], g)):
            cells = [" / ".join(_fmt(worst[e, d].get((g, lv))) for e in cols) for lv in levels]
            print("| %s | %s | %s |" % (tier[g], g, " | ".join(cells)))
        n_skip, n_cells, groups = skipped_share[d]
        print("\nskipped by the parity predicates: %d of %d invariant cells (%.3f %%)%s\n"
              % (n_skip, n_cells, 100.0 * n_skip / n_cells, (": " + ", ".join(groups)) if groups else ""))

    # ---- the sawtooth
    saw = sc.sawtooth_cases()
    labels = [label for label, _ in saw]
    values, offsets = sc.pack([x for _, x in saw])
    snames, sref = oracle_engine_parallel(sc.SAW_PARAMS, values, offsets)
    struth = np.array([sc.sawtooth_truth(x, snames) for _, x in saw])
    engines = {"reference": sref, "emulation": emul_engine(sc.SAW_PARAMS, values, offsets)[1]}
    if args.device:
        short = [i for i, (_, x) in enumerate(saw) if len(x) < sc.SAW_LONG]     # as the GPU test: the LDS and the HBM build apart
        dev = np.empty_like(sref)
        for part in (short, [i for i in range(len(saw)) if i not in short]):
            dev[part] = hip_engine(sc.SAW_PARAMS, *sc.pack([saw[i][1] for i in part]))[1]
        engines["device"] = dev
    sworst = {}
    for name, got in engines.items():
        sworst[name] = {}
        sc.compare_sawtooth(snames, got, struth, labels, worst=sworst[name])
    print("change_quantiles of the jittered sawtooth: worst relative error of the six var columns (and of the six mean columns)"
          "\n\n| series | smallest var | %s |\n|---|---|%s" % (" | ".join(cols), "---|" * len(cols)))
    var = [k for k, n in enumerate(snames) if 'f_agg_"var"' in n]
    for i, label in enumerate(labels):
        print("| %s | %.2g | %s |" % (label, struth[i, var].min(), " | ".join(
            "%s (%s)" % (_fmt(sworst[e][label, "var"]), _fmt(sworst[e][label, "mean"])) for e in cols)))


if __name__ == "__main__":
    main()
