#!/usr/bin/env python
"""The tables of profiles/spectral_route_accuracy.md: per rfft route of k_spectral and level of tests/spectral_truth.py, the
worst error / bar of np.fft.rfft(x) (what tests/parity.py compares against), of the g++ build of the kernel sources and --
with --device -- of the HIP kernels, over both builds and the three modes (default options, "bluestein": 0,
"bluestein_min": 257) with which the route tests reach every route on every length that has two.

    python profiles/spectral_route_accuracy.py [--device]  > table.md

A cell is `bins / aggregated`: fft_coefficient (real, imag, abs of the sampled bins) and fft_aggregated.  The measured
constants of the sweep bars (the float64 restatements' worst error / law) are printed first."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import spectral_truth as st  # noqa: E402
from engines import emul_engine, hip_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="add the HIP kernels' column (needs a GPU)")
    ap.add_argument("--no-constants", action="store_true", help="skip the restatements (a minute of Python loops)")
    args = ap.parse_args()
    if not args.no_constants:
        print("worst error / law of the float64 restatements, {n: (bins >= 1, bin 0)}\n")
        for route, w in st.measure_restatements().items():
            print("* %s: over the grid %.4g and %.4g; per length {%s}" % (
                route, max(v[0] for v in w.values()), max(v[1] for v in w.values()),
                ", ".join("%d: (%.3g, %.3g)" % (n, w[n][0], w[n][1]) for n in sorted(w))))
        print()
    engines = ["np.fft.rfft(x)", "emulation"] + (["device"] if args.device else [])
    failing = {e: 0 for e in engines}
    for dtype_name in ("float64", "float32"):
        worst = {e: {} for e in engines}
        for build in ("lds", "long"):
            for mode in st.MODES:
                cases = st.batch(dtype_name, build)
                if mode != "default":
                    cases = [c for c in cases if len({st.route_of(c.n, m) for m in st.MODES}) > 1]
                st.reference_worst(cases, mode, worst["np.fft.rfft(x)"])
                for k in ("TSFA_EMUL_BLUESTEIN", "TSFA_EMUL_BLUESTEIN_MIN"):
                    os.environ.pop(k, None)
                os.environ.update(st.MODE_ENV[mode])
                names, got = emul_engine(st.params(cases), *st.pack(cases, np.float64))
                failing["emulation"] += len(st.check(names, got, cases, mode, worst=worst["emulation"]))
                if args.device:
                    names, got = hip_engine(st.params(cases), *st.pack(cases, np.dtype(dtype_name)), options=st.MODE_OPTIONS[mode])
                    failing["device"] += len(st.check(names, got, cases, mode, worst=worst["device"]))
        print("%s: worst error / bar, bins / aggregated\n" % dtype_name)
        print(st.worst_table([worst[e] for e in engines], engines))
        print()
    print("cells beyond their bar: " + ", ".join("%s %d" % (e, failing[e]) for e in engines[1:]))


if __name__ == "__main__":
    main()
