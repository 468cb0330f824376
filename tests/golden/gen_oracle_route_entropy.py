"""tests/golden/oracle_route_entropy.json: sample_entropy of the iid series of tests/route_cases.py at 17 408 and 17 409 samples
(TSFA_ENTH_MAXN and one beyond: the last length of the bit-matrix sweep over HBM and the first of the pair sweep), evaluated by
oracle/ (the reference's own loop, one O(n) numpy pass per template: about 40 s per series, so
tests/test_route_edges_gpu.py compares against the stored values).  The reference's approximate_entropy cannot be evaluated at
these lengths (an n x n x m float64 array: 4.8 GB).
    python tests/golden/gen_oracle_route_entropy.py"""
import json
import multiprocessing as mp
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

LENS = (17408, 17409)
KIND, SEED = "iid", 0


def _one(n):
    import numpy as np
    from engines import oracle_engine
    from route_cases import series_at
    x = series_at(n, KIND, SEED).astype(np.float64)
    names, want = oracle_engine({"sample_entropy": None}, x, np.array([0, len(x)], dtype=np.int64))
    return n, float(want[0, 0])


def main():
    with mp.get_context("spawn").Pool(len(LENS)) as pool:
        res = pool.map(_one, LENS)
    doc = {"kind": KIND, "seed": SEED, "sample_entropy": {str(n): repr(v) for n, v in res}}
    json.dump(doc, open(os.path.join(HERE, "oracle_route_entropy.json"), "w"), indent=1)
    print(doc)


if __name__ == "__main__":
    main()
