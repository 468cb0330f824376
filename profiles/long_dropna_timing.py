#!/usr/bin/env python
"""Wall clock of `extract_features_long_tensor(..., nan_policy="drop")` (profiles/long_dropna_timing.md).

--ids ids of --length float32 rows each, shuffled, C = 1 and C = 8 value columns (row-major), an int64 sort column,
MinimalFCParameters; 1 % and 30 % of the rows carry a NaN in one of their C values.  Three legs per measurement, in the same
process, alternating:
  drop      the entry with nan_policy="drop" on the gapped table (mark, scan, compact of the key columns, the set on the kept
            keys, the composed permutation)
  torch     the composition it replaces: a boolean mask over the value matrix, an indexed copy of ids, sort and the matrix,
            then the entry with nan_policy="raise"
  ungapped  the entry with nan_policy="raise" on the same table without gaps: what the call costs when nothing is dropped
            (and what it cost before the keyword existed)
The first two are compared bit for bit.  A host clock around synchronised calls, --rounds alternating rounds after one warm-up
round; medians and the spread (min .. max).  One JSON line per measurement.
    python profiles/long_dropna_timing.py [--ids 10000] [--length 1024] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from long_tensor_timing import alternate, summary   # noqa: E402  (the same clock and rounds as the entry's own timing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=10000)
    ap.add_argument("--length", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    from tsfresh_amd import MinimalFCParameters, extract_features_long_tensor
    if not torch.cuda.is_available():
        raise SystemExit("long_dropna_timing.py needs a GPU: a timing taken elsewhere says nothing")
    params = MinimalFCParameters()
    rng = np.random.default_rng(42)
    n = args.ids * args.length
    shuffle = rng.permutation(n)
    ids = torch.from_numpy(np.repeat(np.arange(args.ids, dtype=np.int64), args.length)[shuffle]).cuda()
    sort = torch.from_numpy(np.tile(np.arange(args.length, dtype=np.int64), args.ids)[shuffle]).cuda()
    for C in (1, 8):
        clean = torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32)).cuda()
        names = ["v%d" % c for c in range(C)]
        for share in (0.01, 0.30):
            rows = torch.from_numpy(rng.choice(n, size=int(n * share), replace=False)).cuda()
            x = clean.clone()
            x[rows, torch.from_numpy(rng.integers(0, C, size=len(rows))).cuda()] = float("nan")

            def drop():
                return extract_features_long_tensor(ids, x, sort=sort, kind_names=names, default_fc_parameters=params, nan_policy="drop")

            def composed():
                keep = ~torch.isnan(x).any(dim=1)
                return extract_features_long_tensor(ids[keep], x[keep], sort=sort[keep], kind_names=names, default_fc_parameters=params)

            def ungapped():
                return extract_features_long_tensor(ids, clean, sort=sort, kind_names=names, default_fc_parameters=params)

            times = alternate(torch, {"drop": drop, "torch": composed, "ungapped": ungapped}, args.rounds)
            got, want = drop(), composed()
            same = got[1] == want[1] and bool(torch.equal(got[2], want[2])) and \
                bool(torch.equal(got[0].view(torch.int64), want[0].view(torch.int64)))
            print(json.dumps({"what": "long_dropna", "rows": n, "C": C, "gapped_share": share, "bit_equal": same,
                              "drop": summary(times["drop"]), "torch": summary(times["torch"]),
                              "ungapped": summary(times["ungapped"])}), flush=True)
            del x
        del clean


if __name__ == "__main__":
    main()
