"""Writes tests/golden/pvalue_adf_truth.json: the many-digit ADF test statistic and lag of every case of
tests/pvalue_cases.py: adf_cases (tests/adf_mp.py, 120 digits; about a minute).  tests/test_pvalue_floor.py recomputes every
entry and compares, so the file cannot go stale unnoticed.

    python tests/golden/gen_pvalue_adf_truth.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pvalue_cases as pc  # noqa: E402

if __name__ == "__main__":
    with open(pc.ADF_TRUTH_FILE, "w") as f:
        json.dump(pc.compute_adf_truth(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", pc.ADF_TRUTH_FILE)
