#!/bin/bash
# A/B of library builds on the headline bench: bash profiles/ab.sh libA.so libB.so ...   (paths relative to tsfresh_amd/)
# the bench line of each build is kept as $AB_OUT/<lib>.json (default bench_outputs/ab)
export TMPDIR=/tmp
O=${AB_OUT:-bench_outputs/ab}
mkdir -p "$O"
for lib in "$@"; do
  TSFA_LIB=$PWD/tsfresh_amd/$lib timeout 600 python bench.py --full --no-cpu-baseline --no-e2e --steps 4 --warmup 1 2>/dev/null | tail -1 > "$O/$lib.json"
  python - <<PY
import json
d = json.load(open("$O/$lib.json"))
print("$lib", round(d["ms_per_step"], 3), {k: round(v, 3) for k, v in d["kernel_ms"].items()}, d.get("parity_sample"))
PY
done
