#!/bin/bash
# headline workload at other samples-per-forward (information only: the bench line stays at 32)
set -u
: "${GRAFT_REPO_ROOT:?run through gpurun}"
cd "$(dirname "$0")/../.."; out=${SF_OUT_DIR:?set SF_OUT_DIR to the directory that receives the outputs}/bsweep; mkdir -p $out
for b in 16 32 48 64; do
  timeout 600 python bench.py --steps 6 --warmup 2 --full --headline-only --batch $b > $out/b$b.json 2> $out/b$b.err
  python - <<PY
import json
d=json.loads(open("$out/b$b.json").read().strip().splitlines()[-1])
print("batch $b", round(d["value"],1), "ODE-steps/s", round(d["ms_per_step"],2), "ms", round(d["ms_per_step"]/$b,3), "ms/sample", round(d["roofline"]["frac"],3))
PY
done
