#!/bin/bash
# Round-2 artefacts in one GPU call: PMC traffic (ODE step + dominant bench kernel), rocprofv3 kernel stats of the bench
# and of the step bench, the default bench line.  Outputs under $SF_OUT_DIR; the summaries are copied into profiles/ by hand.
cd /tmp; export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${SF_OUT_DIR:?set SF_OUT_DIR to the directory that receives the outputs}
bash $R/tools/pmc_step.sh > $OUT/pmc_step.log 2>&1
bash $R/tools/final_profile.sh
for cfg in "1 50 50" "8 50 50" "1 200 200"; do
  tag=$(echo $cfg | tr ' ' '_')
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stepstats_$tag -- python3 $R/tools/stepbench.py $cfg 50 > $OUT/stepstats_$tag.log 2>$OUT/stepstats_$tag.err
done
cd $R
python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -c 600 $OUT/bench_default.json
