#!/bin/bash
# kernel trace of the single-device headline step (1 timed + 1 stage-marked step of --full, no
# warmup, no verification) and its per-step breakdown (tools/step_breakdown.py); outputs under
# $OUT_DIR (default out/ in the repository)
set -o pipefail
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/out}
mkdir -p $O
rm -rf $O/prof_single
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace -d $O/prof_single -o single -- python3 $R/bench.py --steps 1 --warmup 0 --full --no-verify --no-cpu-baseline --no-e2e --no-paths > $O/ps.json 2> $O/ps.err || { echo fail; tail -5 $O/ps.err; exit 1; }
python3 $R/tools/step_breakdown.py $O/prof_single 2 | tee $O/ps_breakdown.txt
