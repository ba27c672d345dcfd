#!/bin/bash
# kernel traces of one step through the sharded path (st_dev_sog_sharded at world 1, RCCL) and
# the single-device path (st_dev_sog), each with its per-step breakdown (tools/step_breakdown.py):
# the per-rank overhead of the multi-GPU code; --full for the stage-marked step the breakdown's
# step count includes; outputs under $OUT_DIR (default out/ in the repository)
set -o pipefail
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT_DIR:-$R/out}
mkdir -p $O
rm -rf $O/prof_dist $O/prof_single
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace -d $O/prof_dist -o dist -- python3 $R/bench.py --dist --steps 1 --warmup 1 --full --no-verify --no-cpu-baseline > $O/pd.json 2> $O/pd.err && \
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace -d $O/prof_single -o single -- python3 $R/bench.py --steps 1 --warmup 1 --full --no-verify --no-cpu-baseline --no-e2e --no-paths > $O/ps.json 2> $O/ps.err && \
python3 $R/tools/step_breakdown.py $O/prof_dist 3 > $O/pd_breakdown.txt && \
python3 $R/tools/step_breakdown.py $O/prof_single 3 > $O/ps_breakdown.txt
echo rc=$?
