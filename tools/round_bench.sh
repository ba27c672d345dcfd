#!/bin/bash
# the round's evidence: full bench line (--full, with the CPU baseline) + rocprofv3 kernel summary
# of the same command; outputs under $OUT_DIR/<tag>_* (default out/; set OUT_DIR to the folder the
# other evidence steps write to when mk_profiles.py is to pick these files up beside theirs)
set -o pipefail
tag=${1:-r01}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 900 python3 bench.py --full > $O/${tag}_bench.json 2> $O/${tag}_bench.err || { tail -20 $O/${tag}_bench.err; exit 1; }
cat $O/${tag}_bench.json
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $O/${tag}_prof -o bench --output-format csv -- python3 bench.py --full --no-cpu-baseline > $O/${tag}_prof.json 2> $O/${tag}_prof.err || { tail -20 $O/${tag}_prof.err; exit 1; }
echo profiled
