#!/bin/bash
# rocprofv3 kernel-trace summary of one bench step (+1 warmup) and of everything --full runs after
# it; output under $OUT_DIR/prof_<tag> (default out/)
set -o pipefail
tag=${1:-run}; shift || true
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof_${tag} -o bench --output-format csv -- python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 1 "$@" > $O/prof_${tag}.json 2> $O/prof_${tag}.err || { tail -20 $O/prof_${tag}.err; exit 1; }
f=$(find $O/prof_${tag} -name '*kernel_stats.csv' | head -1)
cut -d, -f1-8 "$f" | head -40
