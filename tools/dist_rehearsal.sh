#!/bin/bash
# 2-rank rehearsal of bench.py's multi-GPU path on a 1-GPU box (gloo, both ranks on cuda:0), the
# step's output verified (--full); outputs under $OUT_DIR (default out/)
set -o pipefail
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
    --master-port 29533 bench.py --gpus 2 --backend gloo --splats ${1:-2000000} --steps 1 --warmup 1 \
    --full --no-cpu-baseline > $O/rehearsal.json 2> $O/rehearsal.err || { tail -30 $O/rehearsal.err; exit 1; }
cat $O/rehearsal.json
