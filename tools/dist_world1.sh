O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 500 python -u -m pytest tests/test_dist_gpu.py -v --timeout 400 --timeout-method thread > $O/distg.log 2>&1 && \
timeout -k 10 300 python bench.py --dist --backend nccl --steps 3 --warmup 1 --full --no-cpu-baseline > $O/bdist.json 2> $O/bdist.err && \
timeout -k 10 300 python bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-e2e --no-paths > $O/bplain.json 2> $O/bplain.err
echo rc=$?; tail -5 $O/distg.log; tail -3 $O/bdist.err
