#!/usr/bin/env python3
"""The column summary (st_dev_summary) on bench.py's synthetic SH-3 table, 1M and 10M rows.

  kernels   the library's HIP events (set_profiling) around every launch of one dev_summary:
            sm.classify, sm.sum (the sum pass), sm.hist / sm.pick (radix select, four rounds for
            float32), sm.dev (the deviation pass), summed per name; 2 warm-up calls, REPS (default 5)
            timed, medians.  Beside each reading kernel: bytes read / time, where a pass over the
            table reads rows x 62 x 4 bytes (sm.hist reads it once per round).
  yardstick k_mm_partial ("mm.partial", st_dev_minmax) over the same 62 float columns in the same
            process: one plain read of the table, the in-tree rate to compare a pass with.
  whole     dev_summary's host wall clock (the launches, the two read-backs, the host's roundings),
            and the same with ST_SUM_EXACT=1 (every sum through the superaccumulator).
  paths     how many columns took the int128 fast path and the general path (summary_stats).
  numpy     min / max / mean / std / median of the same columns on the host, for scale only: numpy's
            float sums are not exact and its answers are not compared.

Writes out/summary.json (or argv[1])."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import numpy as np
import torch

import splat_hip as sh
from bench import synth_table

WARM = 2
REPS = int(os.environ.get('REPS', '5'))
KERNELS = ('sm.classify', 'sm.sum', 'sm.hist', 'sm.pick', 'sm.dev')


def med(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'reps': len(xs)}


def one_call(ctx, cols):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    ctx.dev_summary(cols)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, {k: ctx.kernel_stats(k) for k in KERNELS}


def bench_table(ctx, n):
    cols = synth_table(n, 1234, 'cuda')
    table_bytes = sum(t.numel() * t.element_size() for t in cols.values())
    torch.cuda.synchronize()
    res = {'rows': n, 'columns': len(cols), 'table_bytes': table_bytes}
    for label, exact in (('default', None), ('exact', '1')):
        os.environ.pop('ST_SUM_EXACT', None)
        if exact:
            os.environ['ST_SUM_EXACT'] = exact
        walls, per = [], {k: [] for k in KERNELS}
        launches = {}
        for r in range(WARM + REPS):
            wall, ks = one_call(ctx, cols)
            if r >= WARM:
                walls.append(wall)
                for k, (ms, cnt) in ks.items():
                    per[k].append(ms)
                    launches[k] = cnt
        out = {'dev_summary_wall': med(walls), 'paths': ctx.summary_stats(), 'kernels': {}}
        for k in KERNELS:
            e = med(per[k])
            e['launches'] = launches[k]
            if k != 'sm.pick':
                passes = launches[k]  # every launch of a reading kernel is one pass over a batch: one batch here
                e['bytes_read'] = table_bytes * passes
                e['GBps'] = e['bytes_read'] / (e['median_ms'] / 1e3) / 1e9
            out['kernels'][k] = e
        out['dev_summary_wall']['table_passes'] = sum(out['kernels'][k]['launches'] for k in KERNELS if k != 'sm.pick')
        res[label] = out
    os.environ.pop('ST_SUM_EXACT', None)
    # the yardstick: k_mm_partial over the same columns
    tensors = list(cols.values())
    ms = []
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        ctx.dev_minmax(tensors)
        t, cnt = ctx.kernel_stats('mm.partial')
        assert cnt == 1
        if r >= WARM:
            ms.append(t)
    y = med(ms)
    y['bytes_read'] = table_bytes
    y['GBps'] = table_bytes / (y['median_ms'] / 1e3) / 1e9
    res['yardstick_mm_partial'] = y
    # numpy on the host, for scale only
    host = {k: t.cpu().numpy() for k, t in list(cols.items())[:8]}
    t0 = time.perf_counter()
    for a in host.values():
        a.min(), a.max(), a.mean(dtype=np.float64), a.std(dtype=np.float64), np.median(a)
    res['numpy_host_ms_per_column'] = (time.perf_counter() - t0) * 1e3 / len(host)
    res['numpy_host_ms_table_extrapolated'] = res['numpy_host_ms_per_column'] * len(cols)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'summary.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    ctx.set_profiling(True)
    res = {'warmups': WARM, 'device': torch.cuda.get_device_name(0)}
    for n in (1_000_000, 10_000_000):
        res[f'n{n}'] = bench_table(ctx, n)
        print(n, json.dumps(res[f'n{n}']), flush=True)
        torch.cuda.empty_cache()
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main()
