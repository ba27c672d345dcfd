#!/usr/bin/env python3
"""Importance, decimation and crops (st_abi.h) on bench.py's synthetic SH-3 table, 1M and 10M rows.

  kernels    the library's HIP events (set_profiling) around its launches, summed per name over one
             call: im.score (the four columns -> keys), im.hist / im.pick (radix select, eight
             rounds), im.flags (split, the tie scan, take), im.sort (radix_sort_u64 of the inverted
             keys), im.box, im.sphere; 2 warm-up calls, REPS (default 5) timed, medians.
  whole      host wall clock of dev_importance_top (count n / 4: decimate's selection -- score,
             select, flags, compaction and its read-back of the count), of dev_importance_order
             (orderByImportance's permutation) and of dev_importance (the scores alone).  The row
             gather that follows in a chain is permuteRows, measured by tools/bench_paths.py.
  crops      filterBox and filterSphere run inside a chain only: dev_compressed_ply over the device
             table with the one action in front, the kernel's events (im.box / im.sphere) beside
             the call's wall clock (which includes the gather and writeCompressedPly of the kept rows).
  yardsticks k_mm_partial ("mm.partial", st_dev_minmax) over the same four float columns: one plain
             read of what im.score reads.  And decimate's row list the other way: the first n / 4
             entries of dev_importance_order sorted ascending (torch.sort), its wall clock beside
             the select path's; the two lists are compared.

Writes out/importance.json (or argv[1])."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import torch

import splat_hip as sh
from bench import synth_table

WARM = 2
REPS = int(os.environ.get('REPS', '5'))
KERNELS = ('im.score', 'im.hist', 'im.pick', 'im.flags', 'im.sort', 'im.box', 'im.sphere')
SCORE_COLS = ('scale_0', 'scale_1', 'scale_2', 'opacity')


def med(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'reps': len(xs)}


def timed(ctx, fn):
    """fn() WARM + REPS times: (wall medians, per-kernel medians and launch counts, the last result)"""
    walls, per, launches, last = [], {k: [] for k in KERNELS}, {}, None
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if r >= WARM:
            walls.append(wall)
            for k in KERNELS:
                ms, cnt = ctx.kernel_stats(k)
                if cnt:
                    per[k].append(ms)
                    launches[k] = cnt
    kernels = {k: dict(med(v), launches=launches[k]) for k, v in per.items() if v}
    return {'wall': med(walls), 'kernels': kernels}, last


def bench_table(ctx, n):
    cols = synth_table(n, 1234, 'cuda')
    items = list(cols.items())
    four = [(k, cols[k]) for k in SCORE_COLS]
    four_bytes = 16 * n
    m = n // 4
    torch.cuda.synchronize()
    res = {'rows': n, 'kept': m, 'score_columns_bytes': four_bytes}
    res['scores'], _ = timed(ctx, lambda: ctx.dev_importance(four))
    res['decimate_select'], top = timed(ctx, lambda: ctx.dev_importance_top(four, m))
    res['order'], order = timed(ctx, lambda: ctx.dev_importance_order(four))
    # the yardstick for decimate: the sort, then the first m rows put back in row order
    def by_sort():
        o = ctx.dev_importance_order(four)
        return torch.sort(o[:m]).values  # row indices below 2^31: int32 order is uint32 order
    res['decimate_by_sort'], top2 = timed(ctx, by_sort)
    res['decimate_lists_equal'] = bool(torch.equal(top, top2))
    e = res['decimate_select']['kernels']['im.score']
    e['bytes_read'] = four_bytes
    e['GBps'] = four_bytes / (e['median_ms'] / 1e3) / 1e9
    e = res['decimate_select']['kernels']['im.hist']
    e['bytes_read'] = 8 * n * e['launches']
    e['GBps'] = e['bytes_read'] / (e['median_ms'] / 1e3) / 1e9
    # the yardstick for the score kernel: k_mm_partial over the same four columns
    ms = []
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        ctx.dev_minmax([cols[k] for k in SCORE_COLS])
        t, cnt = ctx.kernel_stats('mm.partial')
        assert cnt == 1
        if r >= WARM:
            ms.append(t)
    y = med(ms)
    y['bytes_read'] = four_bytes
    y['GBps'] = four_bytes / (y['median_ms'] / 1e3) / 1e9
    res['yardstick_mm_partial'] = y
    # the crops, inside a chain
    chunk = torch.empty((n + 255) // 256 * 18, dtype=torch.float32, device='cuda')
    vertex = torch.empty(n * 4, dtype=torch.int32, device='cuda')
    shb = torch.empty(n * 45, dtype=torch.uint8, device='cuda')
    for name, act in (('filterBox', {'kind': 'filterBox', 'min': (-5, -5, -5), 'max': (5, 5, 5)}),
                      ('filterSphere', {'kind': 'filterSphere', 'center': (0, 0, 0), 'radius': 7.0})):
        r, out = timed(ctx, lambda: ctx.dev_compressed_ply(items, [act], chunk, vertex, shb))
        k = 'im.box' if name == 'filterBox' else 'im.sphere'
        r['kernels'][k]['bytes_read'] = 12 * n
        r['kernels'][k]['GBps'] = 12 * n / (r['kernels'][k]['median_ms'] / 1e3) / 1e9
        r['rows_kept'] = out[0]
        res[name] = r
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'importance.json')
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
