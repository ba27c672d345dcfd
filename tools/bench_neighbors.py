#!/usr/bin/env python3
"""Neighbour distances and filterOutliers (st_abi.h) at 1M and 10M rows, k = 8 and k = 32, on two scenes:
`gaussian` (x, y, z ~ N(0, 1)) and `floaters` (99 % of the rows in 64 clusters of sigma 0.05 with
centres in [-5, 5]^3, 1 % uniform in [-30, 30]^3, shuffled), float32.

  kernels    the library's HIP events (set_profiling) around its launches, summed per name over one
             st_dev_neighbor_dist: nb.fill, nb.extent, nb.keys, nb.sort (the Morton sort alone),
             nb.gather, nb.boxes -- together the build -- and nb.search; 1 warm-up call, REPS (default
             3) timed, medians.  `pairs` (d2 evaluations) and `nodes` (box tests) of
             st_ctx_last_neighbor_stats per query row beside them.
  whole      host wall clock of st_dev_neighbor_dist, and of filterOutliers inside a chain:
             dev_compressed_ply over a 14-column device table with the one action (k, sigma 1) in
             front, beside the same call without it -- the difference is the action with its
             summary, compaction and row gather.
  yardstick  k_mm_partial ("mm.partial", st_dev_minmax) over x, y, z: one plain read of the positions.

Sizes from argv[2:] (default 1000000 10000000).  Writes out/neighbors.json (or argv[1]); a file that
exists is extended, so the sizes can be measured one call at a time."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import numpy as np
import torch

import splat_hip as sh

WARM = 1
REPS = int(os.environ.get('REPS', '3'))
KERNELS = ('nb.fill', 'nb.extent', 'nb.keys', 'nb.sort', 'nb.gather', 'nb.boxes', 'nb.search', 'nb.flags', 'sm.classify',
           'sm.sum', 'sm.dev')
BUILD = ('nb.fill', 'nb.extent', 'nb.keys', 'nb.sort', 'nb.gather', 'nb.boxes')


def med(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'reps': len(xs)}


def timed(ctx, fn):
    walls, per, last = [], {k: [] for k in KERNELS}, None
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
    return {'wall': med(walls), 'kernels': {k: med(v) for k, v in per.items() if v}}, last


def scene(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'gaussian':
        p = rng.normal(0, 1, (n, 3))
    else:
        f = n // 100
        centres = rng.uniform(-5, 5, (64, 3))
        p = np.concatenate([centres[rng.integers(0, 64, n - f)] + rng.normal(0, 0.05, (n - f, 3)),
                            rng.uniform(-30, 30, (f, 3))])
        p = p[rng.permutation(n)]
    return p.astype(np.float32)


def bench_scene(ctx, kind, n):
    p = torch.from_numpy(scene(kind, n, 7)).cuda()
    xyz = [(a, p[:, i].contiguous()) for i, a in enumerate('xyz')]
    g = torch.Generator(device='cuda').manual_seed(11)
    others = ('scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity', 'rot_0', 'rot_1', 'rot_2', 'rot_3')
    table = xyz + [(k, torch.randn(n, device='cuda', generator=g)) for k in others]
    chunk = torch.empty((n + 255) // 256 * 18, dtype=torch.float32, device='cuda')
    vertex = torch.empty(n * 4, dtype=torch.int32, device='cuda')
    shb = torch.empty(max(1, n), dtype=torch.uint8, device='cuda')
    res = {'rows': n, 'position_bytes': 12 * n}
    ms = []
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        ctx.dev_minmax([t for _, t in xyz])
        ms.append(ctx.kernel_stats('mm.partial')[0])
    y = med(ms[WARM:])
    y['GBps'] = 12 * n / (y['median_ms'] / 1e3) / 1e9
    res['yardstick_mm_partial'] = y
    res['chain_without_action'], _ = timed(ctx, lambda: ctx.dev_compressed_ply(table, [], chunk, vertex, shb))
    for k in (8, 32):
        r, _ = timed(ctx, lambda: ctx.dev_neighbor_dist(xyz, k))
        st = ctx.last_neighbor_stats()
        r['stats'] = st
        r['pairs_per_query'] = st['pairs'] / max(1, st['placed'])
        r['nodes_per_query'] = st['nodes'] / max(1, st['placed'])
        r['build_ms'] = sum(r['kernels'][b]['median_ms'] for b in BUILD)
        r['search_ms'] = r['kernels']['nb.search']['median_ms']
        r['search_pairs_per_second'] = st['pairs'] / (r['search_ms'] / 1e3)
        res[f'dist_k{k}'] = r
        print(kind, n, k, json.dumps({a: r[a] for a in ('build_ms', 'search_ms', 'pairs_per_query', 'nodes_per_query')}), flush=True)
        act = {'kind': 'filterOutliers', 'k': k, 'sigma': 1.0}
        w, out = timed(ctx, lambda: ctx.dev_compressed_ply(table, [act], chunk, vertex, shb))
        w['rows_kept'] = out[0]
        w['action_ms'] = w['wall']['median_ms'] - res['chain_without_action']['wall']['median_ms']
        res[f'filterOutliers_k{k}'] = w
        print(kind, n, k, 'filterOutliers', json.dumps({'action_ms': w['action_ms'], 'rows_kept': out[0]}), flush=True)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'neighbors.json')
    sizes = [int(a) for a in sys.argv[2:]] or [1_000_000, 10_000_000]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    res = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            res = json.load(f)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    ctx.set_profiling(True)
    res.update({'warmups': WARM, 'device': torch.cuda.get_device_name(0)})
    for n in sizes:
        for kind in ('gaussian', 'floaters'):
            res[f'{kind}_n{n}'] = bench_scene(ctx, kind, n)
            torch.cuda.empty_cache()
            with open(out_path, 'w') as f:
                json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main()
