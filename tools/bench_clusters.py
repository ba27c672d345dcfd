#!/usr/bin/env python3
"""Connected clusters and filterClusters (st_abi.h, "clusters") at 1M and 10M rows on bench_neighbors.py's
two scenes: `gaussian` (x, y, z ~ N(0, 1)) and `floaters` (99 % of the rows in 64 clusters of sigma
0.05 with centres in [-5, 5]^3, 1 % uniform in [-30, 30]^3, shuffled), float32.  The link radius is the
median dist_8 of the same table, and 4 and 16 times that.

  kernels    the library's HIP events (set_profiling) around its launches, summed per name over one
             st_dev_clusters: nb.extent, nb.keys, nb.sort, nb.gather, nb.boxes and cl.init -- together
             the build -- then cl.cliques (the flags and the hooks), cl.link, cl.flatten and cl.size;
             1 warm-up call, REPS (default 3) timed, medians.  `pairs` (d2 evaluations), `nodes` (box
             tests) and `unions` of st_ctx_last_cluster_stats per placed row beside them, with the
             components found and the largest one.
  beside     the k = 8 neighbour search (nb.search, and its pairs and nodes per row) on the same
             table: the same tree and comparable visits -- the existing number to measure against.
  whole      host wall clock of st_dev_clusters, and of filterClusters inside a chain:
             dev_compressed_ply over a 14-column device table with the one action (keep: 'largest') in
             front, beside the same call without it -- the difference is the action with its
             compaction and row gather.

Sizes from argv[2:] (default 1000000 10000000).  Writes out/clusters.json (or argv[1]); a file that
exists is extended, so the sizes can be measured one call at a time."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

import splat_hip as sh
from bench_neighbors import scene

WARM = 1
REPS = int(os.environ.get('REPS', '3'))
BUILD = ('nb.extent', 'nb.keys', 'nb.sort', 'nb.gather', 'nb.boxes', 'cl.init')
KERNELS = BUILD + ('cl.cliques', 'cl.link', 'cl.flatten', 'cl.size', 'cl.flags', 'nb.fill', 'nb.search')
FACTORS = (1, 4, 16)


def med(xs):
    return {'median_ms': statistics.median(xs), 'min_ms': min(xs), 'max_ms': max(xs), 'reps': len(xs)}


def timed(ctx, fn, reps=REPS):
    walls, per, last = [], {k: [] for k in KERNELS}, None
    for r in range(WARM + reps):
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


def bench_scene(ctx, kind, n):
    p = torch.from_numpy(scene(kind, n, 7)).cuda()
    xyz = [(a, p[:, i].contiguous()) for i, a in enumerate('xyz')]
    g = torch.Generator(device='cuda').manual_seed(11)
    others = ('scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity', 'rot_0', 'rot_1', 'rot_2', 'rot_3')
    table = xyz + [(k, torch.randn(n, device='cuda', generator=g)) for k in others]
    chunk = torch.empty((n + 255) // 256 * 18, dtype=torch.float32, device='cuda')
    vertex = torch.empty(n * 4, dtype=torch.int32, device='cuda')
    shb = torch.empty(max(1, n), dtype=torch.uint8, device='cuda')
    res = {'rows': n}
    r, dist = timed(ctx, lambda: ctx.dev_neighbor_dist(xyz, 8))
    st = ctx.last_neighbor_stats()
    base = float(dist[torch.isfinite(dist)].median())
    res['search_k8'] = {'search_ms': r['kernels']['nb.search']['median_ms'], 'wall': r['wall'],
                        'pairs_per_row': st['pairs'] / max(1, st['placed']), 'nodes_per_row': st['nodes'] / max(1, st['placed'])}
    res['median_dist_8'] = base
    del dist
    print(kind, n, 'k = 8 search', json.dumps(res['search_k8']), 'median dist_8', base, flush=True)
    res['chain_without_action'], _ = timed(ctx, lambda: ctx.dev_compressed_ply(table, [], chunk, vertex, shb))
    for f in FACTORS:
        radius = base * f
        r, _ = timed(ctx, lambda: ctx.dev_clusters(xyz, radius))
        st = ctx.last_cluster_stats()
        P = max(1, st['placed'])
        r.update(radius=radius, stats=st, pairs_per_row=st['pairs'] / P, nodes_per_row=st['nodes'] / P,
                 unions_per_row=st['unions'] / P, build_ms=sum(r['kernels'][b]['median_ms'] for b in BUILD))
        for name in ('cliques', 'link', 'flatten'):
            r[name + '_ms'] = r['kernels']['cl.' + name]['median_ms']
        r['link_over_search_k8'] = r['link_ms'] / res['search_k8']['search_ms']
        res[f'clusters_x{f}'] = r
        print(kind, n, f'radius x{f}', json.dumps({a: r[a] for a in ('build_ms', 'cliques_ms', 'link_ms', 'flatten_ms', 'pairs_per_row',
                                                                      'nodes_per_row', 'unions_per_row', 'link_over_search_k8')}),
              'components', st['components'], 'largest', st['largest'], flush=True)
        act = {'kind': 'filterClusters', 'radius': radius, 'keep': 'largest'}
        w, out = timed(ctx, lambda: ctx.dev_compressed_ply(table, [act], chunk, vertex, shb))
        w['rows_kept'] = out[0]
        w['action_ms'] = w['wall']['median_ms'] - res['chain_without_action']['wall']['median_ms']
        res[f'filterClusters_x{f}'] = w
        print(kind, n, f'radius x{f}', 'filterClusters', json.dumps({'action_ms': w['action_ms'], 'rows_kept': out[0]}), flush=True)
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'clusters.json')
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
