#!/usr/bin/env python3
"""The HTML viewer writer beside the compressed-PLY writer, from in.ply to the output file.

  input     N synthetic SH-3 splats (bench.py's synth_table distributions, made on the device) written
            once as a binary in.ply (untimed); N = 1M and 10M unless given as arguments
  chain     the CLI's `in.ply -r 0,45,0 --filterNaN out.*` (config 3's actions)
  html      ply_html_file into a fresh page-cache file per run, host wall clock
  cply      ply_compressed_ply_file the same way in this process; and, with --baseline-tree DIR, in
            child processes that alternate between this tree and DIR (a built checkout of the parent
            commit: the child imports DIR/splat-transform_amd/py and loads DIR's library), two
            rounds each: the refactored region list must cost nothing
  kernel    k_base64's time over one ply_html_file from the library's HIP events ("base64", one
            launch per 32 MiB of text), and its share of the HBM roof: (7/3 x input bytes) / time /
            8 TB/s -- 1 byte read, 4/3 written; and one launch over 384 MiB of random bytes in two
            segments (st_dev_base64), the rate without the launches' ramps

Every figure is the median of REPS runs after WARM warm runs, with the min and max beside it.
Writes out/write_html.json (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(os.environ.get('ST_BENCH_TREE') or ROOT, 'splat-transform_amd', 'py'))

WARM = 1
REPS = int(os.environ.get('REPS', '5'))
ACTS = [{'kind': 'rotate', 'value': (0, 45, 0)}, {'kind': 'filterNaN'}]
TEMPLATE = ('<!DOCTYPE html>\n<html>\n<head>\n<link rel="stylesheet" href="./index.css">\n</head>\n<body>\n'
            '<script type="module" src="./index.js"></script>\n<script type="module">\n'
            'main({ settings: fetch(settingsUrl).then(response => response.json()), content: fetch(contentUrl) });\n'
            '</script>\n</body>\n</html>\n',
            'body { margin: 0; }\ncanvas { width: 100%; height: 100%; }\n',
            'const main = (o) => o;\nexport { main };\n')


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def timed(fn, out):
    """WARM + REPS runs of fn(out), each into a fresh file: (wall ms per timed run, the last result)"""
    ms = []
    res = None
    for r in range(WARM + REPS):
        if os.path.exists(out):
            os.unlink(out)
        t0 = time.perf_counter()
        res = fn(out)
        if r >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    os.unlink(out)
    return ms, res


def write_input(ctx, n, path):
    from csv_bench import sh3_table
    cols = sh3_table(n)
    ctx.dev_ply_file(cols, path)
    del cols
    import torch
    torch.cuda.empty_cache()


def cply_only(src, out):
    """the child's job: ply_compressed_ply_file alone, on the tree ST_BENCH_TREE names"""
    import splat_hip as sh
    ctx = sh.Context(0)
    ms, res = timed(lambda o: ctx.ply_compressed_ply_file(src, ACTS, o), out)
    ctx.close()
    print(json.dumps({'lib': sh.LIB_PATH, 'result': list(res), 'ms': ms}))


def one_launch(ctx, torch, sh):
    """k_base64 over 384 MiB in one launch: two segments, the second at an odd address"""
    n = 384 << 20
    src = torch.randint(0, 256, (n + 8,), dtype=torch.uint8, device='cuda')
    segs = [src[:1001], src[1002:n + 1]]
    out = torch.empty(sh.base64_size(n), dtype=torch.uint8, device='cuda')
    ctx.set_profiling(True)
    ks = []
    for _ in range(WARM + REPS):
        ctx.reset_kernel_stats()
        assert ctx.dev_base64(segs, out) == out.numel()
        ctx.synchronize()
        ks.append(ctx.kernel_stats('base64')[0])
    ctx.set_profiling(False)
    k = stats(ks[WARM:])
    k['traffic_bytes'] = n * 7 // 3
    k['GBps'] = k['traffic_bytes'] / (k['median_ms'] / 1e3) / 1e9
    k['fraction_of_8TBps'] = k['GBps'] / 8000
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sizes', nargs='*', type=int, default=[1_000_000, 10_000_000])
    ap.add_argument('--out', default=os.path.join(ROOT, 'out', 'write_html.json'))
    ap.add_argument('--baseline-tree', help="a built checkout of the parent commit, timed in a child process")
    ap.add_argument('--cply-only', nargs=2, metavar=('IN', 'OUT'), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.cply_only:
        return cply_only(*a.cply_only)
    import torch

    import splat_hip as sh
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    tmp = os.environ.get('TMPDIR', '/tmp')
    src, out = os.path.join(tmp, 'st_bench_html_in.ply'), os.path.join(tmp, 'st_bench_html_out')
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    res = {'device': torch.cuda.get_device_name(0), 'warm': WARM, 'reps': REPS, 'sizes': {}}
    res['k_base64_one_launch'] = one_launch(ctx, torch, sh)
    print('one launch', json.dumps(res['k_base64_one_launch']), flush=True)
    try:
        for n in a.sizes:
            write_input(ctx, n, src)
            r = {'input_bytes': os.path.getsize(src)}
            # interleaved rounds would share the page cache's state; the three legs run one after the other
            ms, (m, C, csize) = timed(lambda o: ctx.ply_compressed_ply_file(src, ACTS, o), out)
            r['cply'] = dict(stats(ms), file_bytes=csize, rows=m)
            ms, (m2, C2, hsize) = timed(lambda o: ctx.ply_html_file(src, ACTS, TEMPLATE, o), out)
            assert (m2, C2) == (m, C)
            r['html'] = dict(stats(ms), file_bytes=hsize)
            if a.baseline_tree:
                legs = {'cply_child': ROOT, 'cply_baseline': os.path.abspath(a.baseline_tree)}
                ms = {k: [] for k in legs}
                for _ in range(2):
                    for k, tree in legs.items():
                        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--cply-only', src, out],
                                           env=dict(os.environ, ST_BENCH_TREE=tree), check=True,
                                           capture_output=True, text=True)
                        one = json.loads(p.stdout.strip().splitlines()[-1])
                        assert one['result'] == [m, C, csize] and one['lib'].startswith(tree)
                        ms[k] += one['ms']
                for k in legs:
                    r[k] = stats(ms[k])
            ctx.set_profiling(True)
            ks = []
            for _ in range(WARM + REPS):
                ctx.reset_kernel_stats()
                ctx.ply_html_file(src, ACTS, TEMPLATE, out)
                ctx.synchronize()
                k_ms, launches = ctx.kernel_stats('base64')
                ks.append(k_ms)
            ctx.set_profiling(False)
            os.unlink(out)
            k = stats(ks[WARM:])
            k['launches'] = launches
            k['traffic_bytes'] = csize * 7 // 3
            k['GBps'] = k['traffic_bytes'] / (k['median_ms'] / 1e3) / 1e9
            k['fraction_of_8TBps'] = k['GBps'] / 8000
            r['k_base64'] = k
            r['html_minus_cply_ms'] = r['html']['median_ms'] - r['cply']['median_ms']
            r['kernel_share_of_difference'] = k['median_ms'] / max(r['html_minus_cply_ms'], 1e-9)
            res['sizes'][str(n)] = r
            print(n, json.dumps(r), flush=True)
    finally:
        for p in (src, out):
            if os.path.exists(p):
                os.unlink(p)
        ctx.close()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
