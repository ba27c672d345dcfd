#!/usr/bin/env python3
"""The CSV writer's kernels and file form beside the PLY writer's, on one resident table.

  table     N (default 1M) rows of the 62 SH-3 float32 columns with bench.py's synth_table
            distributions (positions N(0,10^2) with 5% in a 1e-3 cube, f_dc N(0,1), f_rest
            N(0,0.1^2), opacity N(0,2^2), scale U(-7,-2), rot N(0,1)) and zero normals
  kernels   st_dev_csv_rows over the whole table: the library's HIP events (set_profiling) around
            k_csv_len ("csv.len"), the scan ("csv.scan") and k_csv_rows ("csv.rows").  A table of
            several pieces runs the length pass and the scan twice per piece (the size is known
            before a byte is written), the write pass once: the times are per launch x the
            launches one production of the text needs.  Rates are text bytes per second.
            k_ply_rows ("ply.rows") on the same table in the same rounds, as a reference point.
  files     dev_csv_file and dev_ply_file of the same table into page-cache files, host wall clock
  target    the kernels' text rate (length pass + scan + write pass) against 1.5 x the bytes per
            second dev_ply_file reaches in this session

Writes out/write_csv.json (or argv[1]) and, next to it, write_csv.md: the table for DESIGN.md."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import torch

import splat_hip as sh

WARM = 2
REPS = int(os.environ.get('REPS', '7'))


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def sh3_table(n, seed=20240):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    f = dict(device='cuda', dtype=torch.float32)
    cols = {}
    cube = torch.rand(n, generator=g, **f) < 0.05
    for a, off in zip('xyz', (1.0, -2.0, 3.0)):
        v = torch.randn(n, generator=g, **f) * 10
        c = off + torch.rand(n, generator=g, **f) * 1e-3
        cols[a] = torch.where(cube, c, v).contiguous()
    for a in ('nx', 'ny', 'nz'):
        cols[a] = torch.zeros(n, **f)
    for i in range(3):
        cols[f'f_dc_{i}'] = torch.randn(n, generator=g, **f)
    for i in range(45):
        cols[f'f_rest_{i}'] = torch.randn(n, generator=g, **f) * 0.1
    cols['opacity'] = torch.randn(n, generator=g, **f) * 2
    for i in range(3):
        cols[f'scale_{i}'] = torch.rand(n, generator=g, **f) * 5 - 7
    for i in range(4):
        cols[f'rot_{i}'] = torch.randn(n, generator=g, **f)
    return list(cols.items())


def main(n):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'write_csv.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    cols = sh3_table(n)
    assert len(cols) == 62
    bound = sh.csv_max_row_bytes(cols)
    text = torch.empty(n * 1300 + 4096, dtype=torch.uint8, device='cuda')
    rows = torch.empty(n * 248, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    res = {'device': torch.cuda.get_device_name(0), 'rows': n, 'columns': 62, 'max_row_bytes': bound,
           'warmups': WARM}

    ctx.set_profiling(True)
    t = {k: [] for k in ('csv_len', 'csv_scan', 'csv_rows', 'ply_rows')}
    launches = {}
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        size = ctx.dev_csv_rows(cols, text)
        ctx.dev_ply_rows(cols, rows)
        ctx.synchronize()
        one = {}
        for k in t:
            ms, cnt = ctx.kernel_stats(k.replace('_', '.'))
            launches[k] = cnt
            one[k] = ms
        # per production of the text: every piece's length pass and scan once
        pieces = launches['csv_rows']
        for k in ('csv_len', 'csv_scan'):
            one[k] *= pieces / launches[k]
        if r >= WARM:
            for k in t:
                t[k].append(one[k])
    ctx.set_profiling(False)
    res['text_bytes'] = size
    res['pieces'] = launches['csv_rows']
    for k, ms in t.items():
        res[k] = stats(ms)
        res[k]['GBps'] = (n * 248 * 2 if k == 'ply_rows' else size) / (res[k]['median_ms'] / 1e3) / 1e9
    all_ms = [a + b + c for a, b, c in zip(t['csv_len'], t['csv_scan'], t['csv_rows'])]
    res['csv_kernels'] = stats(all_ms)
    res['csv_kernels']['text_GBps'] = size / (res['csv_kernels']['median_ms'] / 1e3) / 1e9
    print(json.dumps({k: res[k] for k in ('csv_len', 'csv_scan', 'csv_rows', 'csv_kernels', 'ply_rows')}), flush=True)
    del text, rows

    tmp = os.environ.get('TMPDIR', '/tmp')
    paths = {'csv': os.path.join(tmp, 'st_bench_write.csv'), 'ply': os.path.join(tmp, 'st_bench_write.ply')}
    try:
        wall = {'csv': [], 'ply': []}
        sizes = {}
        for r in range(1 + 3):
            for k, fn in (('ply', ctx.dev_ply_file), ('csv', ctx.dev_csv_file)):
                t0 = time.perf_counter()
                sizes[k] = fn(cols, paths[k])
                if r >= 1:
                    wall[k].append((time.perf_counter() - t0) * 1e3)
        for k in wall:
            f = stats(wall[k])
            f['file_bytes'] = sizes[k]
            f['file_GBps'] = sizes[k] / (f['median_ms'] / 1e3) / 1e9
            res[f'dev_{k}_file'] = f
            print(f'dev_{k}_file', json.dumps(f), flush=True)
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.unlink(p)
    need = 1.5 * res['dev_ply_file']['file_GBps']
    res['target'] = {'kernels_text_GBps': res['csv_kernels']['text_GBps'], 'needed_GBps': need,
                     'met': res['csv_kernels']['text_GBps'] >= need}
    print('target', json.dumps(res['target']), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    md = ['| what | median ms (min - max) | rate |', '|---|---|---|']
    for k, label in (('csv_len', 'k_csv_len'), ('csv_scan', 'scan_u32'), ('csv_rows', 'k_csv_rows'),
                     ('csv_kernels', 'the three together')):
        s = res[k]
        md.append(f"| {label} | {s['median_ms']:.2f} ({s['min_ms']:.2f} - {s['max_ms']:.2f}) | "
                  f"{s.get('GBps', s.get('text_GBps')):.1f} GB/s of text |")
    s = res['ply_rows']
    md.append(f"| k_ply_rows, same table | {s['median_ms']:.2f} ({s['min_ms']:.2f} - {s['max_ms']:.2f}) | "
              f"{s['GBps']:.0f} GB/s read + written |")
    for k in ('csv', 'ply'):
        s = res[f'dev_{k}_file']
        md.append(f"| dev_{k}_file, {s['file_bytes'] / 1e6:.0f} MB into the page cache | {s['median_ms']:.0f} "
                  f"({s['min_ms']:.0f} - {s['max_ms']:.0f}) | {s['file_GBps']:.2f} GB/s of file |")
    with open(os.path.splitext(out_path)[0] + '.md', 'w') as f:
        f.write('\n'.join(md) + '\n')
    print('\n'.join(md))
    ctx.close()


if __name__ == '__main__':
    main(int(os.environ.get('N', '1000000')))
