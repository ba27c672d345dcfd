#!/usr/bin/env python3
"""The PLY writer's interleave kernel beside the reader's transpose, and the file form.

  kernel    k_ply_rows ("ply.rows", st_dev_ply_rows: columns -> rows) and k_ply_cols ("ply.cols",
            st_dev_ply_transpose: rows -> columns, unchanged by the writer's arrival) on the same
            table in the same process, the kernels' time from the library's HIP events
            (set_profiling).  Both move 2 x row bytes per row, so ply.cols is the yardstick.  Each
            round runs ply.rows, then ply.cols on the rows it wrote (the columns must come back
            bit for bit); 3 warm-up rounds, REPS (default 10) timed.  Reported: medians with min /
            max, ply.rows' ratio to the yardstick's median, and the yardstick's own spread
            (max - min) / median.
  tables    10M rows of 14 floats (56 B), 26 floats (104 B), 64 floats (256 B: a row stride of
            whole LDS bank rows) and 62 floats (SH-3 without normals, 248 B)
  file      the 248-byte table from HBM into a page-cache file (dev_ply_file: header + rows through
            the pinned ring), host wall clock, and GB/s of file bytes

Writes out/write_ply.json (or argv[1])."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import torch

import splat_hip as sh

WARM = 3
REPS = int(os.environ.get('REPS', '10'))


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def kernel_ms(ctx, name, fn):
    ctx.reset_kernel_stats()
    fn()
    ctx.synchronize()
    ms, launches = ctx.kernel_stats(name)
    assert launches == 1, (name, launches)
    return ms


def bench_table(ctx, n, ncol):
    R = 4 * ncol
    names = [f'c{i}' for i in range(ncol)]
    cols = [(k, torch.randn(n, dtype=torch.float32, device='cuda')) for k in names]
    rows = torch.empty(n * R, dtype=torch.uint8, device='cuda')
    back = [torch.empty(n, dtype=torch.float32, device='cuda') for _ in names]
    head = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {n}\n' +
            ''.join(f'property float {k}\n' for k in names) + 'end_header\n').encode()
    h = sh.ply_parse_header(head)
    torch.cuda.synchronize()

    t = {'ply_cols': [], 'ply_rows': []}
    for r in range(WARM + REPS):
        a = kernel_ms(ctx, 'ply.rows', lambda: ctx.dev_ply_rows(cols, rows))
        c = kernel_ms(ctx, 'ply.cols', lambda: ctx.dev_ply_transpose(h, 0, rows, back))
        if r >= WARM:
            t['ply_cols'].append(c), t['ply_rows'].append(a)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for (_, x), y in zip(cols, back)), 'rows -> cols did not give the columns back'
    res = {'rows': n, 'row_bytes': R, 'bytes_moved': 2 * R * n}
    for k, ms in t.items():
        res[k] = stats(ms)
        res[k]['GBps'] = 2 * R * n / (res[k]['median_ms'] / 1e3) / 1e9
    yard = res['ply_cols']
    res['yardstick_spread'] = (yard['max_ms'] - yard['min_ms']) / yard['median_ms']
    res['ply_rows']['vs_ply_cols'] = res['ply_rows']['median_ms'] / yard['median_ms']
    return res, cols


def main(n=10_000_000):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'write_ply.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    ctx.set_profiling(True)
    res = {'warmups': WARM, 'device': torch.cuda.get_device_name(0)}
    for key, ncol in (('f14_56B', 14), ('f26_104B', 26), ('r256B', 64), ('sh3_248B', 62)):
        res[key], cols = bench_table(ctx, n, ncol)
        print(key, json.dumps(res[key]), flush=True)
    # the last table (248-byte rows) into a page-cache file
    ctx.set_profiling(False)
    path = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'st_bench_write.ply')
    try:
        wall = []
        for r in range(1 + 3):
            t0 = time.perf_counter()
            size = ctx.dev_ply_file(cols, path)
            if r >= 1:
                wall.append((time.perf_counter() - t0) * 1e3)
        f = stats(wall)
        f['file_bytes'] = size
        f['file_GBps'] = size / (f['median_ms'] / 1e3) / 1e9
        res['sh3_248B_device_to_file'] = f
        print('sh3_248B_device_to_file', json.dumps(f), flush=True)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main(int(os.environ.get('N', '10000000')))
