#!/usr/bin/env python3
"""The .splat / .spz encode kernels beside the PLY writer's interleave, and the .spz file form.

  kernels   k_splat_rows ("wr.splat", st_dev_splat_rows) and k_spz_planes ("wr.spz",
            st_dev_spz_image) at degrees 0 and 3, each beside k_ply_rows ("ply.rows",
            st_dev_ply_rows) on the same columns in the same process: interleaved rounds, the
            kernels' time from the library's HIP events (set_profiling); 3 warm-up rounds, REPS
            (default 10) timed, medians with min / max.  Bytes are algorithmic: the columns read
            once, the output written once -- 4 * 14 + 32 per splat for .splat, 4 * (14 + 3C) + 19 +
            3C for .spz, 2 * 4 * columns for ply.rows.  Both new kernels read the same column
            streams as the yardstick and write fewer bytes; reported is each one's bytes per
            second over the yardstick's, and the yardstick's own spread (max - min) / median.
  file      `in.ply out.spz` (ply_spz_file) of the SH-3 table, host wall clock, raw (gzip_level 0)
            and with the gzip member (level 6): what the deflate costs

Writes out/write_splat_spz.json (or argv[1])."""
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


def table(n, C):
    """a scene-like table: positions within the 12-bit range, scales, colours, unnormalised rotations"""
    scale = {'x': 20.0, 'y': 20.0, 'z': 20.0, 'scale_0': 1.5, 'scale_1': 1.5, 'scale_2': 1.5}
    shift = {'scale_0': -4.0, 'scale_1': -4.0, 'scale_2': -4.0}
    cols = []
    for k in sh.reader_columns(3 * C):
        a = torch.randn(n, dtype=torch.float32, device='cuda')
        a = a * (0.25 if k.startswith('f_rest') else scale.get(k, 1.0)) + shift.get(k, 0.0)
        cols.append((k, a))
    return cols


def bench(ctx, n, C, kernels):
    """kernels: [(key, profiling name, call(cols), bytes per splat)] run beside ply.rows on the same columns"""
    cols = table(n, C)
    R = 4 * len(cols)
    rows = torch.empty(n * R, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    t = {key: [] for key, *_ in kernels}
    t['ply_rows'] = []
    for r in range(WARM + REPS):
        for key, name, call, _ in kernels:
            ms = kernel_ms(ctx, name, lambda: call(cols))
            if r >= WARM:
                t[key].append(ms)
        ms = kernel_ms(ctx, 'ply.rows', lambda: ctx.dev_ply_rows(cols, rows))
        if r >= WARM:
            t['ply_rows'].append(ms)
    res = {'rows': n, 'columns': len(cols)}
    per = {key: b for key, _, _, b in kernels}
    per['ply_rows'] = 2 * R
    for key, ms in t.items():
        res[key] = stats(ms)
        res[key]['bytes_per_splat'] = per[key]
        res[key]['GBps'] = per[key] * n / (res[key]['median_ms'] / 1e3) / 1e9
    yard = res['ply_rows']
    res['yardstick_spread'] = (yard['max_ms'] - yard['min_ms']) / yard['median_ms']
    for key, *_ in kernels:
        res[key]['GBps_over_ply_rows'] = res[key]['GBps'] / yard['GBps']
    return res, cols


def main(n=10_000_000):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'write_splat_spz.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    ctx.set_profiling(True)
    res = {'warmups': WARM, 'device': torch.cuda.get_device_name(0)}
    splat_out = torch.empty(n * 32, dtype=torch.uint8, device='cuda')
    image = torch.empty(sh.spz_image_size(n, 15), dtype=torch.uint8, device='cuda')
    res['degree0_14_columns'], _ = bench(ctx, n, 0, [
        ('splat_rows', 'wr.splat', lambda cols: ctx.dev_splat_rows(cols, splat_out), 4 * 14 + 32),
        ('spz_planes', 'wr.spz', lambda cols: ctx.dev_spz_image(cols, image), 4 * 14 + 19)])
    print('degree0_14_columns', json.dumps(res['degree0_14_columns']), flush=True)
    res['degree3_59_columns'], cols = bench(ctx, n, 15, [
        ('spz_planes', 'wr.spz', lambda cols: ctx.dev_spz_image(cols, image), 4 * 59 + 19 + 45)])
    print('degree3_59_columns', json.dumps(res['degree3_59_columns']), flush=True)
    del splat_out, image
    # in.ply -> out.spz, raw and gzipped
    ctx.set_profiling(False)
    tmp = os.environ.get('TMPDIR', '/tmp')
    src, dst = os.path.join(tmp, 'st_bench_spz_in.ply'), os.path.join(tmp, 'st_bench_out.spz')
    try:
        ctx.dev_ply_file(cols, src)
        del cols
        torch.cuda.empty_cache()
        for level, reps in ((0, 3), (6, 2)):
            wall = []
            for r in range(1 + reps):
                t0 = time.perf_counter()
                rows, size, clamped = ctx.ply_spz_file(src, [], dst, gzip_level=level)
                if r >= 1:
                    wall.append((time.perf_counter() - t0) * 1e3)
            f = stats(wall)
            f.update(rows=rows, file_bytes=size, clamped=clamped, input_bytes=os.path.getsize(src))
            res[f'ply_spz_file_gzip{level}'] = f
            print(f'ply_spz_file_gzip{level}', json.dumps(f), flush=True)
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.unlink(p)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main(int(os.environ.get('N', '10000000')))
