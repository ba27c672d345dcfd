#!/usr/bin/env python3
"""The .ksplat record kernel beside the PLY writer's interleave, the plan, and the .ksplat file form.

  kernels   k_ksplat_records ("wr.ksplat", st_dev_ksplat_records) at modes 0, 1 and 2 and degrees 0
            and 3, each beside k_ply_rows ("ply.rows", st_dev_ply_rows) on the same columns in the
            same process: interleaved rounds, the kernels' time from the library's HIP events
            (set_profiling); 3 warm-up rounds, REPS (default 10) timed, medians with min / max.
            Two cases per mode: `identity` -- the table permuted into bucket order beforehand, the
            kernel run with no order: the same coalesced column streams as the yardstick -- and
            `gathered` -- the table as it came, read through the plan's order.  Both write the same
            bytes.  Bytes are algorithmic: the columns read once, the records written once, plus 4
            (bucket) + 12 (centre) per splat in modes 1 and 2 and 4 (order) when gathered.
            The expectation: identity moves no fewer bytes per second than ply.rows in the same run,
            less the yardstick's own spread (max - min) / median; `meets_expectation` says so.  The
            gathered case has no target.
  plan      st_dev_ksplat_plan (keys, sort, buckets, tables) of the same table: host wall clock, and
            the library's events per stage
  file      `in.ply out.ksplat` (ply_ksplat_file) of the SH-3 table, mode 1, host wall clock

Writes out/write_ksplat.json (or argv[1])."""
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
STRIDE = {(0, 0): 44, (0, 15): 224, (1, 0): 24, (1, 15): 114, (2, 0): 24, (2, 15): 69}


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
    """a scene-like table: positions a few hundred units wide, scales, colours, unnormalised rotations"""
    scale = {'x': 60.0, 'y': 60.0, 'z': 20.0, 'scale_0': 1.5, 'scale_1': 1.5, 'scale_2': 1.5}
    shift = {'scale_0': -4.0, 'scale_1': -4.0, 'scale_2': -4.0}
    cols = []
    for k in sh.reader_columns(3 * C):
        a = torch.randn(n, dtype=torch.float32, device='cuda')
        a = a * (0.25 if k.startswith('f_rest') else scale.get(k, 1.0)) + shift.get(k, 0.0)
        cols.append((k, a))
    return cols


def bench(ctx, n, C):
    cols = table(n, C)
    t0 = time.perf_counter()
    plan = ctx.dev_ksplat_plan(cols)
    plan_first_ms = (time.perf_counter() - t0) * 1e3
    wall, stages = [], {}
    for r in range(1 + 3):
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        ctx.dev_ksplat_plan(cols)
        if r >= 1:
            wall.append((time.perf_counter() - t0) * 1e3)
            for name in ('ksw.keys', 'ksw.sort', 'ksw.buckets', 'ksw.assign'):
                stages.setdefault(name, []).append(ctx.kernel_stats(name)[0])
    res = {'rows': n, 'columns': len(cols), 'full': plan['full'], 'partial': plan['partial'],
           'plan': dict(stats(wall), first_call_ms=plan_first_ms,
                        stage_median_ms={k: statistics.median(v) for k, v in stages.items()})}
    order = plan['order'].long()
    ordered = [(k, a[order].contiguous()) for k, a in cols]
    R = 4 * len(cols)
    rows = torch.empty(n * R, dtype=torch.uint8, device='cuda')
    out = torch.empty(n * STRIDE[(0, C)] + 8, dtype=torch.uint8, device='cuda')
    centres = plan['centres'].contiguous()
    torch.cuda.synchronize()
    cases = []
    for mode in (0, 1, 2):
        grid = 0 if mode == 0 else 16
        per = R + STRIDE[(mode, C)] + grid
        cases.append((f'mode{mode}_identity', per,
                      lambda mode=mode: ctx.dev_ksplat_records(ordered, out, mode, None, plan['bucket'], centres)))
        cases.append((f'mode{mode}_gathered', per + 4,
                      lambda mode=mode: ctx.dev_ksplat_records(cols, out, mode, plan['order'], plan['bucket'], centres)))
    t = {key: [] for key, _, _ in cases}
    t['ply_rows'] = []
    for r in range(WARM + REPS):
        for key, _, call in cases:
            ms = kernel_ms(ctx, 'wr.ksplat', call)
            if r >= WARM:
                t[key].append(ms)
        ms = kernel_ms(ctx, 'ply.rows', lambda: ctx.dev_ply_rows(ordered, rows))
        if r >= WARM:
            t['ply_rows'].append(ms)
    per = {key: b for key, b, _ in cases}
    per['ply_rows'] = 2 * R
    for key, ms in t.items():
        res[key] = stats(ms)
        res[key]['bytes_per_splat'] = per[key]
        res[key]['GBps'] = per[key] * n / (res[key]['median_ms'] / 1e3) / 1e9
    yard = res['ply_rows']
    res['yardstick_spread'] = (yard['max_ms'] - yard['min_ms']) / yard['median_ms']
    for key, _, _ in cases:
        res[key]['GBps_over_ply_rows'] = res[key]['GBps'] / yard['GBps']
        if key.endswith('identity'):
            res[key]['meets_expectation'] = res[key]['GBps'] >= yard['GBps'] * (1 - res['yardstick_spread'])
    return res, cols


def main(n=10_000_000):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'write_ksplat.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    ctx.set_profiling(True)
    res = {'warmups': WARM, 'device': torch.cuda.get_device_name(0)}
    res['degree0_14_columns'], cols = bench(ctx, n, 0)
    print('degree0_14_columns', json.dumps(res['degree0_14_columns']), flush=True)
    del cols
    torch.cuda.empty_cache()
    res['degree3_59_columns'], cols = bench(ctx, n, 15)
    print('degree3_59_columns', json.dumps(res['degree3_59_columns']), flush=True)
    # in.ply -> out.ksplat
    ctx.set_profiling(False)
    tmp = os.environ.get('TMPDIR', '/tmp')
    src, dst = os.path.join(tmp, 'st_bench_ksplat_in.ply'), os.path.join(tmp, 'st_bench_out.ksplat')
    try:
        ctx.dev_ply_file(cols, src)
        del cols
        torch.cuda.empty_cache()
        wall = []
        for r in range(1 + 3):
            t0 = time.perf_counter()
            rows, size, clamped = ctx.ply_ksplat_file(src, [], dst, mode=1)
            if r >= 1:
                wall.append((time.perf_counter() - t0) * 1e3)
        f = stats(wall)
        f.update(rows=rows, file_bytes=size, clamped=clamped, input_bytes=os.path.getsize(src))
        res['ply_ksplat_file_mode1'] = f
        print('ply_ksplat_file_mode1', json.dumps(f), flush=True)
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
