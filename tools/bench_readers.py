#!/usr/bin/env python3
"""The .splat / .ksplat / .spz decode kernels at 10M splats, beside the PLY transpose.

  decode    st_dev_*_decode of synthetic bytes already in HBM: the decode kernel's time from the
            library's HIP events (KTimer "rd.splat" / "rd.ksplat" / "rd.spz": set_profiling) and
            its algorithmic rate, record bytes in + 4 * (14 + D) bytes out per splat
  yardstick k_ply_cols ("ply.cols", st_dev_ply_transpose) on a 14-float-column PLY of the same n in
            the same run: the same kind of work (packed records -> float32 columns) without the
            arithmetic; 2 * 56 bytes per row.  Each format's rate is also given as a ratio to it
  file      .splat only: the file (page cache) -> device columns, host wall clock around
            read_splat_dev ending in a synchronise (the pread and the pinned copies are host work)

3 warm-ups and REPS (default 10) timed repetitions each; medians, with min / max.
Writes out/readers.json (or argv[1])."""
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

WARM = 3
REPS = int(os.environ.get('REPS', '10'))
SH = [0, 9, 24, 45]


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def kernel_times(ctx, name, fn):
    """per-repetition device time of the kernels named `name` inside fn()"""
    out = []
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        fn()
        ctx.synchronize()
        ms, launches = ctx.kernel_stats(name)
        assert launches >= 1, name
        if r >= WARM:
            out.append(ms)
    return out


def rate(res, bytes_per_splat, n):
    res['bytes_per_splat'] = bytes_per_splat
    res['GBps'] = bytes_per_splat * n / (res['median_ms'] / 1e3) / 1e9
    return res


def splat_bytes(n, rng):
    rows = np.empty((n, 8), np.uint32)
    rows[:, 0:3] = rng.standard_normal((n, 3), dtype=np.float32).view(np.uint32)
    rows[:, 3:6] = np.exp(rng.standard_normal((n, 3), dtype=np.float32) - 3).view(np.uint32)
    rows[:, 6:8] = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint32)
    return rows.reshape(-1).view(np.uint8)


def ksplat_bytes(n, mode, degree, rng):
    """one section of n splats in full buckets of 256"""
    base, hb = ((44, 4), (24, 2), (24, 1))[mode]
    stride = base + SH[degree] * hb
    buckets = n // 256
    head = np.zeros(4096 + 1024, np.uint8)
    u32 = head.view(np.uint32)
    head[1] = 1
    u32[1] = 1
    u32[4] = n
    head.view(np.uint16)[10] = mode
    s = head[4096:].view(np.uint32)
    s[0] = n
    s[1] = n
    s[2] = 256
    s[3] = buckets + 1
    head[4096:].view(np.float32)[4] = 5.0
    head[4096:].view(np.uint16)[10] = 12
    s[8] = buckets
    s[9] = 1
    head[4096:].view(np.uint16)[20] = degree
    sizes = np.array([n - buckets * 256], np.uint32).view(np.uint8)
    centres = rng.standard_normal((buckets + 1) * 3, dtype=np.float32).view(np.uint8)
    if mode == 0:
        rec = rng.standard_normal((n, stride // 4), dtype=np.float32)
        rec[:, 3:6] = np.exp(rec[:, 3:6] - 3)
        rec = rec.view(np.uint8)
    else:  # random bits: every half-float exponent, NaN and Inf included
        rec = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    return np.concatenate([head, sizes, centres, rec.reshape(-1)]), stride


def spz_bytes(n, version, degree, rng):
    head = np.zeros(16, np.uint8)
    head[:4] = np.frombuffer(b'NGSP', np.uint8)
    head.view(np.uint32)[1] = version
    head.view(np.uint32)[2] = n
    head[12] = degree
    head[13] = 12
    per = 19 + SH[degree]
    return np.concatenate([head, rng.integers(0, 256, n * per, dtype=np.uint8)]), per


def main(n=10_000_000):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'readers.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.set_profiling(True)
    rng = np.random.default_rng(7)
    res = {'splats': n, 'warmups': WARM, 'device': torch.cuda.get_device_name(0)}

    def columns(nsh):
        cols = {k: torch.empty(n, dtype=torch.float32, device='cuda') for k in sh.reader_columns(nsh)}
        torch.cuda.synchronize()
        return cols

    # the yardstick: 14 float properties, 56-byte rows
    head = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {n}\n' +
            ''.join(f'property float {k}\n' for k in sh.reader_columns(0)) + 'end_header\n').encode()
    h = sh.ply_parse_header(head)
    rows = torch.from_numpy(rng.standard_normal(n * 14, dtype=np.float32).view(np.uint8)).cuda()
    cols = list(columns(0).values())
    res['ply_cols'] = rate(stats(kernel_times(ctx, 'ply.cols', lambda: ctx.dev_ply_transpose(h, 0, rows, cols))), 2 * 56, n)
    del rows, cols
    yard = res['ply_cols']['GBps']

    def record(key, r, bytes_per_splat):
        r = rate(r, bytes_per_splat, n)
        r['vs_ply_cols'] = r['GBps'] / yard
        res[key] = r
        print(key, json.dumps(r), flush=True)

    print('ply_cols', json.dumps(res['ply_cols']), flush=True)

    host = splat_bytes(n, rng)
    dev = torch.from_numpy(host).cuda()
    cols = columns(0)
    record('splat', stats(kernel_times(ctx, 'rd.splat', lambda: ctx.dev_splat_decode(dev, cols))), 32 + 56)
    del dev
    # file -> device columns (page cache warm after the first read)
    path = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'st_bench_readers.splat')
    host.tofile(path)
    try:
        wall = []
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            got = ctx.read_splat_dev(path)
            ctx.synchronize()
            if r >= WARM:
                wall.append((time.perf_counter() - t0) * 1e3)
        ctx.reset_kernel_stats()
        f = stats(wall)
        f['file_GBps'] = host.nbytes / (f['median_ms'] / 1e3) / 1e9
        res['splat_file_to_columns'] = f
        print('splat_file_to_columns', json.dumps(f), flush=True)
        del got
    finally:
        os.unlink(path)
    del host, cols

    for mode, degree in ((0, 2), (1, 2), (2, 2), (2, 1), (1, 0)):
        host, stride = ksplat_bytes(n, mode, degree, rng)
        dev = torch.from_numpy(host).cuda()
        cols = columns(SH[degree])
        headers = host[:8192 + 4].tobytes()
        record(f'ksplat_m{mode}_d{degree}',
               stats(kernel_times(ctx, 'rd.ksplat', lambda: ctx.dev_ksplat_decode(headers, dev, cols))),
               stride + 4 * (14 + SH[degree]))
        del host, dev, cols

    for version, degree in ((2, 0), (2, 3), (3, 3)):
        host, per = spz_bytes(n, version, degree, rng)
        dev = torch.from_numpy(host).cuda()
        cols = columns(SH[degree])
        record(f'spz_v{version}_d{degree}', stats(kernel_times(ctx, 'rd.spz', lambda: ctx.dev_spz_decode(dev, cols))),
               per + 4 * (14 + SH[degree]))
        del host, dev, cols

    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main(int(os.environ.get('N', '10000000')))
