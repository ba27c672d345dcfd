#!/usr/bin/env python3
"""The device DEFLATE of the .spz writer (st_dev_gzip) beside the plane kernel, the host deflate and
the raw file.

  kernels   st_dev_gzip's kernels -- k_defl_hist ("defl.hist"), k_defl_plan ("defl.plan"),
            k_defl_scan ("defl.scan"), k_defl_emit ("defl.emit") and k_crc32 ("crc32") -- beside k_spz_planes ("wr.spz",
            st_dev_spz_image) on the same table in the same process: interleaved rounds, times from
            the library's HIP events (set_profiling); 3 warm-up rounds, REPS (default 10) timed,
            medians with min / max, GB/s of input (the image's bytes).  Degrees 0 and 3 of the
            benchmark's distributions, and degree 3 with every harmonic of half the rows exactly 0.
  file      `in.ply out.spz` (ply_spz_file) of the SH-3 table by host wall clock, interleaved: raw
            (gzip_level 0), deflate='host' (level 6, spz_deflate) and deflate='device'
  sizes     the device member beside spz_deflate at levels 6 and 1 and zlib's Z_RLE strategy in the
            same 64 KiB segments, on both SH-3 tables at N rows and at the tests' 200,000

Writes out/spz_deflate.json (or argv[1]).  N (default 10,000,000) rows.

Another segment size: build st_deflate.hip with -DST_DEFL_SEG_TRIAL=32768 into a library of its own
(tools/ab/), and run this tool with ST_LIB=<that library> SEG=32768 (the size the Z_RLE column uses
and the result records)."""
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import torch

import splat_hip as sh

WARM = 3
REPS = int(os.environ.get('REPS', '10'))
DEFL = ['defl.hist', 'defl.plan', 'defl.scan', 'defl.emit', 'crc32']


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def table(n, C, zero_rows, seed=7):
    """bench.py's distributions; zero_rows: every harmonic of half the rows exactly 0"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    zero = torch.rand(n, device='cuda', generator=g) < 0.5
    cols = []
    for k in sh.reader_columns(3 * C):
        if k.startswith('scale'):
            a = torch.rand(n, device='cuda', generator=g) * 5.0 - 7.0
        else:
            sd = 10.0 if k in ('x', 'y', 'z') else 0.1 if k.startswith('f_rest') else 2.0 if k == 'opacity' else 1.0
            a = torch.randn(n, device='cuda', generator=g) * sd
            if zero_rows and k.startswith('f_rest'):
                a[zero] = 0
        cols.append((k, a.float()))
    return cols


def kernels(ctx, cols, image, out):
    """interleaved rounds of st_dev_spz_image and st_dev_gzip -> per-kernel statistics, the member's size"""
    t = {k: [] for k in ['wr.spz'] + DEFL}
    size = 0
    for r in range(WARM + REPS):
        ctx.reset_kernel_stats()
        ctx.dev_spz_image(cols, image)
        size = ctx.dev_gzip(image, out)
        ctx.synchronize()
        for k in t:
            ms, launches = ctx.kernel_stats(k)
            assert launches == 1, (k, launches)
            if r >= WARM:
                t[k].append(ms)
    res = {'image_bytes': image.numel(), 'member_bytes': size}
    for k, ms in t.items():
        res[k] = stats(ms)
        res[k]['input_GBps'] = image.numel() / (res[k]['median_ms'] / 1e3) / 1e9
    total = [sum(t[k][i] for k in DEFL) for i in range(REPS)]
    res['gzip_kernels_total'] = stats(total)
    res['gzip_kernels_total']['input_GBps'] = image.numel() / (res['gzip_kernels_total']['median_ms'] / 1e3) / 1e9
    return res


SEG = int(os.environ.get('SEG', sh.DEFLATE_SEG))


def rle_segments(raw, seg=SEG):
    """zlib's Z_RLE strategy on independent segments, each ended with a sync flush"""
    mv = memoryview(raw)

    def one(o):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        return len(c.compress(mv[o:o + seg])) + len(c.flush(zlib.Z_SYNC_FLUSH))
    with ThreadPoolExecutor(16) as pool:
        return sum(pool.map(one, range(0, len(raw), seg), chunksize=256)) + 18


def sizes(ctx, n, zero_rows):
    cols = table(n, 15, zero_rows)
    image = torch.empty(sh.spz_image_size(n, 15), dtype=torch.uint8, device='cuda')
    out = torch.empty(sh.gzip_bound(image.numel()), dtype=torch.uint8, device='cuda')
    ctx.dev_spz_image(cols, image)
    member = ctx.dev_gzip(image, out)
    raw = image.cpu().numpy()
    del cols, image, out
    res = {'rows': n, 'raw': len(raw), 'device_member': member, 'host_level6': len(sh.spz_deflate(raw, 6)),
           'host_level1': len(sh.spz_deflate(raw, 1)), 'zlib_rle_64KiB_segments': rle_segments(raw)}
    for k in ('device_member', 'host_level6', 'host_level1', 'zlib_rle_64KiB_segments'):
        res[k + '_ratio'] = round(res[k] / len(raw), 4)
    return res


def main(n):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'spz_deflate.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    res = {'warmups': WARM, 'rows': n, 'segment_bytes': SEG, 'device': torch.cuda.get_device_name(0)}
    ctx.set_profiling(True)
    for key, C, zero_rows in (('degree0', 0, False), ('degree3', 15, False), ('degree3_zero_rows', 15, True)):
        cols = table(n, C, zero_rows)
        image = torch.empty(sh.spz_image_size(n, C), dtype=torch.uint8, device='cuda')
        out = torch.empty(sh.gzip_bound(image.numel()), dtype=torch.uint8, device='cuda')
        res['kernels_' + key] = kernels(ctx, cols, image, out)
        print('kernels_' + key, json.dumps(res['kernels_' + key]), flush=True)
        del cols, image, out
    ctx.set_profiling(False)
    torch.cuda.empty_cache()
    for rows in sorted({n, 200_000}):
        for zero_rows in (False, True):
            key = f'sizes_{rows}' + ('_zero_rows' if zero_rows else '')
            res[key] = sizes(ctx, rows, zero_rows)
            print(key, json.dumps(res[key]), flush=True)
    # in.ply -> out.spz: raw, host deflate, device deflate, interleaved
    tmp = os.environ.get('TMPDIR', '/tmp')
    src, dst = os.path.join(tmp, 'st_bench_defl_in.ply'), os.path.join(tmp, 'st_bench_defl_out.spz')
    forms = {'raw': dict(gzip_level=0), 'host_level6': dict(gzip_level=6), 'device': dict(deflate='device')}
    wall = {k: [] for k in forms}
    info = {}
    try:
        cols = table(n, 15, False)
        ctx.dev_ply_file(cols, src)
        del cols
        torch.cuda.empty_cache()
        for r in range(1 + 5):
            for k, kw in forms.items():
                if k == 'host_level6' and r > 2:
                    continue  # seconds each: one warm-up and two timed
                t0 = time.perf_counter()
                rows, size, clamped = ctx.ply_spz_file(src, [], dst, **kw)
                ms = (time.perf_counter() - t0) * 1e3
                if r >= 1:
                    wall[k].append(ms)
                info[k] = {'rows': rows, 'file_bytes': size, 'clamped': clamped}
        for k in forms:
            res['ply_spz_file_' + k] = dict(stats(wall[k]), input_bytes=os.path.getsize(src), **info[k])
            print('ply_spz_file_' + k, json.dumps(res['ply_spz_file_' + k]), flush=True)
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
