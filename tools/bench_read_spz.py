#!/usr/bin/env python3
"""The device INFLATE of the .spz reader (st_dev_gunzip) beside the host gunzip it replaces.

For N (default 10,000,000) rows of the benchmark's distributions at degrees 0 and 3, and for three
members around the same image -- spz_deflate(level=6) (8 MiB zlib segments joined by sync flushes),
deflate='device' (st_dev_gzip's 64 KiB segments) and one plain zlib stream (zlib.compressobj(6), the
form of .spz files in the wild):

  kernels   st_dev_gunzip's kernels -- k_infl_find ("infl.find"), k_infl_size ("infl.size"),
            k_infl_write ("infl.write"), k_infl_tails ("infl.tails"), k_infl_resolve ("infl.resolve")
            and k_crc32 ("crc32") -- from the library's HIP events (set_profiling): 3 warm-up rounds,
            REPS (default 10) timed, medians with min / max; all of st_dev_gunzip by host wall clock
            in the same rounds; its statistics
  read      `in.spz -> device columns` (read_spz_dev) by host wall clock with inflate='host' and
            inflate='device', interleaved in one process: 1 warm-up and WALL_REPS (default 3) timed
            each; the ratio host / device; the device read's stages (file read, layout and head on
            the host, the one C call) and which way it went
  chunks    with CHUNKS="16384,32768,..." the kernel rounds again (3 timed) at those chunk sizes on
            the degree-3 plain zlib member: the measurement behind ST_INFLATE_CHUNK

Writes out/spz_inflate.json (or argv[1])."""
import gzip
import json
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import numpy as np
import torch

import splat_hip as sh

WARM = 3
REPS = int(os.environ.get('REPS', '10'))
WALL_REPS = int(os.environ.get('WALL_REPS', '3'))
KERNELS = ['infl.find', 'infl.size', 'infl.write', 'infl.tails', 'infl.resolve', 'crc32']


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'reps': len(ms)}


def table(n, C, seed=7):
    """bench.py's distributions"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    cols = []
    for k in sh.reader_columns(3 * C):
        if k.startswith('scale'):
            a = torch.rand(n, device='cuda', generator=g) * 5.0 - 7.0
        else:
            sd = 10.0 if k in ('x', 'y', 'z') else 0.1 if k.startswith('f_rest') else 2.0 if k == 'opacity' else 1.0
            a = torch.randn(n, device='cuda', generator=g) * sd
        cols.append((k, a.float()))
    return cols


def zlib_member(raw):
    """one gzip member around ONE zlib stream (no flush points): the form of files in the wild"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return (b'\x1f\x8b\x08\0\0\0\0\0\0\xff' + c.compress(raw) + c.flush() +
            struct.pack('<II', zlib.crc32(raw), len(raw) & 0xffffffff))


def kernels(ctx, member, out, chunk_bytes, reps):
    """rounds of st_dev_gunzip -> per-kernel statistics, the whole call's wall clock, the statistics"""
    t = {k: [] for k in KERNELS}
    wall, st = [], None
    for r in range(WARM + reps):
        ctx.reset_kernel_stats()
        ctx.synchronize()
        t0 = time.perf_counter()
        st = ctx.dev_gunzip(member, out, chunk_bytes=chunk_bytes)
        ms = (time.perf_counter() - t0) * 1e3
        assert st is not None, ('declined', ctx.last_inflate_stats)
        for k in t:
            kms, launches = ctx.kernel_stats(k)
            assert launches == 1, (k, launches)
            if r >= WARM:
                t[k].append(kms)
        if r >= WARM:
            wall.append(ms)
    res = {'member_bytes': member.numel(), 'image_bytes': out.numel(), 'chunk_bytes': chunk_bytes or sh.INFLATE_CHUNK,
           'stats': st, 'st_dev_gunzip_wall': stats(wall)}
    for k, ms in t.items():
        res[k] = stats(ms)
    res['kernels_total'] = stats([sum(t[k][i] for k in KERNELS) for i in range(reps)])
    for k in ('st_dev_gunzip_wall', 'kernels_total'):
        res[k]['output_GBps'] = out.numel() / (res[k]['median_ms'] / 1e3) / 1e9
    return res


def read_walls(ctx, path):
    """in.spz -> device columns both ways, interleaved"""
    wall = {'host': [], 'device': []}
    went, stages = None, {}
    for r in range(1 + WALL_REPS):
        for way in ('host', 'device'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cols = ctx.read_spz_dev(path, inflate=way)
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            del cols
            if way == 'device':
                went = ctx.last_inflate
            if r >= 1:
                wall[way].append(ms)
    # the device read's stages, once more by hand
    t0 = time.perf_counter()
    with open(path, 'rb') as f:
        file = f.read()
    t1 = time.perf_counter()
    lay = sh.spz_gz_layout(file)
    t2 = time.perf_counter()
    stages = {'file_read_ms': (t1 - t0) * 1e3, 'layout_and_head_host_ms': (t2 - t1) * 1e3, 'layout': lay}
    t0 = time.perf_counter()
    raw = gzip.decompress(file)
    stages['gzip_decompress_alone_ms'] = (time.perf_counter() - t0) * 1e3
    stages['gzip_decompress_MBps'] = len(raw) / stages['gzip_decompress_alone_ms'] / 1e3
    res = {'host': stats(wall['host']), 'device': stats(wall['device']), 'device_read_went': went, 'stages': stages}
    res['host_over_device'] = res['host']['median_ms'] / res['device']['median_ms']
    return res


def main(n):
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'out', 'spz_inflate.json')
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(0)
    res = {'warmups': WARM, 'rows': n, 'device': torch.cuda.get_device_name(0), 'zlib': zlib.ZLIB_RUNTIME_VERSION}
    tmp = os.environ.get('TMPDIR', '/tmp')
    path = os.path.join(tmp, 'st_bench_infl_in.spz')
    sweep = [int(x) for x in os.environ.get('CHUNKS', '').split(',') if x]
    try:
        for key, C in (('degree0', 0), ('degree3', 15)):
            cols = table(n, C)
            image = torch.empty(sh.spz_image_size(n, C), dtype=torch.uint8, device='cuda')
            ctx.dev_spz_image(cols, image)
            dev_member = torch.empty(sh.gzip_bound(image.numel()), dtype=torch.uint8, device='cuda')
            size = ctx.dev_gzip(image, dev_member)
            raw = image.cpu().numpy().tobytes()
            members = {'device_deflate': dev_member[:size].cpu().numpy().tobytes()}
            del cols, dev_member
            t0 = time.perf_counter()
            members['spz_deflate_level6'] = sh.spz_deflate(raw, 6)
            t1 = time.perf_counter()
            members['zlib_single_stream'] = zlib_member(raw)
            print(key, 'host deflate s', round(t1 - t0, 1), round(time.perf_counter() - t1, 1), flush=True)
            del raw
            for mk, blob in members.items():
                name = f'{key}_{mk}'
                member = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
                ctx.set_profiling(True)
                res['kernels_' + name] = kernels(ctx, member, image, 0, REPS)
                print('kernels_' + name, json.dumps(res['kernels_' + name]), flush=True)
                if sweep and name == 'degree3_zlib_single_stream':
                    for cb in sweep:
                        res[f'chunks_{cb}'] = kernels(ctx, member, image, cb, 3)
                        print(f'chunks_{cb}', json.dumps(res[f'chunks_{cb}']), flush=True)
                ctx.set_profiling(False)
                del member
                with open(path, 'wb') as f:
                    f.write(blob)
                res['read_' + name] = read_walls(ctx, path)
                print('read_' + name, json.dumps(res['read_' + name]), flush=True)
            del image, members
            torch.cuda.empty_cache()
    finally:
        if os.path.exists(path):
            os.unlink(path)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({'written': out_path}))
    ctx.close()


if __name__ == '__main__':
    main(int(os.environ.get('N', '10000000')))
