#!/usr/bin/env python3
"""The .sog reader at 1M and 10M SH-3 splats, on files made by `sog_file` (st_dev_sog_file):

  * per texture, the host VP8L decode (st_webp_decode_lossless, one thread) in ms and MPix/s,
    and Pillow's libwebp decoding the same bytes on the same box where Pillow imports, for scale;
  * k_sog_decode alone (st_dev_sog_decode on resident textures) from the library's HIP events,
    with the bytes it moves (20 B of per-splat texels + 8 B of label and 4 C B of palette row
    read, 56 + 12 C B written: 276 B per splat at SH-3) and its share of the HBM roof;
  * the whole read_sog (file -> host columns) and read_sog_dev (file -> device columns) by the
    host's wall clock, one warm run and the median of three.

    python3 tools/bench_read_sog.py [N ...]      writes profiles/read_sog.json
"""
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'splat-transform_amd', 'py'))

import numpy as np
import torch

import splat_hip as sh
from bench import synth_table

HBM_ROOF_GBPS = 8000.0  # MI355X HBM3E peak


def wall(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def measure(ctx, n, dev, tmp):
    C = 15
    cols = synth_table(n, 1002, dev)
    draws = np.random.default_rng(42).random(2 * 65536 * 12)
    W, H, pal, cw, ch = sh.sog_geometry(n, C)
    u8 = dict(device=dev, dtype=torch.uint8)
    tex = {k: torch.empty(W * H * 4, **u8) for k in ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_labels')}
    tex['shN_centroids'] = torch.empty(cw * ch * 4, **u8)
    path = os.path.join(tmp, f'read_{n}.sog')
    meta, _, size = ctx.dev_sog_file(cols, 2, draws, tex, path)
    del cols
    data = open(path, 'rb').read()
    index = {nm: (off, sz) for nm, off, sz, _ in sh.zip_index(data)}
    rec = {'splats': n, 'texture': [W, H], 'shN_centroids': [cw, ch], 'file_bytes': size, 'textures': {}}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for name in sh.SOG_FILES:
        off, sz = index[name]
        blob = data[off:off + sz]
        w, h = sh.webp_info(blob)
        ms = wall(lambda: sh.webp_decode_lossless(blob))
        t = {'bytes': sz, 'pixels': w * h, 'decode_ms': ms, 'mpix_per_s': w * h / ms / 1e3}
        if Image is not None:
            t['libwebp_decode_ms'] = wall(lambda: np.asarray(Image.open(io.BytesIO(blob)).convert('RGBA')))
        rec['textures'][name] = t
        print(n, name, t, flush=True)
    rec['decode_sum_ms'] = sum(t['decode_ms'] for t in rec['textures'].values())
    rec['decode_longest_ms'] = max(t['decode_ms'] for t in rec['textures'].values())
    if Image is not None:
        rec['libwebp_decode_sum_ms'] = sum(t['libwebp_decode_ms'] for t in rec['textures'].values())
    # the kernel alone on the resident textures
    out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in sh.reader_columns(3 * C)}
    ctx.dev_sog_decode(meta, n, tex, out)
    ctx.set_profiling(True)
    ctx.reset_kernel_stats()
    reps = 5
    for _ in range(reps):
        ctx.dev_sog_decode(meta, n, tex, out)
    ctx.synchronize()
    ms, launches = ctx.kernel_stats('rd.sog')
    ctx.set_profiling(False)
    nbytes = n * (20 + 8 + 4 * C + 56 + 12 * C)
    k_ms = ms / max(launches, 1)
    rec['kernel'] = {'ms': k_ms, 'bytes': nbytes, 'GBps': nbytes / k_ms / 1e6,
                     'hbm_roof_share': nbytes / k_ms / 1e6 / HBM_ROOF_GBPS}
    del out, tex
    rec['read_sog_ms'] = wall(lambda: ctx.read_sog(path))
    rec['read_sog_dev_ms'] = wall(lambda: (ctx.read_sog_dev(path), torch.cuda.synchronize()))
    print(json.dumps(rec), flush=True)
    return rec


def main(sizes):
    dev = torch.device('cuda', 0)
    s = torch.cuda.Stream(dev)
    torch.cuda.set_stream(s)
    ctx = sh.Context(0)
    ctx.set_stream(s.cuda_stream)
    with tempfile.TemporaryDirectory(prefix='st_read_sog_') as tmp:
        runs = [measure(ctx, n, dev, tmp) for n in sizes]
    out = {'device': torch.cuda.get_device_name(0), 'host_threads_per_read': 7, 'runs': runs}
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'read_sog.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main([int(a) for a in sys.argv[1:]] or [1_000_000, 10_000_000])
