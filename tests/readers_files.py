"""Helpers of the reader tests: where the planes and sections of a .spz / .ksplat file lie (from the
file's own header), and small builders of such files from a numpy generator."""
import struct

import numpy as np

SH_COUNT = (0, 9, 24, 45)
KS_BASE = (44, 24, 24)     # record bytes before the harmonics, per compression mode
KS_SH_BYTES = (4, 2, 1)
KS_COLOUR = (40, 20, 20)   # offset of the four colour / opacity bytes


# ---- layout from the headers ---------------------------------------------------------------------
def spz_planes(raw):
    """{plane: file offset} of an inflated .spz stream, its row count, f_rest count and version"""
    version, n = struct.unpack_from('<II', raw, 4)
    nsh = SH_COUNT[raw[12]] if raw[12] <= 3 else 0
    off = {'pos': 16, 'alpha': 16 + 9 * n, 'colour': 16 + 10 * n, 'scale': 16 + 13 * n, 'rot': 16 + 16 * n,
           'sh': 16 + 19 * n}
    return off, n, nsh, version


def ksplat_sections(data):
    """(mode, [{count, data_off, partial, stride, degree, storage}]) of a .ksplat file"""
    nsec = struct.unpack_from('<I', data, 4)[0]
    mode = struct.unpack_from('<H', data, 20)[0]
    cur = 4096 + 1024 * nsec
    out = []
    for si in range(nsec):
        h = 4096 + 1024 * si
        count, max_splats, _, buckets = struct.unpack_from('<IIII', data, h)
        storage = struct.unpack_from('<H', data, h + 20)[0]
        partial = struct.unpack_from('<I', data, h + 36)[0]
        degree = struct.unpack_from('<H', data, h + 40)[0]
        stride = KS_BASE[mode] + SH_COUNT[degree] * KS_SH_BYTES[mode]
        meta = 4 * partial + storage * buckets
        out.append(dict(count=count, data_off=cur + meta, partial=partial, stride=stride, degree=degree,
                        storage=storage, start=cur))
        cur += meta + stride * max_splats
    return mode, out


# ---- builders --------------------------------------------------------------------------------------
def spz_raw(rng, version, n, degree, fb):
    """an inflated .spz stream of random plane bytes"""
    body = rng.integers(0, 256, n * (19 + SH_COUNT[degree]), dtype=np.uint8).tobytes()
    return b'NGSP' + struct.pack('<IIBBBB', version, n, degree, fb, 1, 0) + body


def ksplat_file(mode, sections, min_h=0.0, max_h=0.0):
    """sections: dicts with count, max, degree, capacity, buckets, full, partial (sizes), block,
    storage (bytes per bucket, >= 12), quant, centres (float32 array of 3 * buckets) and records
    (uint8 array [max, stride])"""
    head = bytearray(4096 + 1024 * len(sections))
    head[0:2] = bytes([0, 1])
    struct.pack_into('<II', head, 4, len(sections), len(sections))
    struct.pack_into('<I', head, 16, sum(s['count'] for s in sections))
    struct.pack_into('<H', head, 20, mode)
    struct.pack_into('<ff', head, 36, min_h, max_h)
    parts = [head]
    for si, s in enumerate(sections):
        h = 4096 + 1024 * si
        stride = KS_BASE[mode] + SH_COUNT[s['degree']] * KS_SH_BYTES[mode]
        assert s['records'].shape == (s['max'], stride) and s['records'].dtype == np.uint8
        assert s['storage'] >= 12 and len(s['centres']) == 3 * s['buckets']
        struct.pack_into('<IIII', head, h, s['count'], s['max'], s['capacity'], s['buckets'])
        struct.pack_into('<f', head, h + 16, s['block'])
        struct.pack_into('<H', head, h + 20, s['storage'])
        struct.pack_into('<I', head, h + 24, s.get('quant', 0))
        struct.pack_into('<II', head, h + 32, s['full'], len(s['partial']))
        struct.pack_into('<H', head, h + 40, s['degree'])
        centres = np.asarray(s['centres'], np.float32).tobytes()
        parts += [np.asarray(s['partial'], '<u4').tobytes(), centres + bytes(s['storage'] * s['buckets'] - len(centres)),
                  s['records'].tobytes()]
    return bytes(head) + b''.join(bytes(p) for p in parts[1:])


def ksplat_section(rng, mode, degree, count, max_splats, storage, partial, capacity, full, buckets, records=None):
    """a section for ksplat_file: random block size, quantisation range and bucket centres, and
    records of random bytes (every f32 / half / byte pattern can occur) unless some are given"""
    stride = KS_BASE[mode] + SH_COUNT[degree] * KS_SH_BYTES[mode]
    if records is None:
        records = rng.integers(0, 256, (max_splats, stride), dtype=np.uint8)
    return dict(count=count, max=max_splats, degree=degree, capacity=capacity, buckets=buckets, full=full,
                partial=partial, block=float(rng.uniform(1, 8)), storage=storage, quant=int(rng.choice([0, 1000, 4095])),
                centres=rng.normal(0, 20, 3 * buckets).astype(np.float32), records=records)
