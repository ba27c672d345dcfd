"""numpy restatement of the .ksplat writer's rules (include/st_abi.h, "the .ksplat writer") in float64:
one numpy operation per rounding, in the order the rules are written.  Math.exp is V8's, through the
oracle (write_splat_spz_ref.sigmoid / oracle_typed.exp).  Every comparison against it is on bytes.

A table is a list of (name, numpy array) or a dict, as in write_splat_spz_ref.

  plan(cols, block)            -> dict: order, bucket (per record), centres [F + P, 3] float32,
                                  partial_sizes, full, partial, clamped (and per row: key, row_clamped; lo)
  records(cols, mode, ...)     -> uint8 [n, stride] through a given grid (a file's own, or plan()'s)
  image(cols, mode, ...)       -> (bytes of the whole file, clamped)
"""
import struct

import numpy as np

import oracle_typed as ot
from write_splat_spz_ref import REQUIRED, SH_C0, f32_bits, num, q8, sigmoid, table, unit_quat

CELLS = 1 << 21
CAPACITY = 256
COEFFS = (0, 3, 8, 15)
DEGREE = {0: 0, 3: 1, 8: 2, 15: 3}
BASE = (44, 24, 24)
SH_BYTES = (4, 2, 1)


def stride(mode, C):
    return BASE[mode] + SH_BYTES[mode] * 3 * C


def half_bits(t):
    """H(t): round to nearest even from the double to binary16; NaN gives 0x7E00"""
    t = np.asarray(t, np.float64)
    with np.errstate(all='ignore'):
        h = t.astype(np.float16).view(np.uint16).copy()
    h[np.isnan(t)] = 0x7E00
    return h


def fround(d):
    with np.errstate(all='ignore'):
        return np.asarray(d, np.float64).astype(np.float32).astype(np.float64)


def f32_column_bits(a):
    """a float32 column's bits unchanged, other types Math.fround(v)"""
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else f32_bits(num(a))


def nearest(v, k0, top, decode):
    """of k0 - 1, k0, k0 + 1 inside [0, top] the code whose decoded value is nearest v: k0 unless a
    neighbour is strictly nearer; of two strictly nearer neighbours the nearer, k0 - 1 on a tie"""
    with np.errstate(all='ignore'):
        best, bd = k0.copy(), np.abs(decode(k0) - v)
        for step, ok in ((-1.0, k0 - 1.0 >= 0.0), (1.0, k0 + 1.0 <= top)):
            d = np.abs(decode(k0 + step) - v)
            take = ok & (d < bd)
            best = np.where(take, k0 + step, best)
            bd = np.where(take, d, bd)
    return best


def centre_decode(k, quant, ps, c):
    with np.errstate(all='ignore'):
        return fround((k - quant) * ps + c)


def centre_code(v, c, ps, quant):
    with np.errstate(all='ignore'):
        f = np.floor((v - c) / ps + 0.5) + quant
        nan = np.isnan(f)
        k0 = np.minimum(65535.0, np.maximum(0.0, np.where(nan, 0.0, f)))
        k = nearest(v, k0, 65535.0, lambda k: centre_decode(k, quant, ps, c))
    return np.where(nan, 0.0, k).astype(np.uint16)


def sh8_decode(b, lo, span):
    with np.errstate(all='ignore'):
        return fround(lo + (b / 255.0) * span)


def sh8_code(v, sh_min, sh_max):
    lo = float(np.float32(sh_min))
    span = float(np.float32(sh_max)) - lo
    with np.errstate(all='ignore'):
        k0 = q8((v - lo) / span * 255.0).astype(np.float64)
        k = nearest(v, k0, 255.0, lambda b: sh8_decode(b, lo, span))
    return np.where(np.isnan(v), 0.0, k).astype(np.uint8)


def sh_column(i, C):
    """the f_rest index of file component i in a table of C coefficients per channel (read-ksplat.ts:343-360)"""
    if i < 9:
        channel, coeff = i // 3, i % 3
    elif i < 24:
        channel, coeff = (i - 9) // 5, (i - 9) % 5 + 3
    else:
        channel, coeff = (i - 24) // 7, (i - 24) % 7 + 8
    return channel * C + coeff


def check_params(t, mode, degree, block, sh_min, sh_max):
    """(C of the table, C of the file, B, sh_min, sh_max as written) or ValueError naming the parameter"""
    if mode not in (0, 1, 2):
        raise ValueError('mode')
    C = ot.band_coeffs(set(t))
    if degree not in (-1, 0, 1, 2, 3) or degree > DEGREE[C]:
        raise ValueError('degree')
    with np.errstate(all='ignore'):
        B = float(np.float32(block))
    if not (np.isfinite(B) and B > 0):
        raise ValueError('block_size')
    lo, hi = np.float32(sh_min), np.float32(sh_max)
    if mode == 2 and not (np.isfinite(lo) and np.isfinite(hi) and lo != 0 and hi != 0 and lo < hi):
        raise ValueError('sh_min')
    if mode != 2:
        lo, hi = np.float32(-1.5), np.float32(1.5)
    return C, (C if degree < 0 else COEFFS[degree]), B, float(lo), float(hi)


def plan(cols, block=5.0):
    t = table(cols)
    n = len(t['x'])
    assert n > 0
    B = float(np.float32(block))
    los, cells, row_clamped = [], [], np.zeros(n, np.uint32)
    with np.errstate(all='ignore'):
        for name in 'xyz':
            v = num(t[name])
            fin = np.isfinite(v)
            lo = float(v[fin].min()) if fin.any() else 0.0
            f = np.floor((v - lo) / B)
            low = np.isnan(v) | (v < lo)
            row_clamped += (~fin | (~low & (f >= CELLS))).astype(np.uint32)
            cells.append(np.where(low, 0.0, np.minimum(CELLS - 1.0, np.where(np.isnan(f), 0.0, f))).astype(np.uint64))
            los.append(lo)
    key = (cells[2] << np.uint64(42)) | (cells[1] << np.uint64(21)) | cells[0]
    srt = np.argsort(key, kind='stable')
    ks = key[srt]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], n]
    full_rows, part_rows, full_cells, part_cells, sizes = [], [], [], [], []
    for s, e in zip(starts, ends):
        m = e - s
        nf = m // CAPACITY
        full_rows.append(srt[s:s + nf * CAPACITY])
        full_cells += [ks[s]] * nf
        if m % CAPACITY:
            part_rows.append(srt[s + nf * CAPACITY:e])
            part_cells.append(ks[s])
            sizes.append(m % CAPACITY)
    F, P = len(full_cells), len(part_cells)
    order = np.concatenate(full_rows + part_rows).astype(np.uint32)
    bucket = np.concatenate([np.repeat(np.arange(F), CAPACITY), np.repeat(F + np.arange(P), sizes)]).astype(np.uint32)
    bkeys = np.array(full_cells + part_cells, np.uint64)
    centres = np.zeros((F + P, 3), np.float32)
    for a in range(3):
        cell = ((bkeys >> np.uint64(21 * a)) & np.uint64(CELLS - 1)).astype(np.float64)
        centres[:, a] = (los[a] + (cell + 0.5) * B).astype(np.float32)
    return dict(order=order, bucket=bucket, centres=centres, partial_sizes=np.array(sizes, np.uint32), full=F,
                partial=P, clamped=int(row_clamped.sum()), lo=los, key=key, row_clamped=row_clamped)


def records(cols, mode, order=None, bucket=None, centres=None, degree=-1, block=5.0, quant=32767, sh_min=-1.5,
            sh_max=1.5, fields=None):
    """the records in file order.  order: source row of each record (None: the identity); bucket /
    centres: the grid (modes 1 and 2); block: a float32 value; quant: the quantisation range.
    fields: a dict that receives {field: (offset, bytes)} of the layout"""
    t = table(cols)
    for k in REQUIRED:
        if k not in t:
            raise KeyError(k)
    C = ot.band_coeffs(set(t))
    Cout = C if degree < 0 else COEFFS[degree]
    assert Cout <= C
    n = len(t['x'])
    order = np.arange(n) if order is None else np.asarray(order).astype(np.int64)
    m = len(order)

    def col(name):
        return np.asarray(t[name])[order]
    rec = np.zeros((m, stride(mode, Cout)), np.uint8)

    def put(off, words, width):
        rec[:, off:off + width] = np.ascontiguousarray(words.astype(f'<u{width}')).view(np.uint8).reshape(m, width)
    with np.errstate(all='ignore'):
        u = unit_quat({f'rot_{k}': col(f'rot_{k}') for k in range(4)})
        if mode == 0:
            for k, name in enumerate('xyz'):
                put(4 * k, f32_column_bits(col(name)), 4)
            for k in range(3):
                put(12 + 4 * k, f32_bits(ot.exp(num(col(f'scale_{k}')))), 4)
            for k in range(4):
                put(24 + 4 * k, f32_bits(u[k]), 4)
            colour_at, sh_at = 40, 44
        else:
            ps = float(np.float32(block)) / 2.0 / float(quant)
            cen = np.asarray(centres, np.float32).reshape(-1, 3)[np.asarray(bucket).astype(np.int64)].astype(np.float64)
            for k, name in enumerate('xyz'):
                put(2 * k, centre_code(num(col(name)), cen[:, k], ps, float(quant)), 2)
            for k in range(3):
                put(6 + 2 * k, half_bits(ot.exp(num(col(f'scale_{k}')))), 2)
            for k in range(4):
                put(12 + 2 * k, half_bits(u[k]), 2)
            colour_at, sh_at = 20, 24
        for k in range(3):
            rec[:, colour_at + k] = q8((num(col(f'f_dc_{k}')) * SH_C0 + 0.5) * 255.0)
        rec[:, colour_at + 3] = q8(sigmoid(num(col('opacity'))) * 255.0)
        for i in range(3 * Cout):
            a = col(f'f_rest_{sh_column(i, C)}')
            if mode == 0:
                put(sh_at + 4 * i, f32_column_bits(a), 4)
            elif mode == 1:
                put(sh_at + 2 * i, half_bits(num(a)), 2)
            else:
                rec[:, sh_at + i] = sh8_code(num(a), sh_min, sh_max)
    if fields is not None:
        w = SH_BYTES[mode]
        fields.update(centre=(0, 12 if mode == 0 else 6), scale=(12, 12) if mode == 0 else (6, 6),
                      rotation=(24, 16) if mode == 0 else (12, 8), colour=(colour_at, 4), harmonics=(sh_at, 3 * Cout * w))
    return rec


def headers(n, mode, Cout, B, sh_min, sh_max, F, P):
    head = bytearray(5120)
    head[1] = 1
    struct.pack_into('<IIII', head, 4, 1, 1, n, n)
    struct.pack_into('<H', head, 20, mode)
    struct.pack_into('<ff', head, 36, sh_min, sh_max)
    s = 4096
    struct.pack_into('<IIII', head, s, n, n, CAPACITY, F + P)
    struct.pack_into('<f', head, s + 16, B)
    struct.pack_into('<H', head, s + 20, 12)
    struct.pack_into('<I', head, s + 24, 32767)
    struct.pack_into('<II', head, s + 32, F, P)
    struct.pack_into('<H', head, s + 40, DEGREE[Cout])
    return bytes(head)


def image(cols, mode=1, degree=-1, block=5.0, sh_min=-1.5, sh_max=1.5):
    t = table(cols)
    C, Cout, B, lo, hi = check_params(t, mode, degree, block, sh_min, sh_max)
    n = len(t['x'])
    if n == 0:
        raise ValueError('n')
    p = plan(t, B)
    rec = records(t, mode, p['order'], p['bucket'], p['centres'], degree, B, 32767, lo, hi)
    out = (headers(n, mode, Cout, B, lo, hi, p['full'], p['partial']) + p['partial_sizes'].astype('<u4').tobytes()
           + p['centres'].astype('<f4').tobytes() + rec.tobytes())
    assert len(out) == 5120 + 4 * p['partial'] + 12 * (p['full'] + p['partial']) + n * stride(mode, Cout)
    return out, p['clamped']
