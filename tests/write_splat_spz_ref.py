"""numpy restatement of the .splat and .spz writers' encode rules (include/st_abi.h, "the .splat and
.spz writers") in float64: one numpy operation per rounding, in the order the rules are written.
Math.exp is V8's, through the oracle's st_o_exp_n (oracle_typed.exp), as tests/sog_read_ref.py does.
Every comparison against it is on bytes.

A table is a list of (name, numpy array) or a dict; arrays of any of the eight column types.  The
first column of a name wins; columns the format does not use are ignored.

  splat_rows(cols)        -> uint8 [n, 32]
  spz_planes(cols, fb)    -> ({plane: uint8 [n, bytes per splat]}, clamped) in PLANES order
  spz_image(cols, fb)     -> (bytes of header + planes, clamped)
"""
import struct

import numpy as np

import oracle_typed as ot

REQUIRED = ['x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
            'rot_0', 'rot_1', 'rot_2', 'rot_3']
PLANES = ['positions', 'alphas', 'colours', 'scales', 'rotations', 'harmonics']
SH_C0 = 0.28209479177387814
DEGREE = {0: 0, 3: 1, 8: 2, 15: 3}


def table(cols):
    """{name: array}, the first column of a name kept"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    out = {}
    for k, a in items:
        out.setdefault(k, np.asarray(a))
    return out


def num(a):
    """a column's elements as JS numbers: exact for every one of the eight types"""
    return np.asarray(a).astype(np.float64)


def f32_bits(d):
    """Math.fround's bits: round to nearest even; a NaN keeps its sign and the top of its payload
    with the quiet bit set"""
    d = np.ascontiguousarray(d, np.float64)
    nan = np.isnan(d)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        out = np.where(nan, 0.0, d).astype(np.float32).view(np.uint32).copy()
    w = d.view(np.uint64)
    narrow = (((w >> np.uint64(63)) << np.uint64(31)).astype(np.uint32) | np.uint32(0x7fc00000) |
              ((w >> np.uint64(29)).astype(np.uint32) & np.uint32(0x003fffff)))
    out[nan] = narrow[nan]
    return out


def q8(t):
    """0 if t is NaN, else min(255, max(0, floor(t + 0.5)))"""
    t = np.asarray(t, np.float64)
    with np.errstate(all='ignore'):
        r = np.minimum(255.0, np.maximum(0.0, np.floor(t + 0.5)))
    return np.where(np.isnan(t), 0.0, r).astype(np.uint8)


def sigmoid(v):
    with np.errstate(all='ignore'):
        return 1.0 / (1.0 + ot.exp(-v))


def unit_quat(t):
    """u: r / L where L = sqrt(((r0 r0 + r1 r1) + r2 r2) + r3 r3) is finite and > 0, else (1, 0, 0, 0)"""
    r = [num(t[f'rot_{k}']) for k in range(4)]
    with np.errstate(all='ignore'):
        L = np.sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
        ok = (L > 0) & (L < np.inf)
        return [np.where(ok, r[k] / np.where(ok, L, 1.0), 1.0 if k == 0 else 0.0) for k in range(4)]


def _need(t):
    for k in REQUIRED:
        if k not in t:
            raise KeyError(k)


def splat_rows(cols):
    t = table(cols)
    _need(t)
    n = len(t['x'])
    w = np.zeros((n, 8), np.uint32)
    for k, name in enumerate('xyz'):
        a = t[name]
        w[:, k] = np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else f32_bits(num(a))
    with np.errstate(all='ignore'):
        for k in range(3):
            w[:, 3 + k] = f32_bits(ot.exp(num(t[f'scale_{k}'])))
        out = np.zeros((n, 32), np.uint8)
        out[:, :24] = w[:, :6].astype('<u4').view(np.uint8).reshape(n, 24)
        for k in range(3):
            out[:, 24 + k] = q8((num(t[f'f_dc_{k}']) * SH_C0 + 0.5) * 255.0)
        out[:, 27] = q8(sigmoid(num(t['opacity'])) * 255.0)
        u = unit_quat(t)
        for k in range(4):
            out[:, 28 + k] = q8((u[k] + 1.0) * 127.5)
    return out


def spz_planes(cols, fractional_bits=12):
    t = table(cols)
    _need(t)
    assert 0 <= fractional_bits <= 23
    n = len(t['x'])
    C = ot.band_coeffs(set(t))
    planes = {}
    clamped = 0
    with np.errstate(all='ignore'):
        pos = np.zeros((n, 9), np.uint8)
        for a, name in enumerate('xyz'):
            v = num(t[name])
            f = np.floor(v * float(1 << fractional_bits) + 0.5)
            nan = np.isnan(v)
            clamped += int((nan | (f < -8388608.0) | (f > 8388607.0)).sum())
            k = np.where(nan, 0.0, np.minimum(8388607.0, np.maximum(-8388608.0, f))).astype(np.int64) & 0xffffff
            for b in range(3):
                pos[:, 3 * a + b] = (k >> (8 * b)) & 0xff
        planes['positions'] = pos
        planes['alphas'] = q8(sigmoid(num(t['opacity'])) * 255.0).reshape(n, 1)
        planes['colours'] = np.stack([q8((num(t[f'f_dc_{k}']) * 0.15 + 0.5) * 255.0) for k in range(3)], 1).reshape(n, 3)
        planes['scales'] = np.stack([q8((num(t[f'scale_{k}']) + 10.0) * 16.0) for k in range(3)], 1).reshape(n, 3)
        u = unit_quat(t)
        flip = u[0] < 0
        u = [np.where(flip, -c, c) for c in u]
        planes['rotations'] = np.stack([q8((u[k] + 1.0) * 127.5) for k in (1, 2, 3)], 1).reshape(n, 3)
        sh = np.zeros((n, 3 * C), np.uint8)
        for i in range(3 * C):
            sh[:, i] = q8(num(t[f'f_rest_{(i % 3) * C + i // 3}']) * 128.0 + 128.0)
        planes['harmonics'] = sh
    return planes, clamped


def spz_header(n, C, fractional_bits):
    return b'NGSP' + struct.pack('<IIBBBB', 2, n, DEGREE[C], fractional_bits, 0, 0)


def spz_image(cols, fractional_bits=12):
    planes, clamped = spz_planes(cols, fractional_bits)
    n = len(planes['positions'])
    C = planes['harmonics'].shape[1] // 3
    image = spz_header(n, C, fractional_bits) + b''.join(planes[p].tobytes() for p in PLANES)
    assert len(image) == 16 + n * (19 + 3 * C)
    return image, clamped
