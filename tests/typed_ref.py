"""The float64 reference of the typed-column paths: a plain numpy restatement of what the
reference computes when a column is not a Float32Array.

Two references cover the typed kernels ("Typed columns: the two references"):
(a) a float64 or integer column whose values are all float32 values gives the reference the same
JS numbers as the Float32Array would, so the C oracle on `.astype(np.float32)` copies is exact for
the operations that do not store back into the column; (b) this module, pinned to the reference by
tests/golden/typed_edges (tests/test_typed_ref_cpu.py), for everything else:

  transform(cols, params)           transform.ts:12-65 (oracle/oracle_typed.py, shared with oracle.process)
  morton_order(x, y, z, indices)    ordering.ts:4-110 on the columns' numbers
  sog_member_textures(cols, order)  write-sog.ts:161-239,260-265: means_l / means_u / quats, the
                                    alpha byte of sh0, means_min / means_max from the numbers
"""
import numpy as np

from oracle_typed import (POS, ROT, SCL, band_coeffs, clamp_store, exp, load, log, results, same_table, store,  # noqa: F401
                          to_int32, transform)


def _part1by2(a):
    a = a & np.uint32(0x3ff)
    a = (a ^ (a << np.uint32(16))) & np.uint32(0xff0000ff)
    a = (a ^ (a << np.uint32(8))) & np.uint32(0x0300f00f)
    a = (a ^ (a << np.uint32(4))) & np.uint32(0x030c30c3)
    return (a ^ (a << np.uint32(2))) & np.uint32(0x09249249)


def morton_keys(vals):
    """ordering.ts:24-79 for one `generate` call over three float64 arrays: the 30-bit keys, or
    None where the call returns before sorting (non-finite or all-zero extents).  The extents
    start at the first element and `<` / `>` ignore a NaN met later."""
    q = []
    lens = []
    with np.errstate(all='ignore'):
        for v in vals:
            if np.isnan(v[0]):
                return None  # mx = Mx = NaN: every comparison fails, the length is NaN
            mn, mx = np.nanmin(v), np.nanmax(v)
            lens.append((mn, mx - mn))
        if not all(np.isfinite(ln) for _, ln in lens) or all(ln == 0 for _, ln in lens):
            return None
        for v, (mn, ln) in zip(vals, lens):
            mul = 0.0 if ln == 0 else 1024 / ln
            t = (v - mn) * mul
            t = np.where(np.isnan(t), 0.0, np.minimum(1023.0, t))  # Math.min(1023, NaN) >>> 0 = 0
            q.append(np.trunc(t).astype(np.uint32))
    return (_part1by2(q[2]) << np.uint32(2)) + (_part1by2(q[1]) << np.uint32(1)) + _part1by2(q[0])


def morton_order(x, y, z, indices=None):
    """generateOrdering (ordering.ts:4-110) of columns of any type, in float64: a stable sort by
    key, then every run of more than 256 equal keys again with its own extents"""
    cols = [np.asarray(a).astype(np.float64) for a in (x, y, z)]
    idx = (np.arange(len(cols[0]), dtype=np.uint32) if indices is None
           else np.array(indices, dtype=np.uint32, copy=True))
    stack = [(0, len(idx))]
    while stack:
        lo, hi = stack.pop()
        if hi - lo == 0:
            continue
        seg = idx[lo:hi]
        key = morton_keys([c[seg] for c in cols])
        if key is None:
            continue
        order = np.argsort(key, kind='stable')
        idx[lo:hi] = seg[order]
        ks = key[order]
        starts = np.concatenate(([0], np.nonzero(ks[1:] != ks[:-1])[0] + 1, [len(ks)]))
        for a, b in zip(starts[:-1], starts[1:]):
            if b - a > 256:
                stack.append((lo + int(a), lo + int(b)))
    return idx


def _js_sign(v):
    return np.where(v > 0, 1.0, np.where(v < 0, -1.0, v))  # +-0 and NaN stay


def log_transform(v):
    """write-sog.ts:33-35"""
    with np.errstate(all='ignore'):
        return _js_sign(v) * log(np.abs(v) + 1)


def _to_uint8(v):
    return (to_int32(v) & np.uint32(0xff)).astype(np.uint8)


def sog_member_textures(cols, order):
    """writeSog's textures that come straight from the members (write-sog.ts:161-239, 260-265),
    texel i from row order[i]: (dict of flat RGBA arrays means_l, means_u, quats, sh0_alpha,
    means_min[3], means_max[3]).  The arrays hold len(order) texels; the rest of the texture is 0."""
    order = np.asarray(order, np.uint32)
    n = len(order)
    tex = {k: np.zeros(n * 4, np.uint8) for k in ('means_l', 'means_u', 'quats')}
    mins, maxs = [], []
    with np.errstate(all='ignore'):
        for a, k in enumerate('xyz'):
            v = load(cols[k])[order]
            lo, hi = np.inf, -np.inf  # calcMinMax: `<` / `>` from +-Infinity, NaN ignored
            if np.any(~np.isnan(v)):
                lo, hi = np.nanmin(v), np.nanmax(v)
            lo, hi = float(log_transform(np.array([lo]))[0]), float(log_transform(np.array([hi]))[0])
            mins.append(lo)
            maxs.append(hi)
            t = to_int32(65535 * (log_transform(v) - lo) / (hi - lo))
            tex['means_l'][a::4] = (t & np.uint32(0xff)).astype(np.uint8)
            tex['means_u'][a::4] = ((t.view(np.int32) >> 8) & 0xff).astype(np.uint8)
        tex['means_l'][3::4] = 0xff
        tex['means_u'][3::4] = 0xff
        q = [load(cols[f'rot_{j}'])[order] for j in range(4)]
        ln = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
        q = [c / ln for c in q]
        maxc = np.zeros(n, np.int64)
        for j in range(1, 4):
            cur = np.choose(maxc, q)
            maxc = np.where(np.abs(q[j]) > np.abs(cur), j, maxc)
        neg = np.choose(maxc, q) < 0
        q = [np.where(neg, c * -1, c) for c in q]
        sqrt2 = np.sqrt(2.0)
        q = [c * sqrt2 for c in q]
        pick = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
        for k in range(3):
            tex['quats'][k::4] = _to_uint8(255 * (np.choose(pick[maxc, k], q) * 0.5 + 0.5))
        tex['quats'][3::4] = (252 + maxc).astype(np.uint8)
        op = load(cols['opacity'])[order]
        sig = 1 / (1 + exp(-op))
        a = sig * 255
        # Math.max(0, Math.min(255, a)): NaN propagates, then the Uint8Array store
        a = np.where(np.isnan(a), np.nan, np.maximum(0.0, np.minimum(255.0, a)))
        tex['sh0_alpha'] = _to_uint8(a)
    return tex, np.array(mins), np.array(maxs)
