"""numpy restatement of the .sog reader's decode rules (include/st_abi.h, "the .sog reader"): the
inverses of writeSog's quantisers (write-sog.ts:162-268, :319-348) in JS-number (float64)
arithmetic with one Float32Array store per value.  Math.exp / Math.log are V8's, through the
oracle's st_o_exp_n / st_o_log_n.  Every comparison against it is on uint32 views, bit for bit.

decode(meta, count, tex) -> {column name: float32[count]} in reader_columns(nsh) order, and the
number of shN labels outside the palette.
  meta: dict(mins, maxs: 3 float64; scales, sh0, shn: 256 float32 codebooks; bands; palette)
  tex:  dict name -> (h, w, 4) uint8 RGBA (means_l means_u quats scales sh0 shN_centroids shN_labels)
"""
import numpy as np

import oracle_typed as ot

READER_COLS = ['x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
               'rot_0', 'rot_1', 'rot_2', 'rot_3']
COEFFS = [0, 3, 8, 15]


def meta_of_struct(m):
    """the dict decode() takes from a splat_hip.SogMeta"""
    return dict(mins=np.array(m.means_min[:], np.float64), maxs=np.array(m.means_max[:], np.float64),
                scales=np.array(m.scales_codebook[:], np.float32), sh0=np.array(m.sh0_codebook[:], np.float32),
                shn=np.array(m.shn_codebook[:], np.float32), bands=int(m.sh_bands), palette=int(m.palette_size))


def meta_of_json(m):
    """the same from a parsed meta.json"""
    shn = m.get('shN', {})
    return dict(mins=np.array(m['means']['mins'], np.float64), maxs=np.array(m['means']['maxs'], np.float64),
                scales=np.array(m['scales']['codebook'], np.float64).astype(np.float32),
                sh0=np.array(m['sh0']['codebook'], np.float64).astype(np.float32),
                shn=np.array(shn.get('codebook', [0.0] * 256), np.float64).astype(np.float32),
                bands=int(shn.get('bands', 0)), palette=int(shn.get('count', 0)))


def _f32(v):
    """a Float32Array store of JS numbers (a NaN stays a NaN; which NaN is the platform's word, and
    the tests compare NaN rows as NaN only)"""
    return np.asarray(v, np.float64).astype(np.float32)


def decode(meta, count, tex):
    texel = lambda name: np.asarray(tex[name], np.uint8).reshape(-1, 4)[:count].astype(np.int64)
    out = {}
    with np.errstate(all='ignore'):
        # x y z: q = means_l | means_u << 8; v = mins + (maxs - mins) * (q / 65535); sign(v) * (exp(|v|) - 1)
        lo, hi = texel('means_l'), texel('means_u')
        for a, name in enumerate('xyz'):
            q = (lo[:, a] | (hi[:, a] << 8)).astype(np.float64)
            v = meta['mins'][a] + (meta['maxs'][a] - meta['mins'][a]) * (q / 65535.0)
            r = np.sign(v) * (ot.exp(np.abs(v)) - 1.0)
            out[name] = _f32(np.where(np.isnan(v), v, r))
        # scale_k = scales_codebook[scales.k]; f_dc_k = sh0_codebook[sh0.k]: float32 copies
        sc, s0 = texel('scales'), texel('sh0')
        for k in range(3):
            out[f'scale_{k}'] = meta['scales'][sc[:, k]].copy()
        for k in range(3):
            out[f'f_dc_{k}'] = meta['sh0'][s0[:, k]].copy()
        # opacity: p = A / 255; e = min(1 - 1e-6, max(1e-6, p)); log(e / (1 - e))
        p = s0[:, 3].astype(np.float64) / 255.0
        e = np.minimum(1.0 - 1e-6, np.maximum(1e-6, p))
        out['opacity'] = _f32(ot.log(e / (1.0 - e)))
        # rot: t = A & 3; c_k = (byte_k / 255 - 0.5) * sqrt(2); m = sqrt(max(0, 1 - (c0 c0 + c1 c1 + c2 c2)))
        qt = texel('quats')
        tag = qt[:, 3] & 3
        c = [(qt[:, k].astype(np.float64) / 255.0 - 0.5) * np.sqrt(2.0) for k in range(3)]
        m = np.sqrt(np.maximum(0.0, 1.0 - ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])))
        for j in range(4):
            # component j: m where it is the tag; else c0, c1, c2 in ascending index among the others
            k = np.where(j < tag, j, j - 1)
            others = np.choose(np.clip(k, 0, 2), c)
            out[f'rot_{j}'] = _f32(np.where(tag == j, m, others))
    out = {k: out[k] for k in READER_COLS}
    bad = 0
    C = COEFFS[meta['bands']]
    if C:
        lab = texel('shN_labels')
        label = lab[:, 0] | (lab[:, 1] << 8)
        ok = label < meta['palette']
        bad = int((~ok).sum())
        cent = np.asarray(tex['shN_centroids'], np.uint8)
        assert cent.shape[1] == 64 * C
        safe = np.where(ok, label, 0)
        for ch in range(3):
            for j in range(C):
                byte = cent[safe >> 6, (safe & 63) * C + j, ch]
                out[f'f_rest_{j + ch * C}'] = np.where(ok, meta['shn'][byte], np.float32(0.0)).astype(np.float32)
        out = {**{k: out[k] for k in READER_COLS}, **{f'f_rest_{i}': out[f'f_rest_{i}'] for i in range(3 * C)}}
    return out, bad


def bits_equal(a, b):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    b = np.ascontiguousarray(np.asarray(b, np.float32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
