"""transform() over columns of any of the eight PLY types -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of transform.ts:12-65 as the reference runs it on a table whose columns are
not all Float32Arrays: getRow reads every column as a JS number (data-table.ts:63-68), the
arithmetic is IEEE binary64 in source order (numpy's elementwise ops neither contract nor
reassociate), and setRow stores through the column's TypedArray (data-table.ts:70-76): round to
nearest even for float32, identity for float64, ToInt32 cut to the column's width for the
integers (truncate toward zero, modulo 2^32, NaN and +-Inf -> 0; Uint8Array does not clamp).  The
matrices, the quaternion and the SH rotation rows are oracle.transform_params' (the float32 Mat4 /
Mat3 the engine stores); Math.exp / Math.log are the C restatement's fdlibm.

NaN bits.  An invalid operation on operands that hold no NaN (Inf - Inf, 0 * Inf) gives V8's NaN
on x86-64, the default NaN with the sign bit set: 0xfff8000000000000, or 0xffc00000 once stored
to a Float32Array.  numpy's SSE arithmetic on x86-64 produces the same bits, and
`check_default_nan` asserts it where this module is imported.  Math.log of an argument with the
sign bit set (a negative number, -Inf, that negative NaN) is V8's constant 0x7ff4000000000000
(st_o_log), which a Float64Array keeps and a Float32Array store quiets to 0x7fe00000, as numpy's
float64 -> float32 cast does.  A NaN that came from a NaN operand carries that operand's payload
through an operand order the JIT chooses; `taint` reports those rows, which compare as NaN only
(`same_table`)."""
import ctypes

import numpy as np

import oracle

_TWO32 = 4294967296.0
POS = ('x', 'y', 'z')
ROT = ('rot_0', 'rot_1', 'rot_2', 'rot_3')
SCL = ('scale_0', 'scale_1', 'scale_2')


def check_default_nan():
    with np.errstate(invalid='ignore'):
        v = np.array([np.inf]) - np.array([np.inf])
    assert v.view(np.uint64)[0] == 0xfff8000000000000, hex(int(v.view(np.uint64)[0]))


check_default_nan()


def to_int32(v):
    """ToInt32 (ECMA-262 7.1.6) of float64 values, as uint32 bit patterns"""
    v = np.asarray(v, np.float64)
    fin = np.isfinite(v)
    t = np.trunc(np.where(fin, v, 0.0))
    m = np.fmod(t, _TWO32)  # exact
    m = np.where(m < 0, m + _TWO32, m)
    return m.astype(np.uint64).astype(np.uint32)


def store(v, dtype):
    """a TypedArray store of float64 values v into a column of dtype"""
    dtype = np.dtype(dtype)
    v = np.asarray(v, np.float64)
    if dtype == np.float64:
        return v.copy()
    if dtype == np.float32:
        with np.errstate(over='ignore', invalid='ignore'):
            return v.astype(np.float32)
    u = to_int32(v)
    if dtype.itemsize == 4:
        return u.view(dtype).copy()
    return (u & np.uint32((1 << (8 * dtype.itemsize)) - 1)).astype(np.dtype(f'u{dtype.itemsize}')).view(dtype).copy()


def clamp_store(v, dtype):
    """what a saturating store would keep (NOT the reference's rule: the discrimination tests show
    the fixture's wrap rows tell the two apart)"""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    v = np.asarray(v, np.float64)
    t = np.trunc(np.where(np.isnan(v), 0.0, v))
    return np.clip(t, info.min, info.max).astype(dtype)


def load(a):
    """a column's values as JS numbers"""
    return np.asarray(a).astype(np.float64)


def _vec(fn, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    fn(ctypes.c_uint64(x.size), x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def exp(x):
    return _vec(oracle.lib().st_o_exp_n, x)


def log(x):
    return _vec(oracle.lib().st_o_log_n, x)


def band_coeffs(names):
    """{ '9': 1, '24': 2, '-1': 3 }[index of the first missing f_rest_i] ?? 0, as coefficients"""
    first_missing = next((i for i in range(45) if f'f_rest_{i}' not in names), -1)
    return {9: 3, 24: 8, -1: 15}.get(first_missing, 0)


def results(cols, params):
    """the JS numbers transform() hands to setRow, per transformed column (float64, before the
    store), and `taint`: per column, the rows whose operands already held a NaN"""
    names = list(cols)
    out, taint = {}, {}
    m = np.asarray(params['mat4'], np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        if all(k in cols for k in POS):
            x, y, z = (load(cols[k]) for k in POS)
            t = np.isnan(x) | np.isnan(y) | np.isnan(z) | bool(np.isnan(m).any())
            for j, k in enumerate(POS):
                out[k] = x * m[j] + y * m[4 + j] + z * m[8 + j] + m[12 + j]
                taint[k] = t
        if all(k in cols for k in ROT):
            q2w, q2x, q2y, q2z = (load(cols[k]) for k in ROT)
            q1x, q1y, q1z, q1w = (float(v) for v in params['quat'])
            out['rot_1'] = q1w * q2x + q1x * q2w + q1y * q2z - q1z * q2y
            out['rot_2'] = q1w * q2y + q1y * q2w + q1z * q2x - q1x * q2z
            out['rot_3'] = q1w * q2z + q1z * q2w + q1x * q2y - q1y * q2x
            out['rot_0'] = q1w * q2w - q1x * q2x - q1y * q2y - q1z * q2z
            t = np.isnan(q2w) | np.isnan(q2x) | np.isnan(q2y) | np.isnan(q2z) | bool(np.isnan(params['quat']).any())
            for k in ROT:
                taint[k] = t
        if all(k in cols for k in SCL):
            s = float(params['s'])
            for k in SCL:
                v = load(cols[k])
                out[k] = log(exp(v) * s)
                taint[k] = np.isnan(v) | bool(np.isnan(s))
        C = band_coeffs(names)
        if C:
            blocks = [(0, 3, np.asarray(params['sh1'], np.float64).reshape(3, 3))]
            if C >= 8:
                blocks.append((3, 5, np.asarray(params['sh2'], np.float64).reshape(5, 5)))
            if C >= 15:
                blocks.append((8, 7, np.asarray(params['sh3'], np.float64).reshape(7, 7)))
            for ch in range(3):
                # shCoeffs is a Float32Array: the loads round to float32
                src = [load(cols[f'f_rest_{k + ch * C}']).astype(np.float32).astype(np.float64) for k in range(C)]
                for off, w, rows in blocks:
                    t = np.zeros(len(src[0]), bool)
                    for i in range(w):
                        t |= np.isnan(src[off + i])
                    t |= bool(np.isnan(rows).any())
                    for r in range(w):
                        acc = np.zeros(len(src[0]))  # dp (rotate-sh.ts:32-38): from +0, index order
                        for i in range(w):
                            acc = acc + src[off + i] * rows[r, i]
                        k = f'f_rest_{off + r + ch * C}'
                        out[k] = acc.astype(np.float32).astype(np.float64)  # back into shCoeffs
                        taint[k] = t
    return out, taint


def transform(cols, params):
    """transform() in place on a dict name -> array of any of the eight types; returns `taint`"""
    out, taint = results(cols, params)
    for k, v in out.items():
        cols[k][...] = store(v, cols[k].dtype)
    return taint


def same_table(got, want, taint=None, what=''):
    """bit equality of two dicts of columns; rows in `taint` (NaN from a NaN operand) may differ
    in NaN payload where both hold a NaN"""
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        bad = a.view(f'u{a.dtype.itemsize}') != b.view(f'u{a.dtype.itemsize}')
        if a.dtype.kind == 'f' and taint is not None and k in taint:
            bad &= ~(taint[k] & np.isnan(a) & np.isnan(b))
        rows = np.nonzero(bad)[0]
        assert rows.size == 0, f'{what} {k}: {rows.size} rows differ, first {rows[:4]}: {a[rows[:4]]} != {b[rows[:4]]}'
