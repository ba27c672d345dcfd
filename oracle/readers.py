"""CPU restatement of the .splat / .ksplat / .spz readers -- TEST INFRASTRUCTURE ONLY.

Checker for the product's device readers (st_readers.hip).  Only tests/ import this module.
Pinned by tests/golden/readers.* and readers_edges.* (the reference's own readers run on seeded
files): tests/test_readers_oracle_cpu.py.

  read_splat    readers/read-splat.ts:14-148
  read_ksplat   readers/read-ksplat.ts:29-60 (decodeFloat16), :103-384
  read_spz      readers/read-spz.ts:36-45 (getFixed24), :62-241, over the inflated stream

Each takes the file's bytes and returns (columns, n, nsh): a float32 array [column, row] in the
reader's column order (x y z scale_0..2 f_dc_0..2 opacity rot_0..3 f_rest_0..), the row count and
the number of f_rest columns.

The file is read where it lies, one field of every row at a time: whole-array numpy arithmetic in
f64 (IEEE, one rounding per operator, as a JS number) and one conversion to f32 per stored value.
The .ksplat bucket of a splat comes from the reader's own walk, one splat after the other.
Math.log is oracle.py's st_o_log.  Wherever a NaN can come out, its bits are written here and not
left to this machine's FPU (V8 on x86-64 is what the fixtures record):
  * a float32 read as a number and stored again keeps its sign and payload and gets the quiet bit
  * an operator with a NaN operand returns that operand quieted, the first one when both are
  * an invalid operation (0 * Inf, Inf - Inf, Math.sqrt of a negative) gives the default NaN, whose
    sign bit is set: 0xfff8000000000000, stored as 0xffc00000
  * a JS NaN literal and `undefined` as a number are 0x7ff8000000000000, stored as 0x7fc00000
  * Math.log of an argument with the sign bit set (other than -0) returns V8's signalling-NaN
    constant 0x7ff4000000000000, which the store quiets to 0x7fe00000
"""
import ctypes

import numpy as np

import oracle

U32, U64, F32, F64 = np.uint32, np.uint64, np.float32, np.float64

SH_COUNT = (0, 9, 24, 45)
SH_C0 = 0.28209479177387814
JS_NAN = 0x7ff8000000000000       # NaN, undefined as a number
DEFAULT_NAN = 0xfff8000000000000  # what an invalid operation returns
QUIET64 = 0x0008000000000000


class ReaderError(ValueError):
    pass


# ---- numbers ---------------------------------------------------------------------------------
def _bits64(a):
    return np.ascontiguousarray(a, F64).view(U64)


def _from_bits64(bits, n=None):
    """an f64 array from uint64 bits (a scalar is repeated n times)"""
    if n is not None:
        return np.full(n, bits, U64).view(F64)
    return np.ascontiguousarray(bits, U64).view(F64)


def _isnan64(a):
    return (_bits64(a) & U64(0x7fffffffffffffff)) > U64(0x7ff0000000000000)


def _isnan32(b):
    return ((b & U32(0x7f800000)) == U32(0x7f800000)) & ((b & U32(0x007fffff)) != 0)


def _quiet32(b):
    """the bits of a float32 after float32 -> number -> float32"""
    return np.where(_isnan32(b), b | U32(0x00400000), b)


def _f64_of_f32_bits(b):
    """a float32 (given as bits) read as a number"""
    b = np.ascontiguousarray(b, U32)
    nan = _isnan32(b)
    out = np.where(nan, U32(0), b).view(F32).astype(F64)
    wide = ((b >> U32(31)).astype(U64) << U64(63)) | U64(JS_NAN) | ((b & U32(0x007fffff)).astype(U64) << U64(29))
    out.view(U64)[nan] = wide[nan]
    return out


def _f32_bits(d):
    """the bits a number leaves in a Float32Array"""
    d = np.ascontiguousarray(d, F64)
    nan = _isnan64(d)
    with np.errstate(over='ignore', under='ignore'):
        out = np.where(nan, 0.0, d).astype(F32).view(U32).copy()
    w = d.view(U64)
    narrow = ((w >> U64(63)) << U64(31)).astype(U32) | U32(0x7fc00000) | ((w >> U64(29)).astype(U32) & U32(0x003fffff))
    out[nan] = narrow[nan]
    return out


def _binary(op, a, b):
    """a op b for + - * /: NaN operands propagate (the first one first), a new NaN is the default one"""
    a, b = np.broadcast_arrays(np.asarray(a, F64), np.asarray(b, F64))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    an, bn = _isnan64(a), _isnan64(b)
    with np.errstate(all='ignore'):
        r = np.ascontiguousarray(op(np.where(an, 0.0, a), np.where(bn, 0.0, b)), F64)
    rb = r.view(U64)
    rb[_isnan64(r)] = U64(DEFAULT_NAN)
    rb[bn] = b.view(U64)[bn] | U64(QUIET64)
    rb[an] = a.view(U64)[an] | U64(QUIET64)
    return r


def _add(a, b):
    return _binary(np.add, a, b)


def _sub(a, b):
    return _binary(np.subtract, a, b)


def _mul(a, b):
    return _binary(np.multiply, a, b)


def _div(a, b):
    return _binary(np.divide, a, b)


def _sqrt(a):
    """Math.sqrt: the default NaN below zero, a NaN argument quieted"""
    a = np.ascontiguousarray(a, F64)
    nan = _isnan64(a)
    neg = ~nan & (a < 0)
    r = np.sqrt(np.where(nan | neg, 0.0, a))
    rb = r.view(U64)
    rb[neg] = U64(DEFAULT_NAN)
    rb[nan] = a.view(U64)[nan] | U64(QUIET64)
    return r


def _log(x):
    """Math.log (V8's ieee754::log) of an f64 array"""
    x = np.ascontiguousarray(x, F64)
    w = x.view(U64)
    nan = _isnan64(x)
    negative = ((w >> U64(63)) != 0) & (w != U64(0x8000000000000000))  # a negative NaN included
    plain = ~nan & ~negative
    arg = np.ascontiguousarray(np.where(plain, x, 1.0))
    out = np.empty(len(x), F64)
    oracle.lib().st_o_log_n(ctypes.c_uint64(len(x)), arg.ctypes.data_as(ctypes.c_void_p),
                            out.ctypes.data_as(ctypes.c_void_p))
    ob = out.view(U64)
    ob[nan] = w[nan] | U64(QUIET64)            # x + x
    ob[negative] = U64(0x7ff4000000000000)     # std::numeric_limits<double>::signaling_NaN()
    return out


def _colour(b, c0):
    """(b / 255 - 0.5) / c0 of a byte column"""
    return _f32_bits((b.astype(F64) / 255.0 - 0.5) / c0)


def _opacity(b):
    """the inverse sigmoid of an opacity byte (the same lines in all three readers)"""
    epsilon = 1e-6
    p = np.maximum(epsilon, np.minimum(1.0 - epsilon, b.astype(F64) / 255.0))
    return _f32_bits(_log(p / (1.0 - p)))


def _u16(rec, o):
    return rec[:, o].astype(U32) | (rec[:, o + 1].astype(U32) << U32(8))


def _u32(rec, o):
    return _u16(rec, o) | (_u16(rec, o + 2) << U32(16))


def _le(data, o, size):
    return int.from_bytes(data[o:o + size], 'little')


# ---- .splat ------------------------------------------------------------------------------------
def read_splat(data):
    data = bytes(data)
    if len(data) % 32:
        raise ReaderError('Invalid .splat file: file size is not a multiple of 32 bytes')
    n = len(data) // 32
    if n == 0:
        raise ReaderError('Invalid .splat file: file is empty')
    rec = np.frombuffer(data, np.uint8).reshape(n, 32)
    out = np.zeros((14, n), U32)
    for k in range(3):
        out[k] = _quiet32(_u32(rec, 4 * k))
        out[3 + k] = _f32_bits(_log(_f64_of_f32_bits(_u32(rec, 12 + 4 * k))))
        out[6 + k] = _colour(rec[:, 24 + k], SH_C0)
    out[9] = _opacity(rec[:, 27])
    q = [(rec[:, 28 + k].astype(F64) / 255.0) * 2.0 - 1.0 for k in range(4)]
    length = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    for k in range(4):
        # (the bytes have no zero-length quaternion: 127 gives -1/255, 128 gives +1/255)
        identity = 1.0 if k == 3 else 0.0
        with np.errstate(all='ignore'):
            out[10 + k] = _f32_bits(np.where(length > 0, q[k] / np.where(length > 0, length, 1.0), identity))
    return out.view(F32), n, 0


# ---- .ksplat -----------------------------------------------------------------------------------
KS_MODES = (  # centre, scale, rotation, colour, harmonics start bytes; bytes per harmonic; scaleQuantRange
    dict(scale=12, rot=24, colour=40, sh=44, sh_bytes=4, base=44, quant=1),
    dict(scale=6, rot=12, colour=20, sh=24, sh_bytes=2, base=24, quant=32767),
    dict(scale=6, rot=12, colour=20, sh=24, sh_bytes=1, base=24, quant=32767))


def _half_bits(h):
    """decodeFloat16 as the float32 bits the store leaves"""
    h = h.astype(U32)
    s, e, m = (h >> U32(15)) & U32(1), (h >> U32(10)) & U32(0x1f), h & U32(0x3ff)
    sub = (e == 0) & (m != 0)
    ex = np.full(len(h), -14, np.int64)
    mm = m.copy()
    for _ in range(10):  # while (!(m & 0x400)) { m <<= 1; exp--; }
        step = sub & ((mm & U32(0x400)) == 0)
        mm = np.where(step, mm << U32(1), mm)
        ex = np.where(step, ex - 1, ex)
    out = (s << U32(31)) | ((e + U32(112)) << U32(23)) | (m << U32(13))
    out = np.where(sub, (s << U32(31)) | ((ex + 127).astype(U32) << U32(23)) | ((mm & U32(0x3ff)) << U32(13)), out)
    out = np.where((e == 0) & (m == 0), s << U32(31), out)
    out = np.where(e == 0x1f, np.where(m == 0, (s << U32(31)) | U32(0x7f800000), U32(0x7fc00000)), out)
    return out.astype(U32)


def _ks_scale(v):
    """v > 0 ? Math.log(v) : -10 (a NaN is not > 0)"""
    positive = ~_isnan64(v) & (v > 0)
    logs = _f32_bits(_log(np.where(positive, v, 1.0)))
    return np.where(positive, logs, np.array([-10.0], F32).view(U32)[0])


def read_ksplat(data):
    data = bytes(data)
    total = len(data)
    if total < 4096:
        raise ReaderError('File too small to be valid .ksplat format')
    if data[0] != 0 or data[1] < 1:
        raise ReaderError(f'Unsupported version {data[0]}.{data[1]}')
    max_sections, num_splats, mode = _le(data, 4, 4), _le(data, 16, 4), _le(data, 20, 2)
    if mode > 2:
        raise ReaderError(f'Invalid compression mode: {mode}')

    def or_default(o, default):  # getFloat32(o) || default: 0, -0 and NaN are falsy
        v = _f64_of_f32_bits(np.array([_le(data, o, 4)], U32))
        return default if (_isnan64(v)[0] or v[0] == 0) else float(v[0])
    min_h, max_h = or_default(36, -1.5), or_default(40, 1.5)
    range_h = _sub(max_h, min_h)  # Inf - Inf: the default NaN
    if num_splats == 0:
        raise ReaderError('Invalid .ksplat file: file is empty')
    if 4096 + 1024 * max_sections > total:
        raise ReaderError('a section header lies outside the file')

    max_degree = 0
    for si in range(max_sections):
        h = 4096 + 1024 * si
        if _le(data, h, 4):
            max_degree = max(max_degree, _le(data, h + 40, 2))
    nsh_max = SH_COUNT[max_degree]
    out = np.zeros((14 + nsh_max, num_splats), U32)  # new Float32Array: +0
    M = KS_MODES[mode]
    whole = np.frombuffer(data, np.uint8)

    cur = 4096 + 1024 * max_sections
    row = 0
    for si in range(max_sections):
        h = 4096 + 1024 * si
        count, max_splats, capacity, bucket_count = (_le(data, h + 4 * k, 4) for k in range(4))
        block = _f64_of_f32_bits(np.array([_le(data, h + 16, 4)], U32))
        storage = _le(data, h + 20, 2)
        quant = float(_le(data, h + 24, 4) or M['quant'])
        full, npartial, degree = _le(data, h + 32, 4), _le(data, h + 36, 4), _le(data, h + 40, 2)
        full_splats = full * capacity
        bucket_storage = storage * bucket_count + npartial * 4
        nsh = SH_COUNT[degree]
        stride = M['base'] + nsh * M['sh_bytes']
        data_size = stride * max_splats
        pos_scale = _div(_div(block, 2.0), quant)
        centres_off = cur + npartial * 4
        data_off = cur + bucket_storage
        if (centres_off % 4 or centres_off + 12 * bucket_count > total or cur + 4 * npartial > total
                or data_off + data_size > total or count > max_splats):
            raise ReaderError('a view of the section lies outside the file')
        if row + count > num_splats:
            raise ReaderError('more splats in the sections than the header declares')
        centres = np.frombuffer(data, '<u4', bucket_count * 3, centres_off).astype(U32)
        sizes = np.frombuffer(data, '<u4', npartial, cur)

        if count:
            # which bucket each splat belongs to: read-ksplat.ts:251-269, one step per splat at most
            bucket = np.zeros(count, np.int64)
            current, base = full, full_splats
            for s in range(count):
                if s < full_splats:
                    bucket[s] = s // capacity
                else:
                    j = current - full
                    if j < npartial and s >= base + int(sizes[j]):  # (undefined past the last size: never true)
                        current += 1
                        base += int(sizes[j])
                    bucket[s] = current

            rec = whole[data_off:data_off + count * stride].reshape(count, stride)
            rows = slice(row, row + count)
            if mode == 0:
                for k in range(3):
                    out[k, rows] = _quiet32(_u32(rec, 4 * k))
                    out[3 + k, rows] = _ks_scale(_f64_of_f32_bits(_u32(rec, M['scale'] + 4 * k)))
                for k in range(4):
                    out[10 + k, rows] = _quiet32(_u32(rec, M['rot'] + 4 * k))
            else:
                have = bucket < bucket_count  # past the array the centre is undefined
                for k in range(3):
                    centre = _from_bits64(U64(JS_NAN), count).copy()
                    centre[have] = _f64_of_f32_bits(centres[bucket[have] * 3 + k])
                    t = _mul(_sub(_u16(rec, 2 * k).astype(F64), quant), pos_scale)
                    out[k, rows] = _f32_bits(_add(t, centre))
                    out[3 + k, rows] = _ks_scale(_f64_of_f32_bits(_half_bits(_u16(rec, M['scale'] + 2 * k))))
                for k in range(4):
                    out[10 + k, rows] = _half_bits(_u16(rec, M['rot'] + 2 * k))
            for k in range(3):
                out[6 + k, rows] = _colour(rec[:, M['colour'] + k], SH_C0)
            out[9, rows] = _opacity(rec[:, M['colour'] + 3])
            for i in range(nsh):
                if i < 9:
                    channel, coeff = i // 3, i % 3
                elif i < 24:
                    channel, coeff = (i - 9) // 5, (i - 9) % 5 + 3
                else:
                    channel, coeff = (i - 24) // 7, (i - 24) % 7 + 8
                col = channel * (nsh // 3) + coeff
                if mode == 0:
                    v = _quiet32(_u32(rec, M['sh'] + 4 * i))
                elif mode == 1:
                    v = _half_bits(_u16(rec, M['sh'] + 2 * i))
                else:
                    normalized = rec[:, M['sh'] + i].astype(F64) / 255
                    v = _f32_bits(_add(min_h, _mul(normalized, range_h)))
                out[14 + col, rows] = v
        row += count
        cur += data_size + bucket_storage
    if row != num_splats:
        raise ReaderError(f'Splat count mismatch: expected {num_splats}, processed {row}')
    return out.view(F32), num_splats, nsh_max


# ---- .spz --------------------------------------------------------------------------------------
def read_spz(data):
    """data: the inflated stream"""
    data = bytes(data)
    total = len(data)
    if total < 4 or _le(data, 0, 4) != 0x5053474e:
        raise ReaderError('invalid file header')
    if total < 16:
        raise ReaderError('File too small to be valid .spz format')
    version = _le(data, 4, 4)
    if version not in (2, 3):
        raise ReaderError(f'Unsupported version {version}')
    n, degree, fractional = _le(data, 8, 4), data[12], data[13]
    nsh = SH_COUNT[degree] if degree <= 3 else 0  # no entry in the table: no f_rest column
    if 16 + n * (19 + nsh) > total or (version == 3 and n == 1):
        raise ReaderError('a plane lies outside the file')
    whole = np.frombuffer(data, np.uint8)

    def plane(off, width):
        return whole[off:off + n * width].reshape(n, width), off + n * width
    pos, off = plane(16, 9)
    alpha, off = plane(off, 1)
    colour, off = plane(off, 3)
    scales, off = plane(off, 3)
    rot_off = off
    rot, off = plane(off, 3)
    sh, off = plane(off, nsh)

    shift = 1 << (fractional & 31)  # an int32 shift: 1 << 31 is negative
    scale = 1.0 / (shift - (1 << 32) if shift >= 1 << 31 else shift)
    out = np.zeros((14 + nsh, n), U32)
    for k in range(3):
        fixed = (pos[:, 3 * k].astype(np.int64) | (pos[:, 3 * k + 1].astype(np.int64) << 8)
                 | (pos[:, 3 * k + 2].astype(np.int64) << 16))
        fixed = np.where(fixed & 0x800000, fixed - (1 << 24), fixed)
        out[k] = _f32_bits(fixed.astype(F64) * scale)
        out[3 + k] = _f32_bits(scales[:, k].astype(F64) / 16.0 - 10.0)
        out[6 + k] = _colour(colour[:, k], 0.15)
    out[9] = _opacity(alpha[:, 0])

    r = [np.zeros(n, F64) for _ in range(4)]
    if version == 2:
        for k in range(3):
            r[1 + k] = rot[:, k].astype(F64)
    elif n:
        # getUint32(splatIndex): the big-endian word at byte splatIndex of the plane, then int32 operators
        at = rot_off + np.arange(n)
        word = ((whole[at].astype(np.int64) << 24) | (whole[at + 1].astype(np.int64) << 16)
                | (whole[at + 2].astype(np.int64) << 8) | whole[at + 3].astype(np.int64))
        packed = np.where(word >= 1 << 31, word - (1 << 32), word)
        largest = packed >> 30  # -2 .. 1
        sum_squares = np.zeros(n, F64)
        for i in (3, 2, 1, 0):
            take = largest != i
            mag, negbit = packed & 511, (packed >> 9) & 1
            packed = np.where(take, packed >> 10, packed)
            v = 0.7071067811865476 * mag.astype(F64) / 511
            v = np.where(negbit == 1, -v, v)
            r[i] = np.where(take, v, r[i])
            sum_squares = np.where(take, sum_squares + v * v, sum_squares)
        root = _sqrt(1.0 - sum_squares)
        for i in (0, 1):  # (a negative index sets a property of the array that nothing reads)
            r[i] = np.where(largest == i, root, r[i])
    norm = [_sub(_div(r[k], 127.5), 1.0) for k in range(4)]
    if version == 2:
        dot = norm[1] * norm[1] + norm[2] * norm[2] + norm[3] * norm[3]
        s = 1.0 - dot
        norm[0] = np.sqrt(np.where(s > 0.0, s, 0.0))
    for k in range(4):
        out[10 + k] = _f32_bits(norm[k])
    per = nsh // 3
    for i in range(nsh):
        out[14 + (i % 3) * per + i // 3] = _f32_bits((sh[:, i].astype(F64) - 128) / 128)
    return out.view(F32), n, nsh
