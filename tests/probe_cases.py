"""Inputs, references and helpers shared by tests/test_jsmath_cpu.py, tests/test_probe_scalar_gpu.py
and tests/test_prims_gpu.py: the float64 values at which the scalar rules of
splat-transform_amd/csrc/st_jsmath.h (and the bare sqrt, division, floor(t + 0.5) and float
conversion the kernels use beside them) can go wrong, plain references for them, and the stand-alone
program that evaluates them on the host (tests/native/jsmath_cpu_check.cpp, over the expressions of
csrc/st_probe_ops.h that st_dev_probe evaluates on the device).

What is the machine's own:
  * a NaN that a bare operation MAKES from operands that are not NaN (sqrt of a negative, 0 / 0,
    Inf / Inf) is a default NaN: 0xFFF8000000000000 on x86-64, and for these two operations the same
    on gfx950 (its division and square-root sequences give the negative one; st_jsmath.h's x86_nan
    is for the operations whose default NaN there is the positive one).  The tests assert that
    value on both;
  * an operation on TWO NaN operands of different bits returns whichever the machine (and the
    compiler's operand order) picks.  No division pair here has two different NaNs.
    log_transform of a NEGATIVE NaN is sign_(v) * log(|v| + 1): v times its own positive, quieted
    twin.  x86-64 returns the first operand of the multiply instruction, and which that is the
    compiler chooses: the host program gives the positive one, the device the negative one (the
    first operand in source order).  There the device is compared with the host program without
    the sign bit, and with the quieted argument itself, sign included."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'tests', 'native', 'jsmath_cpu_check.cpp')

ONE_INPUT = ['exp', 'log', 'sigmoid', 'log_transform', 'log1abs', 'logexp', 'sqrt', 'round', 'to_int32', 'to_uint8',
             'f32_store', 'f32_cast', 'sign']
TWO_INPUT = ['div', 'min', 'max']
# the type an op's results are compared in: float64 / float32 results as their bits
OUT_DTYPE = {'to_int32': np.int32, 'to_uint8': np.uint8, 'f32_store': np.uint32, 'f32_cast': np.uint32}
X86_NAN = 0xFFF8000000000000
SIGN = 1 << 63


def out_dtype(op):
    return np.dtype(OUT_DTYPE.get(op, np.uint64))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def f64(b):
    return np.ascontiguousarray(b, np.uint64).view(np.float64)


def _b(x):
    return int(bits([x])[0])


def _around(b, r=2):
    return [b + d for d in range(-r, r + 1)]


# ---- exp's and log's constants, as csrc/st_jsmath.h has them ---------------------------------------
INVLN2 = 1.44269504088896338700e+00
O_THRESHOLD, U_THRESHOLD = 7.09782712893383973096e+02, -7.45133219101941108420e+02
EXP_HI_WORDS = [0x40862E42, 0x3fd62e42, 0x3FF0A2B2, 0x3e300000, 0x7ff00000]
LOG_MANTISSAS = [0x6147a, 0x6147b, 0x6b850, 0x6b851, 0x6b852,  # the window of the two tails
                 0x6a09b, 0x6a09c,                             # where (hx + 0x95f64) & 0x100000 switches
                 0xffffd, 0xffffe, 0xfffff, 0x00000, 0x00001, 0x00002]  # (2 + hx) & 0xfffff < 3
LOG_EXPONENTS = [0x3ff, 0x3fe, 0x400, 0x001, 0x7fe, 0x234]


def exp_k(x):
    """the k of js::exp's general branch: (int32_t)(invln2 * x + (x < 0 ? -0.5 : 0.5))"""
    return int(INVLN2 * x + (-0.5 if x < 0 else 0.5))


def exp_k_edge(kk):
    """the bits of the x of smallest magnitude, of kk's sign, at which exp_k reaches kk"""
    lo, hi = _b(0.1), _b(750.0)
    sign = -1.0 if kk < 0 else 1.0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if abs(exp_k(sign * float(f64([mid])[0]))) >= abs(kk):
            hi = mid
        else:
            lo = mid
    return hi | (SIGN if kk < 0 else 0)


def nan_patterns():
    out = []
    for sign in (0, 1):
        for quiet in (0, 1):
            for payload in (0, 1, 0x123456789abc, (1 << 51) - 1, 1 << 50, 1 << 29, (1 << 29) - 1):
                if payload or quiet:
                    out.append((sign << 63) | (0x7ff << 52) | (quiet << 51) | payload)
    return out


def wide_inputs():
    """float64 inputs of the one-input ops, about 40k, the same in every process"""
    if 'wide' in _SETS:
        return _SETS['wide']
    rng = np.random.default_rng(355)
    p = []
    # exp: the thresholds on the high word, both signs, the word and the next one
    for h in EXP_HI_WORDS:
        for sign in (0, SIGN):
            for w in (h, h + 1):
                p += _around(sign | (w << 32))
    p += _around(_b(O_THRESHOLD)) + _around(_b(U_THRESHOLD)) + _around(_b(1.0)) + _around(_b(-1.0))
    for kk in (-1075, -1074, -1023, -1022, -1021, -1020, -2, -1, 1, 2, 1022, 1023, 1024):
        p += _around(exp_k_edge(kk))
    # log: the mantissa thresholds at several exponents, low words 0, 2^31 and 2^32 - 1, and the
    # same mantissas in subnormals (leading one at bit q, the 20 bits under it = the threshold)
    for e in LOG_EXPONENTS:
        for m in LOG_MANTISSAS:
            for low in (0, 0x80000000, 0xffffffff):
                p += _around((e << 52) | (m << 32) | low)
    for q in (51, 40, 21):
        for m in LOG_MANTISSAS:
            p += _around((1 << q) | (m << (q - 20))) + [(1 << q) | (m << (q - 20)) | ((1 << (q - 20)) - 1)]
    # exact powers of two, subnormal ones included
    pw = np.ldexp(1.0, np.arange(-1074, 1024))
    p += [int(v) for v in bits(pw)] + [int(v) | SIGN for v in bits(pw)]
    # subnormals and the first normals
    p += [1, 2, 3, (1 << 52) - 1, (1 << 52) - 2] + _around(1 << 52)
    p += [int(v) for v in rng.integers(1, 1 << 52, 512)]
    p += [int(v) | SIGN for v in rng.integers(1, 1 << 52, 256)]
    # inputs whose exp is subnormal: 2^-1075 < exp(x) < 2^-1022
    p += [_b(v) for v in np.linspace(-745.2, -708.3, 256)] + [_b(v) for v in rng.uniform(-745.2, -708.3, 1024)]
    # zeros, infinities, NaNs
    p += [0, SIGN, 0x7ff << 52, SIGN | (0x7ff << 52)] + nan_patterns()
    p += exact_op_patterns(rng)
    p += [int(v) for v in rng.integers(0, 1 << 64, 1 << 14, dtype=np.uint64)]
    mag = np.ldexp(rng.uniform(1, 2, 1 << 14), rng.integers(-1074, 1024, 1 << 14))
    p += [int(v) for v in bits(mag * np.where(rng.random(1 << 14) < 0.5, -1.0, 1.0))]
    _SETS['wide'] = f64(np.array(p, dtype=np.uint64))
    return _SETS['wide']


def exact_op_patterns(rng):
    """inputs for the conversions, sqrt and floor(t + 0.5)"""
    p = []
    # float32 round-to-even ties: the float64 midway between two neighbouring float32 values, in
    # the normal and in the subnormal range, with its neighbours; both signs
    u = [0x3f800000, 0x3f800001, 0x00800000, 0x00800001, 0x007fffff, 0x007ffffe, 0x7f7ffffe, 0x7f7ffffd, 1, 2, 3,
         0x00400000, 0x3eaaaaab]
    u += [int(v) for v in rng.integers(0x00800000, 0x7f7ffffe, 64)] + [int(v) for v in rng.integers(1, 0x007ffffe, 64)]
    u = np.array(u, np.uint32)
    mid = (u.view(np.float32).astype(np.float64) + (u + 1).view(np.float32).astype(np.float64)) / 2
    for m in bits(mid):
        p += _around(int(m), 1) + _around(int(m) | SIGN, 1)
    p += _around(_b(2.0 ** -150), 1) + _around(_b(-2.0 ** -150), 1)  # the tie between 0 and the least float32
    p += _around(0x47EFFFFFF0000000, 1) + _around(0x47EFFFFFF0000000 | SIGN, 1)  # the tie that overflows
    p += [0x7ff4000000000000, X86_NAN]  # js::log's signalling NaN, the negative default NaN
    # ToInt32
    v = [2.0 ** 31, 2.0 ** 31 - 1, 2.0 ** 31 + 1, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5, 2.0 ** 32, 2.0 ** 32 - 1, 2.0 ** 32 + 1,
         2.0 ** 32 - 0.5, 2.0 ** 32 + 0.5, 2.0 ** 53, 2.0 ** 53 - 1, 2.0 ** 53 + 2, 9.2e18, float(np.nextafter(9.2e18, 0)),
         float(np.nextafter(9.2e18, np.inf)), 2.0 ** 63, 2.0 ** 63 - 1024, 2.0 ** 63 + 2048, 2.0 ** 64, 2.0 ** 64 + 4096,
         2.0 ** 64 - 2048, 2.0 ** 80 + 2.0 ** 28, 2.0 ** 84 + 2.0 ** 32, 2.0 ** 83 + 2.0 ** 31, 1e300, 0.5,
         0.9999999999999999, 1.5, 255.0, 255.5, 256.0, 257.0, 1.0, 2.0, 4.0, 5e-324, 2.2250738585072014e-308]
    p += [_b(x) for x in v] + [_b(-x) for x in v]
    big = np.ldexp(rng.integers(1 << 52, 1 << 53, 2048).astype(np.float64), rng.integers(-52, 41, 2048))
    p += [int(x) for x in bits(big * np.where(rng.random(2048) < 0.5, -1.0, 1.0))]
    # sqrt: perfect squares and their neighbours (k * k < 2^53 is exact)
    ks = [3, 5, 7, (1 << 26) + 1, (1 << 26) - 1, 94906265] + [int(k) for k in rng.integers(2, 94906265, 256)]
    for k in ks:
        p += _around(_b(float(k * k)), 1)
    # floor(t + 0.5): halves and their neighbours, the largest t below 0.5, where t + 0.5 stops being exact
    for k in range(-4, 5):
        p += _around(_b(k + 0.5), 1)
    p += _around(_b(0.49999999999999994), 1) + _around(_b(-0.49999999999999994), 1)
    for x in (2.0 ** 51 + 0.5, 2.0 ** 52, 2.0 ** 52 + 1, 2.0 ** 53, 254.5, 255.5, 65534.5):
        p += _around(_b(x), 1) + _around(_b(-x), 1)
    return p


def pair_inputs():
    """(a, b): float64 inputs of the two-input ops"""
    if 'pairs' in _SETS:
        return _SETS['pairs']
    rng = np.random.default_rng(950)
    a, b = [], []

    def add(x, y):
        a.append(int(x))
        b.append(int(y))

    basic = [_b(v) for v in (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan)]
    for x in basic:
        for y in basic:
            add(x, y)
    for nan in nan_patterns():  # one NaN operand, or the same NaN twice
        for other in (_b(1.0), _b(-0.0), _b(np.inf)):
            add(nan, other)
            add(other, nan)
        add(nan, nan)
    add(_b(np.sqrt(2.0)), _b(2.0))
    add(_b(1.0), _b(3.0))
    # subnormal operands; quotients in and around the subnormal range
    sub = rng.integers(1, 1 << 52, 1024)
    nrm = bits(np.ldexp(rng.uniform(1, 2, 1024), rng.integers(-60, 60, 1024)))
    for i in range(1024):
        s = SIGN if i & 1 else 0
        add(int(sub[i]) | s, nrm[i])
        add(nrm[i], int(sub[i]) | s)
    ea = rng.integers(-1000, 0, 2048)
    eb = ea + rng.integers(1018, 1078, 2048)  # quotient of magnitude 2^-1078 .. 2^-1017 (it must not overflow ldexp)
    qa, qb = np.ldexp(rng.uniform(1, 2, 2048), ea), np.ldexp(rng.uniform(1, 2, 2048), np.minimum(eb, 1023))
    for x, y in zip(bits(qa), bits(qb)):
        add(x, y)
    # exact ties of a subnormal quotient: an odd multiple of 2^-1074 halved, quartered
    for k in rng.integers(0, 1 << 40, 128):
        for d in (2.0, 4.0, 8.0, -2.0):
            add(2 * int(k) + 1, _b(d))
            add(2 * int(k) + 3, _b(d))
    # quotients at the overflow threshold
    big = np.ldexp(rng.uniform(1, 2, 512), rng.integers(500, 1024, 512))
    small = np.ldexp(rng.uniform(1, 2, 512), rng.integers(-1022, -500, 512))
    for x, y in zip(bits(big), bits(small)):
        add(x, y)
    ra, rb = rng.integers(0, 1 << 64, 4096, dtype=np.uint64), rng.integers(0, 1 << 64, 4096, dtype=np.uint64)
    both_nan = np.isnan(f64(ra)) & np.isnan(f64(rb))
    for x, y in zip(ra[~both_nan], rb[~both_nan]):
        add(x, y)
    la = np.ldexp(rng.uniform(1, 2, 4096), rng.integers(-1074, 1024, 4096)) * np.where(rng.random(4096) < 0.5, -1, 1)
    lb = np.ldexp(rng.uniform(1, 2, 4096), rng.integers(-1074, 1024, 4096)) * np.where(rng.random(4096) < 0.5, -1, 1)
    for x, y in zip(bits(la), bits(lb)):
        add(x, y)
    _SETS['pairs'] = (f64(np.array(a, dtype=np.uint64)), f64(np.array(b, dtype=np.uint64)))
    return _SETS['pairs']


_SETS = {}


# ---- plain references -------------------------------------------------------------------------------
def ref_to_int32(x):
    """ECMA-262 ToInt32 in Python integers: trunc(v) mod 2^32, read as a signed word"""
    out = np.zeros(len(x), np.int64)
    for i, v in enumerate(x):
        if np.isfinite(v):
            m = int(v) % (1 << 32)
            out[i] = m - (1 << 32) if m >= (1 << 31) else m
    return out.astype(np.int32)


def ref_to_uint8(x):
    return (ref_to_int32(x).astype(np.int64) & 0xff).astype(np.uint8)


def ref_f32_store(x):
    """the rule in f32_store's comment: round to nearest even; a NaN keeps its sign and the top 22
    bits of its payload, with the quiet bit set"""
    b = bits(x)
    with np.errstate(over='ignore', invalid='ignore'):
        out = np.asarray(x, np.float64).astype(np.float32).view(np.uint32).copy()
    nan = np.isnan(x)
    quiet = ((b >> np.uint64(63)) << np.uint64(31)) | np.uint64(0x7fc00000) | ((b & np.uint64((1 << 52) - 1)) >> np.uint64(29))
    out[nan] = quiet[nan].astype(np.uint32)
    return out


def ref_sign(x):
    x = np.asarray(x, np.float64)
    return bits(np.where(np.isnan(x) | (x == 0), x, np.where(x > 0, 1.0, -1.0)))


def ref_minmax(a, b, want_max):
    """Math.min / Math.max: a NaN operand gives V8's NaN, -0 < +0"""
    out = np.empty(len(a), np.uint64)
    for i, (x, y) in enumerate(zip(a, b)):
        if x != x or y != y:
            out[i] = X86_NAN
        elif x == 0 and y == 0:
            neg = bool(np.signbit(x)) or bool(np.signbit(y))
            both = bool(np.signbit(x)) and bool(np.signbit(y))
            out[i] = (SIGN if both else 0) if want_max else (SIGN if neg else 0)
        else:
            out[i] = _b(max(x, y) if want_max else min(x, y))
    return out


def ulp_errors(fn, x, got):
    """|got - fn(x)| in units of the true value's last place (2^-1074 for a subnormal one), fn an
    mpmath function evaluated at 200 bits -> (errors, true value is subnormal); got must be finite"""
    import mpmath
    err, sub = np.empty(len(x)), np.zeros(len(x), bool)
    with mpmath.workprec(200):
        for i, (v, g) in enumerate(zip(x, got)):
            t = fn(mpmath.mpf(float(v)))
            if t == 0:
                err[i] = 0.0 if g == 0 else np.inf
                continue
            _, man, exp, bc = t._mpf_
            e = max(exp + bc - 1, -1022)  # floor(log2 |t|), held at the subnormals' exponent
            sub[i] = exp + bc - 1 < -1022
            err[i] = float(abs(mpmath.mpf(float(g)) - t) / mpmath.ldexp(1, e - 52))
    return err, sub


# ---- the stand-alone program ---------------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit): with the
    library's -O3 -ffp-contract=off, or with AddressSanitizer and UndefinedBehaviorSanitizer on its host code"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_jsmath_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'jsmath_cpu_check')
        flags = ['-O3']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=off', *flags, '-o', exe,
                               SOURCE])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def host(op, a, b=None, s=0.0, sanitize=False):
    """the program's results of `op` (a name of splat_hip.PROBE_OPS) in out_dtype(op)"""
    import splat_hip as sh
    d = tempfile.mkdtemp(prefix='st_jsmath_io_')
    try:
        bits(a).tofile(os.path.join(d, 'a'))
        if b is not None:
            bits(b).tofile(os.path.join(d, 'b'))
        r = subprocess.run([harness(sanitize), str(sh.PROBE_OPS[op]), os.path.join(d, 'a'),
                            os.path.join(d, 'b') if b is not None else '-', '%016x' % _b(s), os.path.join(d, 'out')],
                           capture_output=True, text=True)
        assert r.returncode == 0, (op, r.stdout[-2000:], r.stderr[-4000:])
        out = np.fromfile(os.path.join(d, 'out'), out_dtype(op))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    assert len(out) == len(a)
    return out


_HOST = {}
LOGEXP_S = 0.75  # the scalar of 'logexp' on the wide set (the fixture has 0.5 and 2)


def host_wide(op):
    """the plain build's results on wide_inputs() / pair_inputs(), computed once per process"""
    if op not in _HOST:
        if op in TWO_INPUT:
            _HOST[op] = host(op, *pair_inputs())
        else:
            _HOST[op] = host(op, wide_inputs(), s=LOGEXP_S)
    return _HOST[op]
