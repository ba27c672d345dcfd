"""Inputs and helpers shared by tests/test_deflate_cpu.py and tests/test_deflate_gpu.py: the byte
strings on which a run-and-prefix-code DEFLATE encoder can go wrong (include/st_abi.h, "the gzip
member around a .spz image"), the two 200,000-row .spz images of the size gate, the stand-alone
program of st_deflate.h's serial encoder (tests/native/deflate_cpu_check.cpp) and a restatement of
the token rule."""
import atexit
import gzip
import os
import shutil
import subprocess
import tempfile

import numpy as np

import splat_hip as sh
import write_splat_spz_ref as ref
from golden_io import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = sh.DEFLATE_SEG
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCES = [os.path.join(ROOT, 'tests', 'native', 'deflate_cpu_check.cpp'),
           os.path.join(ROOT, 'splat-transform_amd', 'csrc', 'st_vp8l.cpp')]
RUN_LENGTHS = [2, 3, 4, 258, 259, 260, 261, 262, 517, 518]
BYTE_COUNTS = sorted({0, 1, 2, 3, 257, 258, 259, 65_535, 65_536, 65_537, SEG - 1, SEG, SEG + 1, 2 * SEG + 1})
FIBONACCI = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
SPZ_FIXTURES = ['spz_v2_d0_n300', 'spz_v2_d3_n300', 'spz_v2_d2_n257']
# the smallest match length of each length symbol 257..285 (RFC 1951 3.2.5)
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
               227, 258]
# runs whose one match makes length symbol 284 / 283 the highest used: a literal/length code of 285
# and 284 lengths (HLIT 28 and 27), the distance lengths right behind them
HIGHEST_284 = [228, 231, 251, 257, 258]
HIGHEST_283 = [196, 200, 227]


def length_symbol(length):
    return 257 + max(i for i, b in enumerate(LENGTH_BASE) if b <= length)


def ramp(n, start=0, values=251):
    """n bytes of which no two neighbours are equal, over `values` byte values"""
    return ((np.arange(n, dtype=np.int64) * 7 + start) % values).astype(np.uint8)


def plane_like(rng, n):
    """bytes like a .spz plane: a bell around 128 with stretches of one value (lengths 1..700)"""
    a = np.clip(rng.normal(128, 20, n), 0, 255).astype(np.uint8)
    pos = 0
    while pos < n:
        pos += int(rng.integers(1, 3000))
        length = int(rng.integers(1, 700))
        a[pos:pos + length] = 128
        pos += length
    return a


def runless(counts):
    """a byte string in which symbol i occurs counts[i] times and no two neighbours are equal (the
    most frequent symbols fill the even places first; needs max(counts) <= ceil(n / 2))"""
    order = np.argsort(-np.asarray(counts), kind='stable')
    flat = np.concatenate([np.full(counts[i], i, np.uint8) for i in order])
    n = len(flat)
    out = np.empty(n, np.uint8)
    half = (n + 1) // 2
    out[0::2] = flat[:half]
    out[1::2] = flat[half:]
    assert (out[1:] != out[:-1]).all()
    return out


def spz_fixture(name):
    """the inflated bytes of a committed .spz fixture file (random plane bytes)"""
    for gname in ('readers', 'readers_edges'):
        g = Golden(gname)
        for c in g.meta['cases']:
            if c['name'] == name:
                return gzip.decompress(g[name + '_file'].tobytes())
    raise KeyError(name)


def cases():
    """{name: bytes}, built once"""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(1951)
    c = {}
    for n in BYTE_COUNTS:
        c[f'bytes_{n}'] = plane_like(rng, n)
    for L in RUN_LENGTHS:
        c[f'run_{L}_at_0'] = np.concatenate([np.full(L, 9, np.uint8), ramp(40, 10)])
        c[f'run_{L}_inside'] = np.concatenate([ramp(333), np.full(L, 9, np.uint8), ramp(77, 10)])
    # a run of 300 across the first segment boundary: 100 bytes before it, 200 after
    c['run_across_segments'] = np.concatenate([ramp(SEG - 100), np.full(300, 200, np.uint8), ramp(50, 3)])
    # every run length 3..259 once, between changing literals
    parts = []
    for L in range(3, 260):
        parts += [np.full(L, L & 255, np.uint8), np.array([(L + 1) & 255, (L + 3) & 255], np.uint8)]
    c['every_run_length'] = np.concatenate(parts)
    # per length symbol a segment whose one match is that symbol's smallest length, the highest used:
    # every HLIT a dynamic block can state (2,000 + 1,200 run-free bytes of 61 values around it choose the dynamic code)
    for sym in range(257, 286):
        c[f'highest_symbol_{sym}'] = np.concatenate([ramp(2000, 0, 61), np.full(LENGTH_BASE[sym - 257] + 1, 252, np.uint8),
                                                     ramp(1200, 10, 61)])
    for L in HIGHEST_284 + HIGHEST_283:
        c[f'longest_run_{L}'] = np.concatenate([ramp(2000, 0, 61), np.full(L, 252, np.uint8), ramp(1200, 10, 61)])
    # a full first segment of bell-shaped bytes (natural runs of 2 or 3 at most) with one run of 250
    g = np.clip(rng.normal(128, 20, 200_000), 0, 255).astype(np.uint8)
    g[1000:1250] = 7
    c['bell_with_run_250'] = g
    c['all_256_values'] = np.concatenate([rng.permutation(256).astype(np.uint8) for _ in range(40)])
    c['one_byte'] = np.array([77], np.uint8)
    c['fibonacci'] = runless(FIBONACCI)
    c['random_70000'] = rng.integers(0, 256, 70_000, dtype=np.uint8)
    for name in SPZ_FIXTURES:
        c[name] = np.frombuffer(spz_fixture(name), np.uint8)
    c['constant_1MiB'] = np.full(1 << 20, 5, np.uint8)
    _CASES.update({k: np.ascontiguousarray(v).tobytes() for k, v in c.items()})
    return _CASES


_CASES = {}
STORED_CASES = ['random_70000'] + SPZ_FIXTURES


def size_table(zero_rows, n=200_000):
    """[(column, float32 array)] of n SH-3 rows: the benchmark's distributions; zero_rows: every
    harmonic of half the rows exactly 0 (the zero-row-rich data of captured scenes)"""
    rng = np.random.default_rng(7)
    zero = rng.random(n) < 0.5
    cols = []
    for k in sh.reader_columns(45):
        if k in ('x', 'y', 'z'):
            a = rng.normal(0, 10, n)
        elif k.startswith('f_dc'):
            a = rng.normal(0, 1, n)
        elif k.startswith('f_rest'):
            a = rng.normal(0, 0.1, n)
            if zero_rows:
                a[zero] = 0
        elif k == 'opacity':
            a = rng.normal(0, 2, n)
        elif k.startswith('scale'):
            a = rng.uniform(-7, -2, n)
        else:
            a = rng.normal(0, 1, n)
        cols.append((k, a.astype(np.float32)))
    return cols


def size_image(zero_rows, n=200_000):
    """the raw .spz image (fractional_bits 12) of size_table, by the restatement"""
    return bytes(ref.spz_image(size_table(zero_rows, n), 12)[0])


# ---- the token rule, restated ------------------------------------------------------------------------
def tokens(data):
    """[[('L', byte) | ('M', length)] per segment] by the rules of st_abi.h"""
    out = []
    for b in range(0, len(data), SEG):
        seg, toks, s = data[b:b + SEG], [], 0
        while s < len(seg):
            e = s
            while e < len(seg) and seg[e] == seg[s]:
                e += 1
            toks.append(('L', seg[s]))
            rest = e - s - 1
            while rest >= 258:
                toks.append(('M', 258))
                rest -= 258
            toks += [('M', rest)] if rest >= 3 else [('L', seg[s])] * rest
            s = e
        out.append(toks)
    return out


# ---- the stand-alone program ---------------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_deflate_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'deflate_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', *flags, '-o', exe, *SOURCES])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def native(mode, data, tmp_path, sanitize=False):
    """(the program's output file, its stdout lines) for mode 'stream' or 'gzip'"""
    src, dst = tmp_path / 'in.bin', tmp_path / 'out.bin'
    src.write_bytes(data)
    r = subprocess.run([harness(sanitize), mode, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == 'OK', lines[0]
    return dst.read_bytes(), lines


_NATIVE = {}


def native_cached(mode, name, tmp_path):
    """the program's bytes for a named case, computed once per session"""
    if (mode, name) not in _NATIVE:
        _NATIVE[mode, name] = native(mode, cases()[name], tmp_path)[0]
    return _NATIVE[mode, name]
