"""Tables shared by tests/test_summary_cpu.py and tests/test_summary_gpu.py: the smallest inputs at
which each piece of the column summary (include/st_abi.h, "column summary") can go wrong, their
expected summaries by tests/summary_ref.py (computed once per process), and the stand-alone program
of st_summary.h's serial host form (tests/native/summary_cpu_check.cpp)."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

import summary_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'tests', 'native', 'summary_cpu_check.cpp')
DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]
PLY_CODE = {np.dtype(d): i + 1 for i, d in enumerate(DTYPES)}
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 257, 4097]
# the three ways every case runs: (id, ST_SUM_EXACT, ST_SUM_FLUSH)
MODES = [('default', None, None), ('exact', '1', None), ('flush64', None, '64')]


def random_column(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    return (rng.normal(0, 1, n) * np.exp(rng.normal(0, 3, n))).astype(dtype)


def f32_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def f64_bits(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def tables():
    """{case: [(column name, numpy array)]}; built once"""
    if _TABLES:
        return _TABLES
    rng = np.random.default_rng(20)
    t = {}
    # lengths, every type
    for n in LENGTHS:
        t[f'len_{n}'] = [(np.dtype(d).name, random_column(rng, d, n)) for d in DTYPES]
    # tables: 62 mixed columns, 300 columns (beyond one launch's batch), two columns sharing a name
    t['cols_62'] = [(f'c{i}', random_column(rng, DTYPES[i % 8], 257)) for i in range(62)]
    t['cols_300'] = [(f'c{i}', random_column(rng, DTYPES[(i * 3) % 8], 65)) for i in range(300)]
    t['same_name'] = [('x', random_column(rng, np.float32, 65)), ('x', random_column(rng, np.int16, 65))]
    # ---- sum
    p53 = float(2 ** 53)
    tiny64 = f64_bits([1])[0]  # 2^-1074
    t['sum'] = []
    s = {
        'f32_cancel': np.array([1e30, 1, -1e30], np.float32),
        'f64_tie_even': np.array([p53, 1.0]),
        'f64_tie_up': np.array([p53 + 2, 1.0]),
        'f64_sticky': np.array([p53, 1.0, tiny64]),
        'f64_subnormals': np.array([tiny64] * 3),
        'f32_full_span': f32_bits([1, 0x7f7fffff]),
        'f32_full_span_neg': f32_bits([0x80000001, 0xff7fffff, 1]),
        'f64_overflow': np.array([1.7e308, 1.7e308]),
        'f64_overflow_neg': np.array([-1.7e308, -1.7e308, 1.0]),
        'f64_excursion': np.array([1.7e308, 1.7e308, -1.7e308]),
        'f64_just_below_overflow': f64_bits([0x7fefffffffffffff, 0x7c90000000000000 - 1]),  # max + just under 2^970
        'f64_just_at_overflow': f64_bits([0x7fefffffffffffff, 0x7c90000000000000]),         # max + 2^970
        'f64_full_span': f64_bits([1, 0x7fefffffffffffff, 0x8000000000000001]),
        'i32_extremes': np.array([-2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31], np.int32),
        'f32_alternating': (np.where(np.arange(4096) % 2 == 0, 1, -1) *
                            np.ldexp(np.float64(1 + 2.0 ** -23), rng.integers(-126, 128, 4096))).astype(np.float32),
        'f64_zeros': np.array([0.0, -0.0, -0.0]),
    }
    t['sum'] = list(s.items())
    t['sum_u32_max'] = [('u32', np.full(2_097_153, 0xFFFFFFFF, np.uint32))]
    # ---- deviation
    d = {f'd124_{np.dtype(x).name}': np.array([1, 2, 4], x) for x in (np.float32, np.float64, np.uint8, np.int32)}
    d['constant_f32'] = np.full(1000, 0.1, np.float32)
    d['constant_f64'] = np.full(1001, 0.1, np.float64)
    d['constant_u16'] = np.full(77, 40000, np.uint16)
    d['t_overflow'] = np.array([1e200, -1e200, 3.0])
    d['sum_inf'] = np.array([1.7e308, 1.7e308, 5.0])
    d['sum_neg_inf'] = np.array([-1.7e308, -1.7e308])
    t['deviation'] = list(d.items())
    # ---- median
    m = {}
    for x in (np.int8, np.uint16, np.uint32, np.float32, np.float64):
        for k in (1, 2, 3, 4):
            m[f'm{k}_{np.dtype(x).name}'] = np.array([7, 3, 100, 5][:k], x)
    m['zeros_2'] = np.array([-0.0, 0.0], np.float32)
    m['zeros_2_f64'] = np.array([0.0, -0.0])
    m['zeros_3'] = np.array([0.0, -0.0, -0.0], np.float32)
    m['all_equal'] = np.full(100, -3.25, np.float32)
    m['low_byte_f32'] = f32_bits(0x3f800000 + rng.permutation(256))
    m['high_byte_f32'] = f32_bits(rng.permutation(256).astype(np.uint32) << 24)
    m['high_byte_u32'] = rng.permutation(256).astype(np.uint32) << 24
    m['high_byte_i32'] = (rng.permutation(256).astype(np.uint32) << 24).view(np.int32)
    m['high_byte_f64'] = f64_bits(rng.permutation(256).astype(np.uint64) << 56)
    m['low_byte_f64'] = f64_bits(np.uint64(0x4000000000000000) + rng.permutation(255).astype(np.uint64))
    dup = np.concatenate([np.full(4000, 0.5, np.float32), rng.normal(0.5, 1, 97).astype(np.float32)])
    m['duplicates_4097'] = rng.permutation(dup)
    mixed = np.concatenate([rng.normal(0, 1, 10), [np.inf, -np.inf, np.inf]]).astype(np.float32)
    mixed = np.concatenate([mixed, f32_bits([0x7fc00000, 0xffc00000, 0xff800001, 0x7f800001])])
    m['nan_inf_mixed_f32'] = rng.permutation(mixed)
    m['nan_inf_mixed_f64'] = np.concatenate([rng.normal(0, 1, 12), [np.inf, -np.inf],
                                             f64_bits([0xfff8000000000000, 0x7ff8000000000001, 0xfff0000000000001])])
    m['all_nan'] = f32_bits([0x7fc00000, 0xffc00000, 0x7f800001] * 30)
    m['all_nan_f64'] = np.full(5, np.nan)
    m['all_inf'] = np.array([np.inf, -np.inf], np.float32)
    m['i8_wide'] = random_column(rng, np.int8, 10001)
    m['u16_wide'] = random_column(rng, np.uint16, 10001)
    m['f64_low_word'] = f64_bits(np.uint64(0x3ff0000000000000) + rng.integers(0, 2 ** 32, 1000, dtype=np.uint64))
    t['median'] = list(m.items())
    _TABLES.update(t)
    return _TABLES


_TABLES = {}
_EXPECTED = {}


def expected(case):
    """[summary_ref.Summary] of a case's columns, computed once per process"""
    if case not in _EXPECTED:
        _EXPECTED[case] = [ref.summarize(a) for _, a in tables()[case]]
    return _EXPECTED[case]


# ---- the stand-alone program -----------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_summary_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'summary_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=off', *flags, '-o', exe,
                               SOURCE])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def run_program(args, sanitize=False):
    r = subprocess.run([harness(sanitize), *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


RECORD = np.dtype([('rows', '<u8'), ('nan_count', '<u8'), ('inf_count', '<u8'), ('min', '<f8'), ('max', '<f8'),
                   ('sum', '<f8'), ('mean', '<f8'), ('ssd', '<f8'), ('std_dev', '<f8'), ('median', '<f8')])


def native(cols, tmp_path, exact=False, flush=1 << 30, sanitize=False):
    """([summary_ref.Summary], [fast]) of [(name, array)] by the program's serial host form"""
    src, out = tmp_path / 'cols.bin', tmp_path / 'summaries.bin'
    with open(src, 'wb') as f:
        for _, a in cols:
            a = np.ascontiguousarray(a)
            f.write(np.int32(PLY_CODE[a.dtype]).tobytes() + np.uint64(len(a)).tobytes() + a.tobytes())
    lines = run_program(['summary', src, out, int(exact), flush], sanitize)
    rec = np.fromfile(out, RECORD)
    assert len(rec) == len(cols) == len(lines)
    got = [ref.Summary(*(r[f].item() for f in ref.FIELDS)) for r in rec]
    return got, [bool(int(l.split()[2])) for l in lines]


def native_text(names, summaries, tmp_path, sanitize=False):
    nf, sf, out = tmp_path / 'names.txt', tmp_path / 'records.bin', tmp_path / 'text.bin'
    nf.write_text(''.join(n + '\n' for n in names))
    rec = np.zeros(len(summaries), RECORD)
    for i, s in enumerate(summaries):
        rec[i] = tuple(s)
    rec.tofile(sf)
    run_program(['text', nf, sf, out], sanitize)
    return out.read_bytes()
