"""The CSV writer on the host side (no GPU): the Python restatement of writeCsv
(tests/write_csv_ref.py) against the reference's own files (tests/golden/write_csv.*, V8's
Number -> String conversions), the product's header text and row bound, and the product's number
formatting (csrc/st_numfmt.h, the functions the kernels call per cell) compiled into a stand-alone
program (tests/native/csv_cpu_check.cpp) against the restatement: the fixture inputs, a million
random bit patterns of each float type, every 8- and 16-bit integer and a million 32-bit ones.
The same program dumps the power-of-ten table, compared here entry by entry with Python integers,
and is built once more under AddressSanitizer + UBSan and run over the fixture inputs.
"""
import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import splat_hip as sh
import write_csv_ref as ref
from golden_io import Golden

C = Golden('write_csv')
CASES = list(C.meta)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CODES = {'i1': 1, 'u1': 2, 'i2': 3, 'u2': 4, 'i4': 5, 'u4': 6, 'f4': 7, 'f8': 8}


def case_columns(name):
    """[(column name, numpy array)] of a write_csv fixture case"""
    return [(c['name'], C[f'{name}_col{i}']) for i, c in enumerate(C.meta[name]['columns'])]


def case_file(name):
    return C[f'{name}_file'].tobytes()


def test_fixture_covers_the_cases():
    m = C.meta
    assert set(m) == {'empty', 'cli', 'types8', 'edges32', 'edges64', 'names'}
    assert m['empty']['rows'] == 0 and len(m['empty']['columns']) == 3
    assert m['cli']['rows'] == 64 and [c['dtype'] for c in m['cli']['columns']] == ['f4'] * 14
    assert sorted(c['dtype'] for c in m['types8']['columns']) == sorted(CODES) and m['types8']['rows'] == 300
    e32 = C['edges32_col0'].view(np.uint32)
    assert set((e32 >> 23) & 0xff) == set(range(256)) and m['edges32']['rows'] == 256 * 5 * 2
    assert {0, 1, 0x7fffff} <= set(e32[((e32 >> 23) & 0xff) == 7] & 0x7fffff) and set(e32 >> 31) == {0, 1}
    e64 = C['edges64_col0']
    assert set((e64.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)) == set(range(2048))
    for v in (1e21, 1e-6, 1e-7, 2.0**53 - 1, 2.0**53 + 2, 123456789012345680000.0, 5e-324, 1.7976931348623157e308,
              -0.0000012345678901234567, np.nextafter(1e21, 0), np.nextafter(1e-6, 1), np.nextafter(1e-7, 0)):
        assert v in e64
    names = [c['name'] for c in m['names']['columns']]
    assert any(',' in k for k in names) and any('"' in k for k in names) and any(' ' in k for k in names)
    assert any(ord(ch) > 127 for k in names for ch in k)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'write_csv.bin')) < 1_000_000


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference(name):
    assert ref.write_csv(case_columns(name)) == case_file(name)


def test_restatement_examples():
    """the issue's examples, as V8 prints them"""
    f32 = lambda x: float(np.float32(x))
    for v, s in [(f32(0.1), '0.10000000149011612'), (f32(1e21), '1.0000000200408773e+21'), (1e21, '1e+21'),
                 (1e-7, '1e-7'), (5e-324, '5e-324'), (1.7976931348623157e308, '1.7976931348623157e+308'),
                 (-0.0, '0'), (float('nan'), 'NaN'), (float('-inf'), '-Infinity'), (123456789012345680000.0,
                 '123456789012345680000'), (-0.0000012345678901234567, '-0.0000012345678901234567'), (1e-6, '0.000001'),
                 (-128, '-128'), (np.uint32(4294967295), '4294967295')]:
        assert ref.js_number(v) == s
    assert len('-0.0000012345678901234567') == 25 == max(ref.MAX_CELL.values())


# ---- the product's host-only calls -----------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_header_text_matches_reference(name):
    cols = case_columns(name)
    want = case_file(name)
    head = sh.csv_header_text(cols)
    assert head == ref.header([k for k, _ in cols]) == want[:len(head)]
    assert head.endswith(b'\n') and (C.meta[name]['rows'] > 0 or head == want)


def test_max_row_bytes():
    for dt, m in ref.MAX_CELL.items():
        assert sh.csv_max_row_bytes([('v', np.dtype(dt))]) == m + 1
    assert [ref.MAX_CELL[k] for k in ('i1', 'u1', 'i2', 'u2', 'i4', 'u4', 'f4', 'f8')] == [4, 3, 6, 5, 11, 10, 25, 25]
    for name in CASES:
        cols = case_columns(name)
        bound = sh.csv_max_row_bytes(cols)
        assert bound == sum(ref.MAX_CELL[a.dtype.str[1:]] + 1 for _, a in cols)
        lines = case_file(name).split(b'\n')[1:-1]
        assert all(len(ln) + 1 <= bound for ln in lines)
    # the bound is reached: the 25-byte value in a float64 column
    assert max(len(ln) for ln in case_file('edges64').split(b'\n')) == 25
    assert sh.csv_max_row_bytes([(f'd{i}', np.float64) for i in range(1500)]) == 1500 * 26


def test_no_columns_is_an_error():
    with pytest.raises(sh.StError) as e:
        sh.csv_header_text([])
    assert e.value.code == sh.ST_ERR_ARG


# ---- st_numfmt.h in a stand-alone program ----------------------------------------------------------
_HARNESS = {}  # built once per session into a directory of its own (removed at exit)


def _harness(sanitize=False):
    if sanitize not in _HARNESS:
        d = tempfile.mkdtemp(prefix='st_csv_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'csv_cpu_check')
        san = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
               '-fno-gpu-sanitize', '-g'] if sanitize else []
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-ffp-contract=off'] + san +
                              ['-o', exe, os.path.join(ROOT, 'tests', 'native', 'csv_cpu_check.cpp')])
        _HARNESS[sanitize] = exe
    return _HARNESS[sanitize]


def native_texts(a, tmp_path, sanitize=False):
    """the program's text and len() of every element of a numpy column: ([bytes], uint8 array)"""
    a = np.ascontiguousarray(a)
    src, txt, lens = tmp_path / 'in.bin', tmp_path / 'out.txt', tmp_path / 'out.len'
    src.write_bytes(struct.pack('<iQ', CODES[a.dtype.str[1:]], len(a)) + a.tobytes())
    r = subprocess.run([_harness(sanitize), 'values', str(src), str(txt), str(lens)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f'OK {len(a)}', (r.returncode, r.stdout, r.stderr[-2000:])
    texts = txt.read_bytes().split(b'\n')
    assert texts.pop() == b''
    return texts, np.fromfile(lens, np.uint8)


def check_column(a, tmp_path, sanitize=False):
    texts, lens = native_texts(a, tmp_path, sanitize)
    want = [s.encode() for s in ref.column_text(a)]
    assert len(texts) == len(want)
    bad = [i for i in range(len(want)) if texts[i] != want[i]]
    assert not bad, [(i, a[i], texts[i], want[i]) for i in bad[:5]]
    assert np.array_equal(lens, np.fromiter(map(len, texts), np.uint8, len(texts)))


@pytest.mark.parametrize('name', [n for n in CASES if n != 'empty'])
def test_native_formatting_on_fixture_inputs(name, tmp_path):
    for k, a in case_columns(name):
        check_column(a, tmp_path)
    # ... and against the file itself: the cells of the reference's rows
    cells = [ln.split(b',') for ln in case_file(name).split(b'\n')[1:-1]]
    for j, (k, a) in enumerate(case_columns(name)):
        assert native_texts(a, tmp_path)[0] == [row[j] for row in cells]


@pytest.mark.parametrize('dtype', ['f4', 'f8'])
def test_native_formatting_on_random_float_bits(dtype, tmp_path):
    rng = np.random.default_rng(32 if dtype == 'f4' else 64)
    with np.errstate(invalid='ignore'):
        check_column(rng.integers(0, 256, 1_000_000 * int(dtype[1]), dtype=np.uint8).view(dtype), tmp_path)


@pytest.mark.parametrize('dtype', ['i1', 'u1', 'i2', 'u2', 'i4', 'u4'])
def test_native_formatting_on_integers(dtype, tmp_path):
    dt = np.dtype(dtype)
    if dt.itemsize == 1:
        a = np.arange(256, dtype=np.uint8).view(dt)
    elif dt.itemsize == 2:
        a = np.arange(65536, dtype=np.uint16).view(dt)
    else:
        a = np.random.default_rng(5).integers(0, 256, 4_000_000, dtype=np.uint8).view(dt)
        a[:4] = np.array([0, 1, 0x7fffffff, 0x80000000], np.uint32).view(dt)
        a[4] = np.array([0xffffffff], np.uint32).view(dt)[0]
    check_column(a, tmp_path)


def test_native_formatting_on_shaped_floats(tmp_path):
    """what random bits rarely give: integer-valued floats, powers of ten, bell-shaped values, subnormals"""
    rng = np.random.default_rng(9)
    pows = np.array([float(f'1e{e}') for e in range(-323, 309)])
    check_column(np.concatenate([pows, -pows, np.nextafter(pows, 0), np.nextafter(pows, np.inf)]), tmp_path)
    check_column(pows[(pows > 1e-45) & (pows < 3e38)].astype(np.float32), tmp_path)
    check_column(rng.integers(-10**7, 10**7, 100_000).astype(np.float64), tmp_path)
    check_column(rng.integers(-2**24, 2**24, 100_000).astype(np.float32), tmp_path)
    check_column(rng.normal(0, 1, 100_000).astype(np.float32), tmp_path)
    check_column(rng.normal(0, 1, 100_000), tmp_path)
    check_column(np.arange(1, 50_000, dtype=np.uint32).view(np.float32), tmp_path)                # float32 subnormals
    check_column(rng.integers(1, 2**52, 100_000, dtype=np.uint64).view(np.float64), tmp_path)    # float64 subnormals
    check_column(2.0 ** np.arange(-1074, 1024), tmp_path)                                         # the irregular spacing


def test_power_table_matches_its_definition(tmp_path):
    """entry e = ceil(10^e * 2^(127 - floor(log2 10^e))), e = -292 .. 324, as (high, low) halves"""
    out = tmp_path / 'table.bin'
    subprocess.run([_harness(), 'table', str(out)], check=True)
    tab = np.fromfile(out, np.uint64).reshape(-1, 2)
    assert len(tab) == 324 + 292 + 1
    for row, e in zip(tab.tolist(), range(-292, 325)):
        if e >= 0:
            p = 10 ** e
            fl = p.bit_length() - 1
            want = p << (127 - fl) if fl <= 127 else -((-p) >> (fl - 127))
        else:
            q = 10 ** -e
            fl = -q.bit_length()                  # 2^fl < 10^e < 2^(fl + 1): q is no power of two
            want = -((-(1 << (127 - fl))) // q)   # ceil(2^(127 - fl) / q)
        assert 1 << 127 <= want < 1 << 128
        assert (row[0] << 64) | row[1] == want, e


@pytest.mark.parametrize('name', [n for n in CASES if n != 'empty'])
def test_native_formatting_under_sanitizers(name, tmp_path):
    """the same program built with -fsanitize=address,undefined (host code; it links no device
    code of its own), run stand-alone over the fixture inputs"""
    for k, a in case_columns(name):
        check_column(a, tmp_path, sanitize=True)
