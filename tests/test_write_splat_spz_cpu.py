"""The .splat / .spz writers without a GPU: the numpy restatement of the encode rules
(tests/write_splat_spz_ref.py) against the reference's own data -- writing the columns the
reference's readers decoded from the committed fixture files (tests/golden/readers.*,
readers_edges.*) gives the files' bytes back --, its half-step accuracy through the readers'
restatement (oracle/readers.py), spz_deflate, and st_writers.hip's __host__ __device__ encode
functions in a stand-alone program (tests/native/writers_cpu_check.cpp) byte for byte against
the restatement.

The fixture files' header byte 14 is 1 (the generator's flags byte); the rules write 0 there, so
the header comparison covers bytes 0-13 and 15: magic, version, count, degree, fractional bits."""
import atexit
import gzip
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import oracle_typed as ot
import readers as oracle_readers
import splat_hip as sh
import write_splat_spz_ref as ref
from golden_io import Golden, bell_splats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {name: Golden(name) for name in ('readers', 'readers_edges')}
SPZ_CASES = ['spz_v2_d0_n300', 'spz_v2_d1_n300', 'spz_v2_d2_n300', 'spz_v2_d3_n300', 'spz_v2_d0_n1', 'spz_v2_d0_n257',
             'spz_v2_d0_n259', 'spz_v2_d2_n257', 'spz_v2_d2_n258', 'spz_v2_d2_n259', 'spz_v2_d2_n5', 'spz_v2_d3_n257']
SPLAT_CASES = ['splat_n1', 'splat_n255', 'splat_n257', 'splat_n1025']
PLANE_BYTES = {'positions': 9, 'alphas': 1, 'colours': 3, 'scales': 3, 'rotations': 3}


def fixture(name):
    """(the file's bytes -- inflated for .spz --, [(column, float32 array)] as the reference decoded it)"""
    for g in SETS.values():
        c = next((c for c in g.meta['cases'] if c['name'] == name), None)
        if c is not None:
            data = g[name + '_file'].tobytes()
            cols = g[name + '_cols']
            return (gzip.decompress(data) if c['format'] == 'spz' else data), [(k, cols[i]) for i, k in enumerate(c['columns'])]
    raise KeyError(name)


def split_planes(raw):
    """{plane: uint8 [n, bytes per splat]} of a raw version-2 image"""
    n = struct.unpack_from('<I', raw, 8)[0]
    nsh = (len(raw) - 16) // n - 19 if n else 0
    out, off = {}, 16
    for p in ref.PLANES:
        w = PLANE_BYTES.get(p, nsh)
        out[p] = np.frombuffer(raw, np.uint8, n * w, off).reshape(n, w)
        off += n * w
    assert off == len(raw)
    return out


def check_spz_against_file(image, raw, cols):
    """the conditions under which an image written from a fixture's columns must equal its file"""
    assert len(image) == len(raw)
    assert image[:14] == raw[:14] and image[15] == raw[15] and image[14] == 0
    got, want = split_planes(image), split_planes(raw)
    for p in ref.PLANES:
        if p != 'rotations':
            assert np.array_equal(got[p], want[p]), p
    # where the three stored components exceed unit length the reader's w = 0 loses the bytes
    keep = dict(cols)['rot_0'] > 0
    assert keep.sum() >= 0.4 * len(keep)
    assert np.array_equal(got['rotations'][keep], want['rotations'][keep])
    return int(keep.sum())


def is_snan32(w):
    return ((w & 0x7f800000) == 0x7f800000) & ((w & 0x007fffff) != 0) & ((w & 0x00400000) == 0)


def check_splat_against_file(rows, data, cols):
    """the same for .splat rows: uint8 [n, 32] against the file's bytes"""
    n = len(data) // 32
    file = np.frombuffer(data, np.uint8).reshape(n, 32)
    assert rows.shape == file.shape
    assert np.array_equal(rows[:, 24:28], file[:, 24:28])
    gw = np.ascontiguousarray(rows[:, :24]).view('<u4').astype(np.int64)
    fw = np.ascontiguousarray(file[:, :24]).view('<u4').astype(np.int64)
    snan = is_snan32(fw[:, :3])
    if n >= 255:
        assert snan.sum() == 1
    assert np.array_equal(gw[:, :3][~snan], fw[:, :3][~snan])
    # exp of the float32-rounded log: the rounding amplified by exp, in float32 units in the last place
    worst = 0
    table = dict(cols)
    for k in range(3):
        f = fw[:, 3 + k]
        ok = (f > 0) & (f < 0x7f800000)  # finite and positive
        bound = np.ceil(np.abs(table[f'scale_{k}'].astype(np.float64))) + 1
        ulps = np.abs(gw[:, 3 + k] - f)
        assert (ulps[ok] <= bound[ok]).all(), (k, ulps[ok].max())
        worst = max(worst, int(ulps[ok].max()) if ok.any() else 0)
    return worst


# ---- 1. the restatement against the reference's data ------------------------------------------------
@pytest.mark.parametrize('name', SPZ_CASES)
def test_spz_restatement_gives_the_fixture_file_back(name):
    raw, cols = fixture(name)
    assert raw[4] == 2 and raw[13] <= 23 and raw[12] <= 3
    image, clamped = ref.spz_image(cols, raw[13])
    compared = check_spz_against_file(image, raw, cols)
    print(name, 'rotation rows compared:', compared, 'of', len(cols[0][1]))
    assert clamped == 0


@pytest.mark.parametrize('name', SPLAT_CASES)
def test_splat_restatement_gives_the_fixture_file_back(name):
    data, cols = fixture(name)
    worst = check_splat_against_file(ref.splat_rows(cols), data, cols)
    print(name, 'largest scale distance in float32 ulps:', worst)


# ---- 2. half-step accuracy ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bell():
    names, cols = bell_splats(300, 15, 1, 0.05)
    return [(k, cols[k]) for k in names]


def test_spz_half_step_accuracy(bell):
    fb = 12
    image, clamped = ref.spz_image(bell, fb)
    back, n, nsh = oracle_readers.read_spz(image)
    assert (n, nsh, clamped) == (300, 45, 0)
    back = dict(zip(sh.reader_columns(nsh), back.astype(np.float64)))
    src = {k: a.astype(np.float64) for k, a in bell}
    for k in 'xyz':
        assert (np.abs(src[k]) * 2.0 ** fb < 2 ** 23 - 1).all()
        assert np.abs(back[k] - src[k]).max() <= 2.0 ** -(fb + 1)
    for k in range(3):
        s = src[f'scale_{k}']
        ok = (s >= -10) & (s <= 5.9375)
        assert ok.all() and np.abs(back[f'scale_{k}'] - s)[ok].max() <= 1 / 32
        c = src[f'f_dc_{k}']
        ok = ((c * 0.15 + 0.5) * 255 >= 0) & ((c * 0.15 + 0.5) * 255 <= 255)
        assert ok.sum() > 250 and np.abs(back[f'f_dc_{k}'] - c)[ok].max() <= 0.5 / (255 * 0.15)
    for i in range(45):
        h = src[f'f_rest_{i}']
        ok = (h >= -1) & (h <= 127 / 128)
        assert ok.all() and np.abs(back[f'f_rest_{i}'] - h)[ok].max() <= 1 / 256


def test_splat_half_step_accuracy(bell):
    rows = ref.splat_rows(bell)
    back, n, nsh = oracle_readers.read_splat(rows.tobytes())
    assert (n, nsh) == (300, 0)
    back = dict(zip(sh.reader_columns(0), back))
    src = dict(bell)
    for k in 'xyz':
        assert np.array_equal(back[k].view(np.uint32), src[k].view(np.uint32))
    for k in range(3):
        c = src[f'f_dc_{k}'].astype(np.float64)
        ok = ((c * ref.SH_C0 + 0.5) * 255 >= 0) & ((c * ref.SH_C0 + 0.5) * 255 <= 255)
        assert ok.sum() > 150
        assert np.abs(back[f'f_dc_{k}'].astype(np.float64) - c)[ok].max() <= 0.5 / (255 * ref.SH_C0)


# ---- 3. spz_deflate ------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,segment', [(0, 8 << 20), (1, 8 << 20), (4096 + 1, 4096), (3 * 4096, 4096),
                                          (100_000, 8 << 20)])
@pytest.mark.parametrize('level', [1, 6, 9])
def test_spz_deflate_is_one_member_whatever_the_threads(size, segment, level):
    rng = np.random.default_rng(size)
    raw = (rng.integers(0, 256, size, dtype=np.uint8) & rng.integers(0, 256, size, dtype=np.uint8)).tobytes()
    one = sh.spz_deflate(raw, level, threads=1, _segment=segment)
    assert one == sh.spz_deflate(raw, level, threads=8, _segment=segment)
    assert one == sh.spz_deflate(np.frombuffer(raw, np.uint8), level, _segment=segment)
    assert one[:10] == b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff'  # no name, mtime 0
    assert gzip.decompress(one) == raw
    d = zlib.decompressobj(31)
    assert d.decompress(one) == raw
    assert d.eof and d.unused_data == b''


def test_spz_deflate_default_segment():
    assert sh.SPZ_DEFLATE_SEGMENT == 8 << 20


def test_spz_image_size():
    assert sh.spz_image_size(0, 0) == 16
    assert sh.spz_image_size(300, 15) == 16 + 300 * 64
    assert sh.spz_image_size(257, 8) == 16 + 257 * 43
    assert sh.spz_image_size((1 << 32) - 1, 15) == 16 + ((1 << 32) - 1) * 64
    assert sh.spz_image_size(1 << 32, 0) == 0
    assert sh.spz_image_size(10, 4) == 0 and sh.spz_image_size(10, -1) == 0


# ---- 4. the product's encode functions on the host -------------------------------------------------------
NP_TO_PLY = {np.dtype(t): i for i, t in enumerate(
    [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64], start=1)}
SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30]


def ordinary(rng, n, C, dtype=np.float32):
    """a plain table of n rows in the readers' column order with 3C f_rest columns"""
    cols = [(k, rng.normal(0, 1.5, n).astype(dtype)) for k in sh.reader_columns(3 * C)]
    return [(k, (a * 20).astype(dtype) if k in 'xyz' else (a - 4).astype(dtype) if k.startswith('scale') else
             (a / 4).astype(dtype) if k.startswith('f_rest') else a) for k, a in cols]


def specials_table(dtype=np.float32):
    """every special in every column, one column at a time: 7 rows per column"""
    names = sh.reader_columns(9)
    cols = dict(ordinary(np.random.default_rng(7), 7 * len(names), 3, dtype))
    for j, k in enumerate(names):
        cols[k][7 * j:7 * j + 7] = np.array(SPECIALS, np.float64).astype(dtype)
    return [(k, cols[k]) for k in names]


def boundaries_table():
    """values exactly on rounding boundaries and at the clamp ends, float64 columns (every value
    exact), fractional_bits 12"""
    n = 1024
    cols = dict(ordinary(np.random.default_rng(8), n, 15, np.float64))
    k = np.arange(n, dtype=np.float64)
    cols['scale_0'] = ((k % 256) + 0.5) / 16 - 10            # every scale boundary
    cols['scale_1'] = np.nextafter(cols['scale_0'], -np.inf)  # ... and its two neighbours
    cols['scale_2'] = np.nextafter(cols['scale_0'], np.inf)
    cols['x'] = (k - 512 + 0.5) / 4096                        # position boundaries around zero
    cols['y'] = np.nextafter(cols['x'], -np.inf)
    ends = np.array([2 ** 23 - 1, 2 ** 23, -2 ** 23, -2 ** 23 - 1, 2 ** 23 - 0.5, 2 ** 23 - 1.5, -2 ** 23 - 0.5,
                     -2 ** 23 - 0.5000001, 1e300, -1e300], np.float64) / 4096
    cols['z'] = np.resize(ends, n)                            # at and one past both clamp ends
    cols['f_rest_0'] = ((k % 256) + 0.5) / 128 - 1            # harmonics boundaries
    cols['f_rest_44'] = np.nextafter(cols['f_rest_0'], -np.inf)
    cols['f_dc_0'] = (((k % 256) + 0.5) / 255 - 0.5) / 0.15   # near the colour boundaries (not exact)
    cols['opacity'] = (k - 512) / 16
    return [(kk, cols[kk]) for kk in sh.reader_columns(45)]


def quaternions_table():
    """the zero quaternion, rot_0 < 0, rot_0 = -0, squares that overflow, non-finite members"""
    q = np.array([[0, 0, 0, 0], [-0.0, 0, 0, 0], [-1, 0, 0, 0], [-0.5, 0.5, -0.5, 0.5], [-0.0, 1, 2, 3], [0.0, -1, -2, -3],
                  [1e200, 1, 1, 1], [-1e200, 1e200, 0, 0], [1e-200, 0, 0, 0], [-1e-170, 1e-170, 0, 0], [np.inf, 1, 1, 1],
                  [1, np.nan, 1, 1], [-3e38, 3e38, 3e38, 3e38], [5e-324, 0, 0, 0], [-1, 1e-9, -1e-9, 0],
                  [-1e-9, 1, 0, 0]], np.float64)
    cols = dict(ordinary(np.random.default_rng(9), len(q), 0, np.float64))
    for k in range(4):
        cols[f'rot_{k}'] = q[:, k].copy()
    return [(k, cols[k]) for k in sh.reader_columns(0)]


def mixed_types_table():
    """float64, int32 and uint8 (and the other integer types) among the fourteen, extra columns
    between them, a second `x` that must lose, f_rest columns up to band 2 with a gap after it"""
    rng = np.random.default_rng(10)
    n = 600
    cols = [('nx', rng.normal(0, 1, n).astype(np.float32)),
            ('x', rng.normal(0, 30, n)), ('y', rng.integers(-3000, 3000, n).astype(np.int32)),
            ('z', rng.integers(-128, 128, n).astype(np.int8)),
            ('x', np.full(n, 99.0, np.float32)),
            ('scale_0', rng.integers(-12, 8, n).astype(np.int16)), ('scale_1', rng.normal(-4, 2, n).astype(np.float32)),
            ('scale_2', rng.integers(0, 7, n).astype(np.uint8)),
            ('f_dc_0', rng.normal(0, 1, n)), ('f_dc_1', rng.integers(0, 3, n).astype(np.uint16)),
            ('f_dc_2', rng.integers(0, 3, n).astype(np.uint32)),
            ('opacity', rng.integers(-9, 9, n).astype(np.int32)),
            ('rot_0', rng.integers(-5, 5, n).astype(np.int8)), ('rot_1', rng.normal(0, 1, n)),
            ('rot_2', rng.integers(0, 5, n).astype(np.uint8)), ('rot_3', rng.normal(0, 1, n).astype(np.float32))]
    cols += [(f'f_rest_{i}', rng.normal(0, 0.4, n).astype(np.float32 if i % 2 else np.float64)) for i in range(24)]
    cols += [('f_rest_30', np.zeros(n, np.float32))]
    return cols


def directed_tables():
    """{name: (columns, fractional_bits)}: the tables of the issue's native and GPU comparisons"""
    return {'specials_f32': (specials_table(np.float32), 12), 'specials_f64': (specials_table(np.float64), 10),
            'boundaries': (boundaries_table(), 12), 'quaternions': (quaternions_table(), 12),
            'mixed_types': (mixed_types_table(), 8)}


_HARNESS = []  # built once per session into a directory of its own (removed at exit)
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _harness():
    if not _HARNESS:
        d = tempfile.mkdtemp(prefix='st_writers_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'writers_cpu_check')
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-ffp-contract=off', '-o', exe,
                               os.path.join(ROOT, 'tests', 'native', 'writers_cpu_check.cpp')])
        _HARNESS.append(exe)
    return _HARNESS[0]


def native(fmt, cols, fb, tmp_path):
    """(output bytes, sh_coeffs, clamped) of the product's host encode, or the 'ERR ...' line"""
    src, dst = tmp_path / f'{fmt}.table', tmp_path / f'{fmt}.out'
    n = len(cols[0][1])
    with open(src, 'wb') as f:
        f.write(struct.pack('<QII', n, len(cols), 0))
        for k, a in cols:
            f.write(struct.pack('<I28s', NP_TO_PLY[np.asarray(a).dtype], k.encode()))
        for _, a in cols:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([_harness(), fmt, str(fb), str(src), str(dst)], capture_output=True, text=True, check=True)
    words = r.stdout.split()
    if words[0] != 'OK':
        return r.stdout.strip()
    assert int(words[1]) == n
    return dst.read_bytes(), int(words[2]), int(words[3])


def first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    if len(a) != len(b):
        return 'lengths', len(a), len(b)
    d = np.flatnonzero(a != b)
    return (int(d[0]), int(a[d[0]]), int(b[d[0]]), len(d)) if len(d) else None


def check_native(cols, fb, tmp_path):
    got, C, clamped = native('spz', cols, fb, tmp_path)
    want, want_clamped = ref.spz_image(cols, fb)
    assert first_difference(got, want) is None
    assert (C, clamped) == (ot.band_coeffs({k for k, _ in cols}), want_clamped)
    got, _, _ = native('splat', cols, 0, tmp_path)
    assert first_difference(got, ref.splat_rows(cols).tobytes()) is None
    return clamped


@pytest.mark.parametrize('name', SPZ_CASES + SPLAT_CASES)
def test_host_encode_matches_restatement_on_fixture_columns(name, tmp_path):
    raw, cols = fixture(name)
    check_native(cols, raw[13] if name.startswith('spz') else 12, tmp_path)


@pytest.mark.parametrize('name', list(directed_tables()))
def test_host_encode_matches_restatement_on_directed_tables(name, tmp_path):
    cols, fb = directed_tables()[name]
    clamped = check_native(cols, fb, tmp_path)
    if name == 'boundaries':   # z: 7 of every 10 values are past an end; x and y: none
        z = dict(cols)['z'] * 4096
        assert clamped == int(((np.floor(z + 0.5) > 2 ** 23 - 1) | (np.floor(z + 0.5) < -2 ** 23)).sum()) > 0
    if name.startswith('specials'):
        assert clamped == 3 * 5   # NaN, +-Inf and +-1e30 in each of x, y and z


def test_host_encode_fractional_bits_ends(tmp_path):
    cols, _ = directed_tables()['boundaries']
    for fb in (0, 23):
        got, _, clamped = native('spz', cols, fb, tmp_path)
        want, want_clamped = ref.spz_image(cols, fb)
        assert first_difference(got, want) is None and clamped == want_clamped


def test_host_encode_argument_errors(tmp_path):
    cols, _ = directed_tables()['quaternions']
    for fb in (-1, 24):
        assert native('spz', cols, fb, tmp_path).startswith(f'ERR {sh.ST_ERR_ARG} ')
    for missing in ('x', 'opacity', 'rot_3'):
        line = native('spz', [(k, a) for k, a in cols if k != missing], 12, tmp_path)
        assert line.startswith(f'ERR {sh.ST_ERR_ARG} ') and line.endswith('missing column ' + missing)
        line = native('splat', [(k, a) for k, a in cols if k != missing], 12, tmp_path)
        assert line.startswith(f'ERR {sh.ST_ERR_ARG} ') and line.endswith('missing column ' + missing)
    empty = [(k, a[:0]) for k, a in cols]
    assert native('splat', empty, 0, tmp_path).startswith(f'ERR {sh.ST_ERR_ARG} ')
    got, C, clamped = native('spz', empty, 12, tmp_path)
    assert (got, C, clamped) == (ref.spz_image(empty, 12)[0], 0, 0) and len(got) == 16
