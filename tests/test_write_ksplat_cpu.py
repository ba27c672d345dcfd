"""The .ksplat writer without a GPU: the numpy restatement of its rules (tests/write_ksplat_ref.py)
against the reference's own data -- re-encoding the columns the reference's reader decoded from the
committed fixture files, through each file's own bucket table, gives the files' record bytes back
outside the classes of fields a decode cannot give back --, the nearest-code property through the
readers' restatement (oracle/readers.py), the plan on tables whose outcome is known by construction,
the round trip of whole images, and st_ksplat_encode.h's __host__ __device__ functions in a
stand-alone program (tests/native/ksplat_write_cpu_check.cpp), plain and under ASan/UBSan, byte for
byte against the restatement.

Shares of the fixture rows each class excuses, as this test prints them (pytest -s), are recorded in
DESIGN.md (g).  One class is not in the list the feature was specified with: `past_table`, the
position fields of records whose bucket index lies past the file's centre table.  The reader reads
`undefined` there and stores NaN whatever the code was (ksplat_partial_short,
ksplat_m2_walk257_short), so no writer can give those codes back; like every class it is computed
from the file's bytes alone."""
import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_typed as ot
import readers as oracle_readers
import splat_hip as sh
import write_ksplat_cases as kc
import write_ksplat_ref as ref
from readers_files import ksplat_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_TO_PLY = {np.dtype(t): i for i, t in enumerate(
    [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64], start=1)}


# ---- anchor on the fixtures ------------------------------------------------------------------------
def f32_ulps(a, b):
    """distance of two float32 bit patterns of one sign in units in the last place"""
    return np.abs(a.astype(np.int64) - b.astype(np.int64))


@pytest.mark.parametrize('set_name,name', kc.KSPLAT_CASES, ids=[n for _, n in kc.KSPLAT_CASES])
def test_restatement_gives_the_fixture_records_back(set_name, name):
    data, cols, _ = kc.fixture(set_name, name)
    for sec in kc.sections(data, cols):
        want, got = sec['records'], kc.restated(sec)
        assert got.shape == want.shape
        cls = kc.excused(sec)
        diff = got != want
        allowed = np.zeros_like(diff)
        for k, m in cls.items():
            share = float(m.any(axis=1).mean())
            print(f'{name} rows {sec["row0"]}+{len(want)} mode {sec["mode"]} degree {sec["degree"]}: class {k} '
                  f'excuses {100 * share:.1f} % of rows')
            if k != 'scale_log':
                allowed |= m
        # mode 0 scales through a float32 log: |log t| <= 104 carries half a float32 step of its own,
        # |s| * 2^-24, which exp turns into a relative error <= |s| * 2^-24 <= |s| float32 steps of t;
        # the final rounding adds half a step: within ceil(|s|) + 1 steps, i.e. 2 ceil(|s|) + 2 halves
        if sec['mode'] == 0:
            table = dict(sec['table'])
            for k in range(3):
                m = cls['scale_log'][:, 12 + 4 * k]
                a, b = kc.words(got, 12 + 4 * k, 1, 4)[:, 0], kc.words(want, 12 + 4 * k, 1, 4)[:, 0]
                bound = np.ceil(np.abs(table[f'scale_{k}'].astype(np.float64))) + 1
                assert (f32_ulps(a, b)[m] <= bound[m]).all(), (name, k)
                allowed[:, 12 + 4 * k:16 + 4 * k] |= m[:, None]
                print(f'{name}: scale_{k} differs on {100 * float((a != b)[m].mean()) if m.any() else 0:.1f} % of '
                      f'its rows, at most {int(f32_ulps(a, b)[m].max()) if m.any() else 0} float32 steps')
        bad = np.argwhere(diff & ~allowed)
        assert len(bad) == 0, (name, [(int(r), int(b), int(got[r, b]), int(want[r, b])) for r, b in bad[:8]])
        # colour and opacity have no exception at all
        c0 = kc.KS_COLOUR[sec['mode']]
        assert not allowed[:, c0:c0 + 4].any() and np.array_equal(got[:, c0:c0 + 4], want[:, c0:c0 + 4])
        if name in kc.NINE:
            # position, colour, opacity and finite harmonics fields match on every row
            # (mode 0 float32 words that are signalling NaNs apart: the reader quiets them)
            assert not (cls['ps'].any() or cls['past_table'].any() or cls['sh_range'].any())
            width = 12 if sec['mode'] == 0 else 6
            keep = ~cls['snan'][:, :width]
            assert np.array_equal(got[:, :width][keep], want[:, :width][keep])
            h0 = ref.BASE[sec['mode']]
            keep = ~(cls['half_nan'] | cls['snan'])[:, h0:]
            assert np.array_equal(got[:, h0:][keep], want[:, h0:][keep])


# ---- nearest-code property ---------------------------------------------------------------------------
def decode_centre(codes, centre, block, quant):
    """x of one-record-per-code mode 1 files through the readers' restatement"""
    n = len(codes)
    rec = np.zeros((n, 24), np.uint8)
    rec[:, 0:2] = np.asarray(codes, '<u2').view(np.uint8).reshape(n, 2)
    sec = dict(count=n, max=n, degree=0, capacity=n, buckets=1, full=1, partial=[], block=block, storage=12, quant=quant,
               centres=np.array([centre, 0, 0], np.float32), records=rec)
    out, _, _ = oracle_readers.read_ksplat(ksplat_file(1, [sec]))
    return out[0].astype(np.float64)


def decode_sh8(codes, sh_min, sh_max):
    n = len(codes)
    rec = np.zeros((n, 24 + 9), np.uint8)
    rec[:, 24] = codes
    sec = dict(count=n, max=n, degree=1, capacity=n, buckets=1, full=1, partial=[], block=5.0, storage=12, quant=0,
               centres=np.zeros(3, np.float32), records=rec)
    out, _, _ = oracle_readers.read_ksplat(ksplat_file(2, [sec], sh_min, sh_max))
    return out[14].astype(np.float64)


def decode_half(codes):
    n = len(codes)
    rec = np.zeros((n, 24 + 18), np.uint8)
    rec[:, 24:26] = np.asarray(codes, '<u2').view(np.uint8).reshape(n, 2)
    sec = dict(count=n, max=n, degree=1, capacity=n, buckets=1, full=1, partial=[], block=5.0, storage=12, quant=0,
               centres=np.zeros(3, np.float32), records=rec)
    out, _, _ = oracle_readers.read_ksplat(ksplat_file(1, [sec]))
    return out[14].astype(np.float64)


def decode_colour(codes, opacity=False):
    n = len(codes)
    rec = np.zeros((n, 24), np.uint8)
    rec[:, 23 if opacity else 20] = codes
    sec = dict(count=n, max=n, degree=0, capacity=n, buckets=1, full=1, partial=[], block=5.0, storage=12, quant=0,
               centres=np.zeros(3, np.float32), records=rec)
    out, _, _ = oracle_readers.read_ksplat(ksplat_file(1, [sec]))
    return out[9 if opacity else 6].astype(np.float64)


def assert_nearest(v, code, top, decode, what, slack=0.0):
    """|decode(code) - v| <= |decode(code +- 1) - v| + slack wherever the neighbour exists"""
    v = np.asarray(v, np.float64)
    code = code.astype(np.int64)
    with np.errstate(all='ignore'):
        d0 = np.abs(decode(code) - v)
        for step in (-1, 1):
            nb = code + step
            ok = (nb >= 0) & (nb <= top)
            d = np.abs(decode(np.clip(nb, 0, top)) - v)
            bad = ok & (d + slack < d0)
            assert not bad.any(), (what, step, v[bad][:4], code[bad][:4])


@pytest.mark.parametrize('centre,block,quant', [(0.0, 5.0, 32767), (2.5, 5.0, 32767), (-1237.5, 5.0, 32767),
                                                (99997.5, 5.0, 32767), (0.625, 1.25, 32767), (12.5, 5.0, 1000),
                                                (3e6, 0.5, 32767)])
def test_centre_code_is_the_nearest(centre, block, quant):
    rng = np.random.default_rng(21)
    ps = block / 2.0 / quant
    c = float(np.float32(centre))
    k = np.r_[0, 1, 2, 32766, 32767, 32768, 65533, 65534, 65535, rng.integers(0, 65536, 200)].astype(np.float64)
    exact = (k - quant) * ps + c
    mid = exact + ps / 2                     # ties and the values beside each rounding boundary
    v = np.r_[exact, mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf),
              np.float32(mid).astype(np.float64), c + rng.uniform(-1.2, 1.2, 400) * block / 2,
              c - 1e9, c + 1e9, -np.inf, np.inf, c - (quant + 0.5) * ps, c + (65535.5 - quant) * ps]
    code = ref.centre_code(v, np.full(len(v), c), ps, float(quant))
    assert_nearest(v, code, 65535, lambda kk: decode_centre(kk, centre, block, quant if quant != 32767 else 0), 'centre')
    # both clamp ends
    assert code[-4] == 0 and code[-3] == 65535 and code[-6] == 0 and code[-5] == 65535
    assert ref.centre_code(np.array([np.nan]), np.array([c]), ps, float(quant))[0] == 0


@pytest.mark.parametrize('sh_min,sh_max', [(-1.5, 1.5), (-0.25, 4.0), (1e-3, 2e-3), (-3e4, 7.0)])
def test_mode2_harmonic_code_is_the_nearest(sh_min, sh_max):
    rng = np.random.default_rng(22)
    lo, hi = float(np.float32(sh_min)), float(np.float32(sh_max))
    b = np.arange(256, dtype=np.float64)
    exact = lo + b / 255 * (hi - lo)
    mid = exact + (hi - lo) / 510
    v = np.r_[exact, mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), np.float32(mid).astype(np.float64),
              rng.uniform(lo - (hi - lo) * 0.1, hi + (hi - lo) * 0.1, 500), lo - 1e6, hi + 1e6, -np.inf, np.inf]
    code = ref.sh8_code(v, sh_min, sh_max)
    assert_nearest(v, code, 255, lambda kk: decode_sh8(kk.astype(np.uint8), sh_min, sh_max), 'sh8')
    assert code[-4] == 0 and code[-3] == 255 and code[-2] == 0 and code[-1] == 255
    assert ref.sh8_code(np.array([np.nan]), sh_min, sh_max)[0] == 0


def test_half_code_is_the_nearest():
    """H(t) against decodeFloat16: IEEE's rule, in which +-Inf stand at +-65536 for the comparison (a
    value of 65520 or more is nearer to 2^16 than to 65504, the largest finite half)"""
    rng = np.random.default_rng(23)
    h = np.r_[0, 1, 2, 0x3ff, 0x400, 0x401, 0x3c00, 0x7bfe, 0x7bff, rng.integers(0, 0x7c00, 300)].astype(np.uint16)
    exact = kc.half_value(h)
    nxt = kc.half_value(np.minimum(h + 1, 0x7bff).astype(np.uint16))
    mid = (exact + nxt) / 2
    v = np.r_[exact, mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), 65519.999, 65520.0, 65536.0, 1e30,
              2.0 ** -25, np.nextafter(2.0 ** -25, 1), 2.0 ** -26, rng.lognormal(0, 6, 400)]
    v = np.r_[v, -v]
    code = ref.half_bits(v)

    def decode(c):
        d = decode_half(c.astype(np.uint16))
        return np.where(np.isinf(d), np.sign(d) * 65536.0, d)
    mag = (code & 0x7fff).astype(np.int64)
    sign = np.where(code & 0x8000, -1.0, 1.0)
    d0 = np.abs(decode(code) - v)
    for step in (-1, 1):
        nb = mag + step
        ok = (nb >= 0) & (nb <= 0x7c00)
        d = np.abs(sign * np.abs(decode(np.clip(nb, 0, 0x7c00))) - v)
        assert not (ok & (d < d0)).any(), step
    # ties go to the even code; the ends
    assert ref.half_bits(np.array([65519.999]))[0] == 0x7bff and ref.half_bits(np.array([65520.0]))[0] == 0x7c00
    assert ref.half_bits(np.array([-1e30]))[0] == 0xfc00 and ref.half_bits(np.array([np.nan]))[0] == 0x7e00
    assert ref.half_bits(np.array([2.0 ** -25]))[0] == 0 and ref.half_bits(np.array([3 * 2.0 ** -25]))[0] == 2
    assert ref.half_bits(np.array([-0.0]))[0] == 0x8000


def test_colour_and_opacity_bytes_are_the_nearest():
    """the .splat writer's closed forms, which no decode corrects: on an exact tie the two neighbours'
    decoded values differ from the tie only by the reader's float32 store, so the comparison allows
    that store's error on both sides: 2^-24 of the largest colour (1.78 < 2), twice.  For opacity the
    stored logit o carries |o| 2^-24 and the probability p (1 - p) times that: below 2^-25 for
    1/255 <= p <= 254/255 (p (1 - p) |o| < 0.3), twice"""
    rng = np.random.default_rng(24)
    b = np.arange(256, dtype=np.float64)
    v = np.r_[(b / 255 - 0.5) / ref.SH_C0, ((b + 0.5) / 255 - 0.5) / ref.SH_C0, rng.normal(0, 1.5, 500), -50, 50,
              -np.inf, np.inf]
    with np.errstate(all='ignore'):
        code = ref.q8((v * ref.SH_C0 + 0.5) * 255.0)
    assert_nearest(v, code, 255, lambda kk: decode_colour(kk.astype(np.uint8)), 'colour', 2.0 ** -22)
    assert code[-4] == 0 and code[-3] == 255
    # opacity: compared as the reader's clamped probability, the quantity the byte holds
    p = np.r_[(b[1:255]) / 255, (b[1:255] + 0.5) / 255, rng.uniform(0.01, 0.99, 400)]
    o = np.log(p / (1 - p))
    with np.errstate(all='ignore'):
        code = ref.q8(ref.sigmoid(np.r_[o, -40, 40, -np.inf, np.inf]) * 255.0)
    assert code[-4] == 0 and code[-3] == 255 and code[-2] == 0 and code[-1] == 255
    sig = lambda x: 1 / (1 + np.exp(-x))  # noqa: E731
    assert_nearest(p, code[:-4], 255, lambda kk: sig(decode_colour(kk.astype(np.uint8), True)), 'opacity', 2.0 ** -24)


# ---- plan properties ---------------------------------------------------------------------------------
PLAN_TABLES = kc.plan_tables()


def check_plan_invariants(cols, block, p):
    t = ref.table(cols)
    n = len(t['x'])
    order, bucket = p['order'].astype(np.int64), p['bucket'].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n))
    F, P = p['full'], p['partial']
    sizes = np.r_[np.full(F, 256), p['partial_sizes']].astype(np.int64)
    assert (sizes > 0).all() and (p['partial_sizes'] < 256).all() and sizes.sum() == n
    assert np.array_equal(bucket, np.repeat(np.arange(F + P), sizes))
    key = p['key'][order]
    bkey = key[np.r_[0, np.cumsum(sizes)[:-1]]]
    assert (key == np.repeat(bkey, sizes)).all()                       # one cell per bucket
    assert (np.diff(bkey[:F].astype(np.int64)) >= 0).all() and (np.diff(bkey[F:].astype(np.int64)) > 0).all()
    for b0, b1 in ((0, F * 256), (F * 256, n)):                         # stable inside each region
        k, o = key[b0:b1], order[b0:b1]
        same = k[1:] == k[:-1]
        assert (o[1:][same] > o[:-1][same]).all()


@pytest.mark.parametrize('name', list(PLAN_TABLES))
def test_plan_properties(name):
    cols, block, expected = PLAN_TABLES[name]
    p = ref.plan(cols, block)
    check_plan_invariants(cols, block, p)
    if expected:
        F, P, sizes, clamped = expected
        assert (p['full'], p['partial'], p['partial_sizes'].tolist(), p['clamped']) == (F, P, sizes, clamped)
    t = dict(cols)
    if name == 'two_cells':
        cell = (t['x'][p['order']] > 4).astype(int)
        assert cell.tolist() == [0] * 256 + [0] * 44 + [1] * 212 and p['bucket'].tolist() == [0] * 256 + [1] * 44 + [2] * 212
    if name == 'reverse':
        assert p['order'].tolist() == [r for c in range(5, -1, -1) for r in range(100 * c, 100 * c + 100)]
    if name == 'axis_without_finite':
        assert p['lo'][1] == 0.0 and p['lo'][2] == 0.0
        assert p['clamped'] == 80                                        # every y and z value
        cz = (p['key'] >> np.uint64(42)).astype(np.int64)
        assert set(cz[::2].tolist()) == {(1 << 21) - 1} and set(cz[1::2].tolist()) == {0}
        assert ((p['key'] >> np.uint64(21)) & np.uint64((1 << 21) - 1)).max() == 0
    if name == 'specials':
        cx = (p['key'] & np.uint64((1 << 21) - 1)).astype(np.int64)
        assert cx[0] == 0 and cx[1] == (1 << 21) - 1 and cx[2] == 0 and cx[3] == (1 << 21) - 1
        assert p['row_clamped'][:8].tolist() == [1] * 8 and p['clamped'] == 40  # x of rows 0-3, y of rows 4-7
    if name == 'one_point':
        assert np.array_equal(p['order'], np.arange(700)) and len(p['centres']) == 3
        assert p['centres'].tolist() == [[5.0, 1.5, 11.5]] * 3


# ---- round trip ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('C,degree', [(0, -1), (3, -1), (8, -1), (15, -1), (15, 1), (8, 0)])
def test_round_trip_through_the_readers(mode, C, degree):
    cols = kc.image_table(515, C, seed=31)
    t = dict(cols)
    image, clamped = ref.image(cols, mode, degree, 5.0, -1.25, 1.75)
    assert clamped == 0
    Cout = C if degree < 0 else ref.COEFFS[degree]
    assert sh.ksplat_layout(image) == (515, 3 * Cout)
    out, n, nsh = oracle_readers.read_ksplat(image)
    assert (n, nsh) == (515, 3 * Cout)
    p = ref.plan(cols, 5.0)
    order = p['order'].astype(np.int64)
    lo, hi = (-1.25, 1.75) if mode == 2 else (-1.5, 1.5)
    with np.errstate(all='ignore'):
        for a, k in enumerate('xyz'):
            src = t[k][order].astype(np.float64)
            got = out[a].astype(np.float64)
            if mode == 0:
                assert np.array_equal(out[a].view(np.uint32), t[k][order].view(np.uint32))
            else:
                c = np.abs(p['centres'][p['bucket'], a].astype(np.float64))
                ps = 5.0 / 2 / 32767
                assert (np.abs(got - src) <= ps / 2 + c * 2.0 ** -23 + np.abs(got) * 2.0 ** -23).all()
                code = ref.centre_code(src, p['centres'][p['bucket'], a].astype(np.float64), ps, 32767.0)
                assert np.array_equal(out[a], ref.centre_decode(code.astype(np.float64), 32767.0, ps,
                                                                p['centres'][p['bucket'], a].astype(np.float64)).astype(np.float32))
        u = ref.unit_quat({f'rot_{k}': t[f'rot_{k}'][order] for k in range(4)})
        for k in range(3):
            e = ot.exp(t[f'scale_{k}'][order].astype(np.float64))
            stored = ref.fround(e) if mode == 0 else kc.half_value(ref.half_bits(e))
            assert np.array_equal(out[3 + k].view(np.uint32), oracle_readers._ks_scale(stored).astype(np.uint32))
            byte = ref.q8((t[f'f_dc_{k}'][order].astype(np.float64) * ref.SH_C0 + 0.5) * 255.0)
            assert np.array_equal(out[6 + k], ((byte / 255.0 - 0.5) / ref.SH_C0).astype(np.float32))
        for k in range(4):
            stored = ref.fround(u[k]) if mode == 0 else kc.half_value(ref.half_bits(u[k]))
            assert np.array_equal(out[10 + k], stored.astype(np.float32))
        for ch in range(3):
            for j in range(Cout):
                src = t[f'f_rest_{ch * C + j}'][order]
                got = out[14 + ch * Cout + j]
                if mode == 0:
                    assert np.array_equal(got.view(np.uint32), src.view(np.uint32))
                elif mode == 1:
                    assert np.array_equal(got, kc.half_value(ref.half_bits(src.astype(np.float64))).astype(np.float32))
                else:
                    code = ref.sh8_code(src.astype(np.float64), lo, hi).astype(np.float64)
                    assert np.array_equal(got, ref.sh8_decode(code, lo, hi - lo).astype(np.float32))


# ---- the stand-alone program ---------------------------------------------------------------------------
_HARNESS = {}
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SANITIZE = ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined']


def _harness(sanitize):
    if not _HARNESS:
        d = tempfile.mkdtemp(prefix='st_ksplat_write_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = os.path.join(ROOT, 'tests', 'native', 'ksplat_write_cpu_check.cpp')
        for key, extra in ((False, []), (True, SANITIZE)):
            exe = os.path.join(d, 'ksplat_write_cpu_check' + ('_san' if key else ''))
            subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-ffp-contract=off', *extra, '-o',
                                   exe, src])
            _HARNESS[key] = exe
    return _HARNESS[sanitize]


def native(cols, mode, degree, sh_min, sh_max, block, quant, grid, tmp_path, public, sanitize):
    """(header bytes, records, per-row cells) of the product's host functions, or the 'ERR ...' line"""
    cols = list(cols.items()) if isinstance(cols, dict) else list(cols)
    n = len(cols[0][1]) if cols else 0
    src, gsrc, dst = tmp_path / 'table.bin', tmp_path / 'grid.bin', tmp_path / 'out.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<QII', n, len(cols), 0))
        for k, a in cols:
            f.write(struct.pack('<I28s', NP_TO_PLY[np.asarray(a).dtype], k.encode()))
        for _, a in cols:
            f.write(np.ascontiguousarray(a).tobytes())
    order, bucket, centres, F, P, lo = grid
    with open(gsrc, 'wb') as f:
        f.write(struct.pack('<QQQQddd', len(order), len(centres), F, P, *lo))
        f.write(np.asarray(order, '<u4').tobytes() + np.asarray(bucket, '<u4').tobytes())
        f.write(np.asarray(centres, '<f4').tobytes())
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1', UBSAN_OPTIONS='halt_on_error=1')
    r = subprocess.run([_harness(sanitize), str(mode), str(degree), repr(float(sh_min)), repr(float(sh_max)),
                        repr(float(block)), str(quant), str(src), str(gsrc), str(dst), '1' if public else '0'],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    words = r.stdout.split()
    if words[0] != 'OK':
        return r.stdout.strip()
    Cout = int(words[2])
    raw = dst.read_bytes()
    stride = ref.stride(mode, Cout)
    nrec = len(order)
    rec = np.frombuffer(raw, np.uint8, nrec * stride, 5120).reshape(nrec, stride)
    cells = np.frombuffer(raw, np.uint8, n * 24, 5120 + nrec * stride).reshape(n, 24)
    return raw[:5120], rec, cells


def check_native_public(cols, mode, degree, block, sh_min, sh_max, tmp_path):
    """the product's host functions against the restatement on the public writer's own grid"""
    t = ref.table(cols)
    C, Cout, B, lo, hi = ref.check_params(t, mode, degree, block, sh_min, sh_max)
    p = ref.plan(cols, B)
    grid = (p['order'], p['bucket'], p['centres'], p['full'], p['partial'], p['lo'])
    want = ref.records(cols, mode, p['order'], p['bucket'], p['centres'], degree, B, 32767, lo, hi)
    for sanitize in (False, True):
        head, rec, cells = native(cols, mode, degree, sh_min, sh_max, B, 32767, grid, tmp_path, True, sanitize)
        assert head == ref.headers(len(t['x']), mode, Cout, B, lo, hi, p['full'], p['partial'])
        assert np.array_equal(rec, want), np.argwhere(rec != want)[:5]
        assert np.array_equal(np.ascontiguousarray(cells[:, 0:8]).view('<u8')[:, 0], p['key'])
        assert np.array_equal(np.ascontiguousarray(cells[:, 8:12]).view('<u4')[:, 0], p['row_clamped'])
        cell_centres = np.ascontiguousarray(cells[:, 12:24]).view('<f4')
        assert np.array_equal(cell_centres[p['order']].view(np.uint32), p['centres'][p['bucket']].view(np.uint32))


SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30]


def specials_table(dtype):
    names = sh.reader_columns(9)
    cols = dict(kc.ordinary(np.random.default_rng(7), 7 * len(names), 3, dtype))
    for j, k in enumerate(names):
        cols[k][7 * j:7 * j + 7] = np.array(SPECIALS, np.float64).astype(dtype)
    return [(k, cols[k]) for k in names]


def boundaries_table():
    """float64 columns on and beside the rounding boundaries of every quantised field"""
    n = 1024
    cols = dict(kc.ordinary(np.random.default_rng(8), n, 15, np.float64))
    k = np.arange(n, dtype=np.float64)
    ps = 5.0 / 2 / 32767
    cols['x'] = 2.5 + (k - 512 + 0.5) * ps                      # centre-code ties in the first cell (lo = 0 below)
    cols['x'][0] = 0.0
    cols['y'] = np.nextafter(cols['x'], -np.inf)
    cols['z'] = np.r_[0.0, 5.0, np.nextafter(5.0, 0), 4.99999, 10.0, 1e7, 5.0 * (1 << 21), np.nextafter(5.0 * (1 << 21), 0),
                      1e300, np.resize([0.3, 7.7, 12.1], n - 9)]  # cell boundaries and the last cell
    h = kc.half_value(np.arange(0x3800, 0x3800 + n).astype(np.uint16))
    cols['scale_0'] = np.log((h + kc.half_value((np.arange(0x3800, 0x3800 + n) + 1).astype(np.uint16))) / 2)
    cols['f_rest_0'] = -1.5 + ((k % 256) + 0.5) / 255 * 3.0     # mode 2 ties
    cols['f_rest_44'] = np.nextafter(cols['f_rest_0'], -np.inf)
    cols['f_rest_7'] = (h + np.nextafter(h, 1)) / 2 * 0 + (h + kc.half_value((np.arange(0x3800, 0x3800 + n) + 1).astype(np.uint16))) / 2
    cols['f_dc_0'] = (((k % 256) + 0.5) / 255 - 0.5) / ref.SH_C0
    cols['opacity'] = (k - 512) / 16
    return [(kk, cols[kk]) for kk in sh.reader_columns(45)]


def mixed_types_table():
    rng = np.random.default_rng(10)
    n = 600
    cols = [('nx', rng.normal(0, 1, n).astype(np.float32)),
            ('x', rng.normal(0, 30, n)), ('y', rng.integers(-3000, 3000, n).astype(np.int32)),
            ('z', rng.integers(-128, 128, n).astype(np.int8)), ('x', np.full(n, 99.0, np.float32)),
            ('scale_0', rng.integers(-12, 8, n).astype(np.int16)), ('scale_1', rng.normal(-4, 2, n).astype(np.float32)),
            ('scale_2', rng.integers(0, 7, n).astype(np.uint8)),
            ('f_dc_0', rng.normal(0, 1, n)), ('f_dc_1', rng.integers(0, 3, n).astype(np.uint16)),
            ('f_dc_2', rng.integers(0, 3, n).astype(np.uint32)), ('opacity', rng.integers(-9, 9, n).astype(np.int32)),
            ('rot_0', rng.integers(-5, 5, n).astype(np.int8)), ('rot_1', rng.normal(0, 1, n)),
            ('rot_2', rng.integers(0, 5, n).astype(np.uint8)), ('rot_3', rng.normal(0, 1, n).astype(np.float32))]
    cols += [(f'f_rest_{i}', rng.normal(0, 0.4, n).astype(np.float32 if i % 2 else np.float64)) for i in range(24)]
    cols += [('f_rest_30', np.zeros(n, np.float32))]
    return cols


DIRECTED = {'specials_f32': lambda: specials_table(np.float32), 'specials_f64': lambda: specials_table(np.float64),
            'boundaries': boundaries_table, 'mixed_types': mixed_types_table}


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('name', list(DIRECTED))
def test_host_encode_matches_restatement_on_directed_tables(name, mode, tmp_path):
    cols = DIRECTED[name]()
    check_native_public(cols, mode, -1, 5.0, -1.5, 1.5, tmp_path)
    if name == 'boundaries':
        check_native_public(cols, mode, 1, 1.25, -0.75, 2.0, tmp_path)


@pytest.mark.parametrize('set_name,name', kc.KSPLAT_CASES, ids=[n for _, n in kc.KSPLAT_CASES])
def test_host_encode_matches_restatement_on_fixture_columns(set_name, name, tmp_path):
    """the fixture columns through the file's own grid: any block size, range and centre table"""
    data, cols, _ = kc.fixture(set_name, name)
    for sec in kc.sections(data, cols):
        want = kc.restated(sec)
        grid = (np.arange(len(want)), sec['bucket'], sec['centres'], 0, 0, (0.0, 0.0, 0.0))
        finite = np.isfinite(sec['sh_min']) and np.isfinite(sec['sh_max']) and sec['sh_min'] < sec['sh_max']
        lo, hi = (sec['sh_min'], sec['sh_max']) if finite else (-1.5, 1.5)
        if sec['mode'] == 2 and not finite:
            continue  # a range the writer refuses (its harmonics are the class sh_range)
        for sanitize in (False, True):
            _, rec, _ = native(sec['table'], sec['mode'], -1, lo, hi, sec['block'], sec['quant'], grid, tmp_path, False,
                               sanitize)
            assert np.array_equal(rec, want), (name, np.argwhere(rec != want)[:5])


# ---- arguments -----------------------------------------------------------------------------------------
def test_argument_errors_name_the_parameter(tmp_path):
    cols = kc.image_table(20, 3)
    p = ref.plan(cols, 5.0)
    grid = (p['order'], p['bucket'], p['centres'], p['full'], p['partial'], p['lo'])

    def run(cols=cols, mode=1, degree=-1, lo=-1.5, hi=1.5, block=5.0, grid=grid):
        return native(cols, mode, degree, lo, hi, block, 32767, grid, tmp_path, True, False)
    A, U = sh.ST_ERR_ARG, sh.ST_ERR_UNSUPPORTED
    assert U != A
    for kw, word in ((dict(mode=3), 'mode'), (dict(mode=-1), 'mode'), (dict(degree=2), 'degree'), (dict(degree=4), 'degree'),
                     (dict(degree=-2), 'degree'), (dict(block=0.0), 'block_size'), (dict(block=-1.0), 'block_size'),
                     (dict(block=float('inf')), 'block_size'), (dict(block=float('nan')), 'block_size'),
                     (dict(block=1e-60), 'block_size'), (dict(block=1e60), 'block_size'),
                     (dict(mode=2, lo=0.0), 'sh_min'), (dict(mode=2, hi=0.0), 'sh_max'), (dict(mode=2, lo=2.0), 'sh_min'),
                     (dict(mode=2, lo=float('nan')), 'sh_min'), (dict(mode=2, hi=float('inf')), 'sh_max'),
                     (dict(cols=[c for c in cols if c[0] != 'rot_2']), 'rot_2')):
        got = run(**kw)
        assert isinstance(got, str) and got.startswith(f'ERR {A} ') and word in got, (kw, got)
        with pytest.raises((ValueError, KeyError)):
            ref.image(kw.get('cols', cols), kw.get('mode', 1), kw.get('degree', -1), kw.get('block', 5.0),
                      kw.get('lo', -1.5), kw.get('hi', 1.5))
    empty = [(k, a[:0]) for k, a in cols]
    got = run(cols=empty, grid=(p['order'][:0], p['bucket'][:0], p['centres'], 0, 0, p['lo']))
    assert isinstance(got, str) and got.startswith(f'ERR {A} ') and 'no rows' in got
    # the refused range is not consulted outside mode 2, as the rules say
    assert not isinstance(run(mode=1, lo=0.0, hi=0.0), str)


def test_image_size():
    assert sh.ksplat_image_size(1, 0, 0, 0, 1) == 5120 + 4 + 12 + 44
    assert sh.ksplat_image_size(513, 15, 1, 2, 1) == 5120 + 4 + 36 + 513 * 114
    assert sh.ksplat_image_size(513, 8, 2, 1, 3) == 5120 + 12 + 48 + 513 * 48
    assert [ref.stride(m, c) for m in range(3) for c in ref.COEFFS] == [44, 80, 140, 224, 24, 42, 72, 114, 24, 33, 48, 69]
    for bad in ((0, 0, 0, 0, 0), (1 << 32, 0, 0, 0, 0), (10, 4, 0, 0, 1), (10, 0, 3, 0, 1), (10, 0, -1, 0, 1),
                (10, 0, 0, 11, 0)):
        assert sh.ksplat_image_size(*bad) == 0
    for n, C, mode in ((1, 0, 0), (300, 3, 1), (515, 15, 2)):
        image, _ = ref.image(kc.image_table(n, C), mode)
        p = ref.plan(kc.image_table(n, C))
        assert len(image) == sh.ksplat_image_size(n, C, mode, p['full'], p['partial'])
