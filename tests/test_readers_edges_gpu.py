"""The .splat / .ksplat / .spz readers on the GPU where a decode out of staged LDS can go wrong:
plane and record offsets that are 1, 2 and 3 mod 4, file lengths that are no multiple of 4, last
tiles of one to three rows, sections that start mid-tile, twenty partial buckets over three tiles.

  * every case of tests/golden/readers_edges.* (the reference's own readers) through every form
  * guard rows around the output columns of the decode-from-HBM forms
  * seeded random files, built here, against the CPU restatement (oracle/readers.py, itself pinned
    to both fixture sets by test_readers_oracle_cpu.py); every half pattern and every byte value

Every comparison is bit for bit.
"""
import functools
import gzip
import struct

import numpy as np
import pytest

import readers as oracle_readers
import splat_hip as sh
from golden_io import Golden
from readers_files import KS_BASE, KS_COLOUR, SH_COUNT, ksplat_file, ksplat_section, ksplat_sections, spz_planes, spz_raw
from test_ply_cpu import same

pytestmark = pytest.mark.gpu

G = Golden('readers_edges')
CASES = {c['name']: c for c in G.meta['cases']}
SENTINEL = struct.unpack('<f', bytes.fromhex('a5c3965a'))[0]  # 0x5a96c3a5: no decode writes it
GUARD = 32


@pytest.fixture(scope='module')
def ctx():
    import torch  # noqa: F401
    c = sh.Context(0)
    yield c
    c.close()


def check_columns(got, want, what):
    assert list(got) == list(want), what
    for k, w in want.items():
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k)
        if not same(g, w):
            i = int(np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))[0])
            raise AssertionError(f'{what}: {k}[{i}] = {g.view(np.uint32)[i]:#010x}, expected '
                                 f'{w.view(np.uint32)[i]:#010x}')


def named(cols, nsh):
    return dict(zip(sh.reader_columns(nsh), cols))


def device_bytes(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


class Guarded:
    """output columns that are rows [32, 32 + n) of tensors of n + 64 rows full of a sentinel"""

    def __init__(self, nsh, n):
        import torch
        self.n = n
        self.whole = {k: torch.full((n + 2 * GUARD,), SENTINEL, device='cuda') for k in sh.reader_columns(nsh)}
        self.out = {k: t[GUARD:GUARD + n] for k, t in self.whole.items()}
        torch.cuda.synchronize()  # the fills run on torch's stream, the decode on the context's

    def check(self, want, what):
        check_columns(self.out, want, what)
        bits = np.float32(SENTINEL).view(np.uint32)
        for k, t in self.whole.items():
            g = t.cpu().numpy().view(np.uint32)
            guard = np.concatenate([g[:GUARD], g[GUARD + self.n:]])
            assert len(guard) == 2 * GUARD and (guard == bits).all(), f'{what}: {k} written outside its {self.n} rows'


def decode_from_hbm(ctx, fmt, data, want, n, nsh, what):
    """st_dev_<fmt>_decode into guarded columns; .ksplat once with the whole file on the host and once
    with the headers alone (data: the file's bytes, for .spz inflated)"""
    if fmt == 'splat':
        runs = [('', lambda out: ctx.dev_splat_decode(device_bytes(data), out))]
    elif fmt == 'spz':
        runs = [('', lambda out: ctx.dev_spz_decode(device_bytes(data), out))]
    else:
        headers = 4096 + 1024 * int.from_bytes(data[4:8], 'little')
        runs = [(f' with {len(h)} host bytes', lambda out, h=h: ctx.dev_ksplat_decode(h, device_bytes(data), out))
                for h in (data, data[:headers])]
    for tag, run in runs:
        g = Guarded(nsh, n)
        run(g.out)
        ctx.synchronize()
        g.check(want, what + tag)


def every_form(ctx, tmp_path, fmt, disk, want, n, nsh, what):
    """read_<fmt>, read_<fmt>_dev, read_table and the decode from HBM of one file (disk: its bytes as
    they lie on disk)"""
    path = tmp_path / f'f.{fmt}'
    path.write_bytes(disk)
    path = str(path)
    check_columns(getattr(ctx, f'read_{fmt}')(path), want, f'{what} host columns')
    dev = getattr(ctx, f'read_{fmt}_dev')(path)
    ctx.synchronize()
    check_columns(dev, want, f'{what} device columns')
    check_columns(ctx.read_table(path), want, f'{what} read_table')
    decode_from_hbm(ctx, fmt, sh.spz_inflate(disk) if fmt == 'spz' else disk, want, n, nsh, f'{what} decode')


# ---- 1. the fixtures through every form; 2. guard rows (every decode from HBM here is guarded) -----
@pytest.mark.parametrize('name', list(CASES))
def test_edge_case_matches_reference_in_every_form(ctx, tmp_path, name):
    c = CASES[name]
    want = G[name + '_cols']
    assert want.shape == (14 + c['nsh'], c['n'])
    every_form(ctx, tmp_path, c['format'], G[name + '_file'].tobytes(), dict(zip(c['columns'], want)), c['n'], c['nsh'], name)


def test_guard_rows_cover_every_format():
    """the guarded decodes above include .spz at n = 257 and .ksplat at 129 records; .splat has its
    own guarded decode in test_random_splat"""
    assert any(c['format'] == 'spz' and c['n'] == 257 for c in CASES.values())
    assert any(c['format'] == 'ksplat' and c['n'] == 129 for c in CASES.values())


# ---- 3. seeded random files against the restatement -------------------------------------------------
def restated(fmt, data):
    """(columns by name, n, nsh) of the restatement"""
    cols, n, nsh = getattr(oracle_readers, f'read_{fmt}')(data)
    return named(cols, nsh), n, nsh


SPZ_ROWS = (1, 2, 3, 255, 256, 257, 511, 513, 514, 515, 4099)
SPZ_FB = (0, 12, 23, 31)


@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('version', [2, 3])
def test_random_spz(ctx, tmp_path, version, degree):
    rng = np.random.default_rng(7000 + 10 * version + degree)
    skews = set()
    for i, n in enumerate(SPZ_ROWS):
        if version == 3 and n == 1:
            continue  # (the reference rejects it: a 4-byte read in a 3-byte rotation plane)
        fb = SPZ_FB[(i + degree + version) % 4]
        raw = spz_raw(rng, version, n, degree, fb)
        want, rows, nsh = restated('spz', raw)
        assert (rows, nsh) == (n, SH_COUNT[degree])
        off = spz_planes(raw)[0]
        skews |= {(p, off[p] % 4) for p in off}
        what = f'spz v{version} degree {degree} n {n} fb {fb}'
        if n in (3, 257, 4099):
            every_form(ctx, tmp_path, 'spz', gzip.compress(raw, 1), want, n, nsh, what)
        else:
            decode_from_hbm(ctx, 'spz', raw, want, n, nsh, what)
    assert {(p, k) for p in ('alpha', 'scale', 'sh') for k in (1, 2, 3)} <= skews and ('colour', 2) in skews


def test_spz_every_byte_value(ctx):
    """259 rows whose plane bytes are (row + 17 * column) mod 256: every byte value in every
    byte-typed field (alpha, colour, scale, version-2 rotation, SH), and in the position bytes"""
    n = 259
    for version in (2, 3):
        raw = bytearray(spz_raw(np.random.default_rng(1), version, n, 3, 12))
        off, _, nsh, _ = spz_planes(raw)
        for plane, width in (('pos', 9), ('alpha', 1), ('colour', 3), ('scale', 3), ('rot', 3), ('sh', nsh)):
            b = (np.arange(n)[:, None] + 17 * np.arange(width)[None, :] + len(plane)) % 256
            assert all(len(set(col)) == 256 for col in b.T)
            raw[off[plane]:off[plane] + n * width] = b.astype(np.uint8).tobytes()
        raw = bytes(raw)
        want, rows, nsh = restated('spz', raw)
        decode_from_hbm(ctx, 'spz', raw, want, rows, nsh, f'spz v{version} every byte')


KS_COUNTS = (1, 127, 128, 129, 257, 1000)


def random_ksplat(rng, mode, degree, i, count):
    """one section of random record bytes; i picks the storage size and the shape of the partial
    sizes: short of the partial splats, beyond them, or as drawn (more entries than splats at
    count 1)"""
    capacity = 16
    full = min(int(rng.integers(0, 4)), (count - 1) // capacity)
    partial_splats = count - full * capacity
    sizes = [int(v) if rng.random() > 0.3 else 0 for v in rng.integers(1, 2 + partial_splats // 4, int(rng.integers(1, 30)))]
    if (i + 1) % 3 == 0:
        while sizes and sum(sizes) >= partial_splats:
            sizes.pop()
    elif (i + 1) % 3 == 1:
        sizes.append(partial_splats + 5)
    s = ksplat_section(rng, mode, degree, count, count + i % 3, storage=12 + (i + mode + degree) % 4, partial=sizes,
                       capacity=capacity, full=full, buckets=full + len(sizes) + i % 2)
    return ksplat_file(mode, [s], min_h=float(rng.uniform(-3, -1)), max_h=float(rng.uniform(1, 3)))


@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_random_ksplat(ctx, tmp_path, mode, degree):
    rng = np.random.default_rng(8000 + 10 * mode + degree)
    for i, count in enumerate(KS_COUNTS):
        data = random_ksplat(rng, mode, degree, i, count)
        want, n, nsh = restated('ksplat', data)
        assert (n, nsh) == (count, SH_COUNT[degree])
        s = ksplat_sections(data)[1][0]
        what = f'ksplat mode {mode} degree {degree} count {count} storage {s["storage"]} data_off % 4 = {s["data_off"] % 4}'
        if count in (129, 1000):
            every_form(ctx, tmp_path, 'ksplat', data, want, n, nsh, what)
        else:
            decode_from_hbm(ctx, 'ksplat', data, want, n, nsh, what)


def test_random_ksplat_storage_sizes_cover_every_record_offset():
    """(no GPU work: what test_random_ksplat's files are) storage sizes 12..15 all occur, and the
    records of every mode start at every offset mod 4"""
    storage, residues = set(), {m: set() for m in (0, 1, 2)}
    for mode in (0, 1, 2):
        for degree in (0, 1, 2, 3):
            rng = np.random.default_rng(8000 + 10 * mode + degree)
            for i, count in enumerate(KS_COUNTS):
                s = ksplat_sections(random_ksplat(rng, mode, degree, i, count))[1][0]
                storage.add(s['storage'])
                residues[mode].add(s['data_off'] % 4)
    assert storage == {12, 13, 14, 15}
    assert all(r == {0, 1, 2, 3} for r in residues.values()), residues


def test_ksplat_three_sections_two_of_them_unaligned(ctx, tmp_path):
    """storage sizes 13 and 14 put the records of sections 0 and 1 at offsets 3 and 2 mod 4; their
    record counts bring the next section back to a multiple of 4 (the reader needs that for its
    typed arrays)"""
    rng = np.random.default_rng(8100)
    mode = 2
    plan = [dict(degree=1, count=130, storage=13, buckets=3, partial=[20, 0, 300]),
            dict(degree=1, count=200, storage=14, buckets=5, partial=[7, 0, 0, 90, 100]),
            dict(degree=2, count=131, storage=12, buckets=4, partial=[1, 2])]
    sections = []
    for p in plan:
        stride = KS_BASE[mode] + SH_COUNT[p['degree']]
        meta = 4 * len(p['partial']) + p['storage'] * p['buckets']
        max_splats = next(m for m in range(p['count'], p['count'] + 4) if (meta + stride * m) % 4 == 0)
        sections.append(ksplat_section(rng, mode, p['degree'], p['count'], max_splats, storage=p['storage'],
                                       partial=p['partial'], capacity=8, full=2, buckets=p['buckets']))
    data = ksplat_file(mode, sections, min_h=-2.0, max_h=0.75)
    _, lay = ksplat_sections(data)
    assert [s['start'] % 4 for s in lay] == [0, 0, 0] and [s['data_off'] % 4 for s in lay] == [3, 2, 0]
    want, n, nsh = restated('ksplat', data)
    assert (n, nsh) == (461, 24)
    every_form(ctx, tmp_path, 'ksplat', data, want, n, nsh, 'three sections')


@functools.lru_cache(None)
def half_file():
    """mode 1, degree 2, 21,846 records: the three scale slots enumerate every half pattern once
    (they go through Math.log), the 28 rotation and SH slots do so nine times over"""
    n = 21846
    rng = np.random.default_rng(8200)
    rec = rng.integers(0, 256, (n, 72), dtype=np.uint8)
    halves = rec.view('<u2')  # [n, 36]: 3 positions, 3 scales, 4 rotations, 2 colour words, 24 harmonics
    r = np.arange(n)[:, None]
    halves[:, 3:6] = (3 * r + np.arange(3)) % 65536
    other = (28 * r + np.arange(28)) % 65536
    halves[:, 6:10] = other[:, :4]
    halves[:, 12:36] = other[:, 4:]
    assert len(set(halves[:, 3:6].ravel())) == 65536
    assert len(set(np.concatenate([halves[:, 6:10], halves[:, 12:36]], 1).ravel())) == 65536
    s = ksplat_section(rng, 1, 2, n, n, storage=14, partial=[100, 0, 50], capacity=256, full=80, buckets=85, records=rec)
    data = ksplat_file(1, [s])
    return data, restated('ksplat', data)


def test_ksplat_every_half_pattern(ctx):
    data, (want, n, nsh) = half_file()
    assert ksplat_sections(data)[1][0]['data_off'] % 4 == 2
    decode_from_hbm(ctx, 'ksplat', data, want, n, nsh, 'every half pattern')


def test_ksplat_every_byte_value(ctx):
    """mode 2, degree 3, 259 records: every byte value in the colour, opacity and harmonics bytes"""
    n = 259
    rng = np.random.default_rng(8300)
    rec = rng.integers(0, 256, (n, KS_BASE[2] + 45), dtype=np.uint8)
    fields = list(range(KS_COLOUR[2], KS_COLOUR[2] + 4)) + list(range(KS_BASE[2], KS_BASE[2] + 45))
    for j, f in enumerate(fields):
        rec[:, f] = (np.arange(n) + 29 * j) % 256
        assert len(set(rec[:, f])) == 256
    s = ksplat_section(rng, 2, 3, n, n, storage=13, partial=[70, 0, 60, 100], capacity=16, full=2, buckets=7, records=rec)
    data = ksplat_file(2, [s], min_h=-1.75, max_h=2.25)
    want, rows, nsh = restated('ksplat', data)
    decode_from_hbm(ctx, 'ksplat', data, want, rows, nsh, 'every byte value')


@functools.lru_cache(None)
def splat_file():
    """4,099 rows of random 32-bit words: arbitrary f32 patterns in positions and scales"""
    data = np.random.default_rng(9000).integers(0, 1 << 32, 4099 * 8, dtype=np.uint64).astype('<u4').tobytes()
    return data, restated('splat', data)


def test_random_splat(ctx, tmp_path):
    data, (want, n, nsh) = splat_file()
    assert (n, nsh) == (4099, 0)
    every_form(ctx, tmp_path, 'splat', data, want, n, nsh, 'splat 4099 random rows')


def test_random_splat_one_block_per_chunk(ctx, tmp_path, monkeypatch):
    """the same file through pinned chunks of 8192 bytes: one 256-row block each, seventeen of them"""
    data, (want, n, _) = splat_file()
    p = tmp_path / 'chunks.splat'
    p.write_bytes(data)
    monkeypatch.setenv('ST_PLY_CHUNK', '8192')
    check_columns(ctx.read_splat(str(p)), want, 'host columns')
    dev = ctx.read_splat_dev(str(p))
    ctx.synchronize()
    check_columns(dev, want, 'device columns')
