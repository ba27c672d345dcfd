"""The .splat / .spz writers on the GPU (k_splat_rows, k_spz_planes, the image and file forms, the
one-call chain forms) against the numpy restatement of the encode rules
(tests/write_splat_spz_ref.py), byte for byte, and the reference's fixture files under the
conditions of tests/test_write_splat_spz_cpu.py."""
import gzip
import os

import numpy as np
import pytest
import torch

import oracle_typed as ot
import readers as oracle_readers
import splat_hip as sh
import write_ply_ref
import write_splat_spz_ref as ref
from test_write_ply_gpu import CHAINS, to_dev
from test_write_splat_spz_cpu import (SPLAT_CASES, SPZ_CASES, check_splat_against_file, check_spz_against_file,
                                      directed_tables, first_difference, fixture, ordinary)

pytestmark = pytest.mark.gpu

GUARD = 32
FILL = 0xA5
COEFFS = [0, 3, 8, 15]
PER_SPLAT = [9, 1, 3, 3, 3]


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def guarded(nbytes, offset=0):
    """(buffer of FILL, the view of nbytes at GUARD + offset inside it): sentinels on either side"""
    buf = torch.full((GUARD + offset + nbytes + GUARD + 4,), FILL, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(buf, offset, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:GUARD + offset] == FILL).all() and (host[GUARD + offset + nbytes:] == FILL).all())


def spz_image_check(ctx, cols, fb, offset=0):
    want, want_clamped = ref.spz_image(cols, fb)
    buf, view = guarded(len(want), offset)
    size, clamped = ctx.dev_spz_image(to_dev(cols), view, fb)
    assert size == len(want) == sh.spz_image_size(len(cols[0][1]), ot.band_coeffs({k for k, _ in cols}))
    assert first_difference(view.cpu().numpy().tobytes(), want) is None
    assert guards_intact(buf, offset, len(want))
    assert clamped == want_clamped
    return clamped


def splat_rows_check(ctx, cols, dev, row0, nrows, offset=0):
    want = ref.splat_rows([(k, a[row0:row0 + nrows]) for k, a in cols]).tobytes()
    buf, view = guarded(len(want), offset)
    ctx.dev_splat_rows(dev, view, row0, nrows)
    assert first_difference(view.cpu().numpy().tobytes(), want) is None, (row0, nrows, offset)
    assert guards_intact(buf, offset, len(want))


# ---- the kernels against the restatement ----------------------------------------------------------
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 255, 256, 257, 258, 259, 513])
def test_dev_spz_image_matches_restatement(ctx, n, degree):
    """whole images: these sizes put every plane start and the image end at each offset modulo 4
    and leave a last tile of 1-3 rows"""
    cols = ordinary(np.random.default_rng(100 * n + degree), n, COEFFS[degree])
    assert spz_image_check(ctx, cols, 12) == 0
    if n in (259, 513):   # the image itself at an odd address; positions past the range counted over three tiles
        assert spz_image_check(ctx, cols, 23, offset=1 + degree % 3) > n


@pytest.mark.parametrize('degree', [1, 3])
@pytest.mark.parametrize('row0', [3, 256, 257])
def test_dev_spz_planes_from_inside_the_table(ctx, row0, degree):
    """each plane in a guarded buffer of its own at byte offsets 0-3, from a row inside the table"""
    n, C = 513, COEFFS[degree]
    cols = ordinary(np.random.default_rng(row0 + degree), n, C)
    planes, _ = ref.spz_planes(cols, 12)
    _, want_clamped = ref.spz_planes([(k, a[row0:]) for k, a in cols], 20)
    dev = to_dev(cols)
    for shift in range(4):
        bufs = [guarded((n - row0) * w, (shift + p) % 4) for p, w in enumerate(PER_SPLAT + [3 * C])]
        clamped = ctx.dev_spz_planes(dev, [v for _, v in bufs], 12, row0)
        assert clamped == 0
        for p, name in enumerate(ref.PLANES):
            want = planes[name][row0:].tobytes()
            assert first_difference(bufs[p][1].cpu().numpy().tobytes(), want) is None, (name, shift)
            assert guards_intact(bufs[p][0], (shift + p) % 4, len(want)), (name, shift)
    # a skipped plane is not written, the others are, and the count does not depend on it
    bufs = [guarded((n - row0) * w) for w in PER_SPLAT + [3 * C]]
    clamped = ctx.dev_spz_planes(dev, [None if p in (0, 5) else v for p, (_, v) in enumerate(bufs)], 20, row0)
    assert clamped == want_clamped > 0
    for p, name in enumerate(ref.PLANES):
        got = bufs[p][1].cpu().numpy()
        if p in (0, 5):
            assert (got == FILL).all()
        else:
            assert first_difference(got.tobytes(), planes[name][row0:].tobytes()) is None, name


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1025])
def test_dev_splat_rows_matches_restatement(ctx, n):
    cols = ordinary(np.random.default_rng(n), n, 0)
    dev = to_dev(cols)
    splat_rows_check(ctx, cols, dev, 0, n)
    splat_rows_check(ctx, cols, dev, 0, n, offset=4)    # 4-byte aligned only: the eight-word stores
    if n > 3:
        splat_rows_check(ctx, cols, dev, 3, n - 3)
        splat_rows_check(ctx, cols, dev, 3, n - 3, offset=8)
        splat_rows_check(ctx, cols, dev, n - 1, 1)


@pytest.mark.parametrize('name', list(directed_tables()))
def test_directed_tables(ctx, name):
    """the specials, the rounding boundaries and clamp ends, the quaternion cases, and float64 /
    integer columns among the fourteen"""
    cols, fb = directed_tables()[name]
    clamped = spz_image_check(ctx, cols, fb)
    if name != 'quaternions' and name != 'mixed_types':
        assert clamped > 0
    splat_rows_check(ctx, cols, to_dev(cols), 0, len(cols[0][1]))
    if name == 'boundaries':
        for ends in (0, 23):
            spz_image_check(ctx, cols, ends)


# ---- the reference's fixtures on the device ---------------------------------------------------------
@pytest.mark.parametrize('name', SPZ_CASES)
def test_spz_fixture_read_and_written_on_the_device(ctx, tmp_path, name):
    raw, cols = fixture(name)
    src = tmp_path / 'in.spz'
    src.write_bytes(gzip.compress(raw))
    dev = ctx.read_spz_dev(str(src))
    size = sh.spz_image_size(len(cols[0][1]), (len(cols) - 14) // 3)
    buf, view = guarded(size)
    assert ctx.dev_spz_image(dev, view, raw[13]) == (len(raw), 0)
    check_spz_against_file(view.cpu().numpy().tobytes(), raw, cols)
    assert guards_intact(buf, 0, size)


@pytest.mark.parametrize('name', SPLAT_CASES)
def test_splat_fixture_read_and_written_on_the_device(ctx, tmp_path, name):
    data, cols = fixture(name)
    src = tmp_path / 'in.splat'
    src.write_bytes(data)
    dev = ctx.read_splat_dev(str(src))
    buf, view = guarded(len(data))
    ctx.dev_splat_rows(dev, view)
    check_splat_against_file(view.cpu().numpy().reshape(-1, 32), data, cols)
    assert guards_intact(buf, 0, len(data))
    out = tmp_path / 'out.splat'
    assert ctx.dev_splat_file(dev, str(out)) == len(data)
    assert out.read_bytes() == view.cpu().numpy().tobytes()


# ---- file forms -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stream_case():
    return ordinary(np.random.default_rng(50_001), 50_001, 15)


def test_splat_file_streams_through_the_ring(ctx, tmp_path, monkeypatch, stream_case):
    """50,001 rows through 1 MiB slots (32,768 rows a piece) into a longer file at a non-zero position"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols = stream_case
    want = ref.splat_rows(cols).tobytes()
    assert len(want) == 50_001 * 32 > (1 << 20)
    p = tmp_path / 'at.splat'
    p.write_bytes(b'\xee' * (len(want) + 4097))
    fd = os.open(str(p), os.O_RDWR)
    try:
        os.lseek(fd, 37, os.SEEK_SET)
        assert ctx.dev_splat_file(to_dev(cols), fd) == len(want)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want) == os.fstat(fd).st_size
    finally:
        os.close(fd)
    assert p.read_bytes() == b'\xee' * 37 + want
    h = tmp_path / 'host.splat'
    assert ctx.splat_file(cols, [], str(h)) == (50_001, len(want))
    assert h.read_bytes() == want


def test_spz_file_raw_and_gzipped(ctx, tmp_path, monkeypatch, stream_case):
    """50,001 rows at degree 3 (3.2 MB of image through 1 MiB slots), raw and as one gzip member"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols = stream_case
    want, want_clamped = ref.spz_image(cols, 12)
    dev = to_dev(cols)
    raw_path, gz_path = tmp_path / 'raw.spz', tmp_path / 'gz.spz'
    raw_path.write_bytes(b'\xee' * (len(want) + 4097))   # a longer file is cut
    assert ctx.dev_spz_file(dev, str(raw_path), gzip_level=0) == (50_001, len(want), want_clamped)
    assert first_difference(raw_path.read_bytes(), want) is None
    fd = os.open(str(gz_path), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.write(fd, b'P' * 5 + b'\xee' * (len(want) + 64))
        os.lseek(fd, 5, os.SEEK_SET)
        rows, size, clamped = ctx.dev_spz_file(dev, fd)
        assert (rows, clamped) == (50_001, want_clamped)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 5 + size == os.fstat(fd).st_size
    finally:
        os.close(fd)
    member = gz_path.read_bytes()[5:]
    assert gz_path.read_bytes()[:5] == b'P' * 5 and len(member) == size < len(want)
    assert member == sh.spz_deflate(want, 6)
    assert gzip.decompress(member) == want
    # our own reader on the gzipped file against the readers' restatement on the raw bytes
    gz_path.write_bytes(member)
    got = ctx.read_spz(str(gz_path))
    back, n, nsh = oracle_readers.read_spz(want)
    assert (n, nsh) == (50_001, 45) and list(got) == sh.reader_columns(45)
    for k, w in zip(got, back):
        assert np.array_equal(got[k].view(np.uint32), w.view(np.uint32)), k
    # the host-table form
    h = tmp_path / 'host.spz'
    assert ctx.spz_file(cols, [], str(h), gzip_level=0) == (50_001, len(want), want_clamped)
    assert first_difference(h.read_bytes(), want) is None


@pytest.fixture(scope='module')
def ring_case():
    """220,753 rows of degree 0 and their .splat rows, made once: every case below is a prefix of them"""
    cols = ordinary(np.random.default_rng(220_753), 220_753, 0)
    return cols, ref.splat_rows([(k, a[:163_841]) for k, a in cols]).tobytes()


@pytest.mark.parametrize('form, n', [('splat', 32_768),    # one slot exactly: a full last piece, none after it
                                     ('splat', 32_769),    # a second piece of 32 bytes
                                     ('splat', 163_841),   # six pieces: slots 0 and 1 are taken a second time
                                     ('spz', 220_752),     # 16 + 19 n = 4 slots exactly, copied down as they are
                                     ('spz', 220_753)])    # the fifth piece takes slot 0 again
def test_file_forms_at_the_ring_slot_boundaries(ctx, tmp_path, monkeypatch, ring_case, form, n):
    """outputs that end on a 1 MiB slot boundary, one byte run past it, and more pieces than the ring
    has slots (4), into a longer file at a non-zero position"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    table, rows = ring_case
    cols = [(k, a[:n]) for k, a in table]
    if form == 'splat':
        want, result = rows[:32 * n], 32 * n
    else:
        want, want_clamped = ref.spz_image(cols, 12)
        assert len(want) == 16 + 19 * n
        result = (n, len(want), want_clamped)
    assert (len(want) % (1 << 20) == 0) == (n in (32_768, 220_752))
    p = tmp_path / f'at.{form}'
    p.write_bytes(b'\xee' * (len(want) + 4097))
    fd = os.open(str(p), os.O_RDWR)
    try:
        os.lseek(fd, 37, os.SEEK_SET)
        if form == 'splat':
            assert ctx.dev_splat_file(to_dev(cols), fd) == result
        else:
            assert ctx.dev_spz_file(to_dev(cols), fd, gzip_level=0) == result
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want) == os.fstat(fd).st_size
    finally:
        os.close(fd)
    got = p.read_bytes()
    assert got[:37] == b'\xee' * 37 and len(got) == 37 + len(want)
    assert first_difference(got[37:], want) is None


@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_file_forms_refuse_descriptor(ctx, tmp_path, flags):
    cols = ordinary(np.random.default_rng(3), 100, 3)
    dev = to_dev(cols)
    p = tmp_path / 'keep.bin'
    p.write_bytes(b'keep')
    fd = os.open(str(p), flags)
    try:
        calls = [lambda: ctx.dev_splat_file(dev, fd), lambda: ctx.splat_file(cols, [], fd),
                 lambda: ctx.dev_spz_file(dev, fd, gzip_level=0), lambda: ctx.dev_spz_file(dev, fd),
                 lambda: ctx.spz_file(cols, [], fd, gzip_level=0), lambda: ctx.spz_file(cols, [], fd)]
        for call in calls:
            with pytest.raises(sh.StError) as e:
                call()
            assert e.value.code == sh.ST_ERR_ARG
    finally:
        os.close(fd)
    assert p.read_bytes() == b'keep'


# ---- processDataTable + the writers --------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['config1', 'filters_sh3'])
def test_one_call_forms_with_actions(ctx, tmp_path, case):
    """the expectation: the restatement applied to ctx.process's table (pinned by the process_chain
    tests); from a host table and from a .ply file"""
    make, acts = CHAINS[case]
    cols = make(np.random.default_rng(len(case)))
    processed = ctx.process([(k, a.copy()) for k, a in cols], acts)
    m = len(processed[0][1])
    if case == 'filters_sh3':
        assert 0 < m < 777 and len(processed) == len(cols) - 36
    want_splat = ref.splat_rows(processed).tobytes()
    want_spz, want_clamped = ref.spz_image(processed, 12)
    assert len(want_spz) == 16 + m * (19 + (9 if case == 'filters_sh3' else 0))
    src = tmp_path / 'in.ply'
    src.write_bytes(write_ply_ref.write_ply(['the input'], [('vertex', cols)]))
    keep = [(k, a.copy()) for k, a in cols]
    a, b = tmp_path / 'a.splat', tmp_path / 'b.splat'
    assert ctx.splat_file(cols, acts, str(a)) == (m, len(want_splat))
    assert ctx.ply_splat_file(str(src), acts, str(b)) == (m, len(want_splat))
    assert a.read_bytes() == want_splat == b.read_bytes()
    a, b = tmp_path / 'a.spz', tmp_path / 'b.spz'
    assert ctx.spz_file(cols, acts, str(a), gzip_level=0) == (m, len(want_spz), want_clamped)
    rows, size, clamped = ctx.ply_spz_file(str(src), acts, str(b))
    assert (rows, clamped) == (m, want_clamped) and size == b.stat().st_size
    assert a.read_bytes() == want_spz == gzip.decompress(b.read_bytes())
    assert all(x.tobytes() == y.tobytes() for (_, x), (_, y) in zip(cols, keep))


# ---- argument errors, each of which leaves the output untouched ------------------------------------------------
def test_argument_errors_leave_the_output_untouched(ctx, tmp_path):
    cols = ordinary(np.random.default_rng(5), 100, 3)
    dev = to_dev(cols)
    size = sh.spz_image_size(100, 3)
    buf, view = guarded(4096)
    assert size < 3200
    p = tmp_path / 'keep.bin'
    p.write_bytes(b'keep')

    def refused(call, code=sh.ST_ERR_ARG, text=''):
        with pytest.raises(sh.StError) as e:
            call()
        assert e.value.code == code and text in str(e.value)
        assert int(buf.min()) == FILL == int(buf.max())
        assert p.read_bytes() == b'keep'

    for missing in ('z', 'scale_1', 'rot_3'):
        less, dless = [c for c in cols if c[0] != missing], [c for c in dev if c[0] != missing]
        text = 'missing column ' + missing
        refused(lambda: ctx.dev_spz_image(dless, view), text=text)
        refused(lambda: ctx.dev_spz_planes(dless, [view] * 6), text=text)
        refused(lambda: ctx.dev_splat_rows(dless, buf[:3200]), text=text)
        refused(lambda: ctx.dev_splat_file(dless, str(p)), text=text)
        refused(lambda: ctx.dev_spz_file(dless, str(p)), text=text)
        refused(lambda: ctx.splat_file(less, [], str(p)), text=text)
        refused(lambda: ctx.spz_file(less, [], str(p), gzip_level=0), text=text)
    for fb in (-1, 24):
        refused(lambda: ctx.dev_spz_image(dev, view, fb))
        refused(lambda: ctx.dev_spz_planes(dev, [view] * 6, fb))
        refused(lambda: ctx.dev_spz_file(dev, str(p), fb, gzip_level=0))
        refused(lambda: ctx.spz_file(cols, [], str(p), fb))
    empty = [(k, a[:0]) for k, a in cols]
    refused(lambda: ctx.dev_splat_file(to_dev(empty), str(p)))
    refused(lambda: ctx.splat_file(empty, [], str(p)))
    refused(lambda: ctx.splat_file(cols, [{'kind': 'filterByValue', 'columnName': 'x', 'comparator': 'gt', 'value': 1e9}],
                                   str(p)))
    refused(lambda: ctx.dev_spz_image(dev, view[:size - 1]))               # a cap one byte short
    refused(lambda: ctx.dev_splat_rows(dev, buf[1:3201]))                  # not 4-byte aligned
    refused(lambda: ctx.dev_splat_rows(dev, buf[:3200], 98, 3))            # rows outside the table
    refused(lambda: ctx.dev_spz_planes(dev, [view] * 6, 12, 98, 3))
    # n = 0 of .spz is the header alone
    q = tmp_path / 'empty.spz'
    assert ctx.spz_file(empty, [], str(q), gzip_level=0) == (0, 16, 0)
    assert q.read_bytes() == ref.spz_image(empty, 12)[0]
