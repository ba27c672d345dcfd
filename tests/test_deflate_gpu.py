"""DEFLATE on the device (st_deflate.hip; include/st_abi.h, "the gzip member around a .spz image"):
st_dev_deflate and st_dev_gzip give the bytes of st_deflate.h's serial encoder run on the host
(tests/native/deflate_cpu_check.cpp, checked against zlib in tests/test_deflate_cpu.py), byte for
byte, on every input of tests/deflate_cases.py, with inputs and outputs at every offset modulo 4
between sentinels; the three .spz file forms with deflate='device' write a member that inflates to
the raw form's file; and the member of a 200,000-row image is no larger than zlib level 1's."""
import gzip
import os
import zlib

import numpy as np
import pytest
import torch

import deflate_cases as dc
import readers as oracle_readers
import splat_hip as sh
import write_ply_ref
import write_splat_spz_ref as ref
from test_write_ply_gpu import to_dev
from test_write_splat_spz_cpu import SPZ_CASES, first_difference, fixture, ordinary

pytestmark = pytest.mark.gpu

GUARD = 32
FILL = 0xA5
CASES = sorted(dc.cases())
OFFSETS = [(0, 0), (1, 3), (2, 1), (3, 2)]


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def on_device(data, offset):
    """the bytes in a device tensor that starts `offset` bytes past a 256-byte boundary"""
    buf = torch.full((offset + len(data) + 8,), 0x5A, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + len(data)]
    if len(data):
        view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    return view


def guarded(nbytes, offset):
    """(buffer of FILL, the view of nbytes at GUARD + offset inside it): sentinels on either side"""
    buf = torch.full((GUARD + offset + nbytes + GUARD + 4,), FILL, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def run(call, data, want, in_off, out_off, slack=0):
    """call(input view, output view) -> size; the output view is exactly `want` + slack bytes"""
    src = on_device(data, in_off)
    buf, view = guarded(len(want) + slack, out_off)
    size = call(src, view, len(data))
    host = buf.cpu().numpy()
    got = host[GUARD + out_off:GUARD + out_off + size].tobytes()
    assert size == len(want)
    assert first_difference(got, want) is None
    assert (host[:GUARD + out_off] == FILL).all() and (host[GUARD + out_off + size:] == FILL).all()
    return got


@pytest.mark.parametrize('name', CASES)
def test_dev_deflate_gives_the_native_bytes(ctx, name, tmp_path):
    data = dc.cases()[name]
    want = dc.native_cached('stream', name, tmp_path)
    for k, (i, o) in enumerate(OFFSETS):
        # exactly the stream's size of room, then the bound's
        run(ctx.dev_deflate, data, want, i, o, slack=0 if k % 2 == 0 else sh.deflate_bound(len(data)) - len(want))
    k = CASES.index(name)
    member = dc.native_cached('gzip', name, tmp_path)
    got = run(ctx.dev_gzip, data, member, k % 4, (k // 4) % 4)
    assert gzip.decompress(got) == data


def test_every_pair_of_offsets(ctx, tmp_path):
    name = 'bytes_%d' % (dc.SEG + 1)
    data, want = dc.cases()[name], dc.native_cached('stream', name, tmp_path)
    for i in range(4):
        for o in range(4):
            run(ctx.dev_deflate, data, want, i, o)


def test_two_calls_give_equal_bytes(ctx, tmp_path):
    name = 'bytes_%d' % (2 * dc.SEG + 1)
    data, want = dc.cases()[name], dc.native_cached('gzip', name, tmp_path)
    assert run(ctx.dev_gzip, data, want, 1, 2) == run(ctx.dev_gzip, data, want, 1, 2)


@pytest.mark.parametrize('name', ['bytes_0', 'bytes_3', 'bytes_%d' % (dc.SEG + 1), 'random_70000'])
def test_a_buffer_one_byte_short_is_left_untouched(ctx, name, tmp_path):
    data = dc.cases()[name]
    for call, mode in ((ctx.dev_deflate, 'stream'), (ctx.dev_gzip, 'gzip')):
        want = dc.native_cached(mode, name, tmp_path)
        src = on_device(data, 1)
        buf, view = guarded(len(want) - 1, 3)
        with pytest.raises(sh.StError) as e:
            call(src, view, len(data))
        assert e.value.code == sh.ST_ERR_ARG
        assert int(buf.min()) == FILL == int(buf.max())


# ---- the three file forms with deflate='device' --------------------------------------------------------------
@pytest.fixture(scope='module')
def stream_case():
    return ordinary(np.random.default_rng(50_001), 50_001, 15)


def test_dev_spz_file_through_the_ring(ctx, tmp_path, monkeypatch, stream_case):
    """50,001 rows at degree 3 (3.2 MB of image, its member through 1 MiB slots) into a longer file
    at a non-zero position; the member inflates to the raw form's file and reads back as it does"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols = stream_case
    dev = to_dev(cols)
    raw_path, gz_path = tmp_path / 'raw.spz', tmp_path / 'gz.spz'
    rows, raw_size, raw_clamped = ctx.dev_spz_file(dev, str(raw_path), gzip_level=0)
    raw = raw_path.read_bytes()
    assert rows == 50_001 and raw_size == len(raw) == 16 + 50_001 * 64
    fd = os.open(str(gz_path), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.write(fd, b'P' * 5 + b'\xee' * (len(raw) + 4097))  # a longer file is cut
        os.lseek(fd, 5, os.SEEK_SET)
        rows, size, clamped = ctx.dev_spz_file(dev, fd, deflate='device')
        assert (rows, clamped) == (50_001, raw_clamped)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 5 + size == os.fstat(fd).st_size
    finally:
        os.close(fd)
    data = gz_path.read_bytes()
    member = data[5:]
    assert data[:5] == b'P' * 5 and (1 << 20) < len(member) == size < len(raw)
    assert gzip.decompress(member) == raw
    assert member == dc.native('gzip', raw, tmp_path)[0]
    gz_path.write_bytes(member)
    got, want = ctx.read_spz(str(gz_path)), oracle_readers.read_spz(raw)[0]
    assert list(got) == sh.reader_columns(45)
    for k, w in zip(got, want):
        assert np.array_equal(got[k].view(np.uint32), w.view(np.uint32)), k
    # gzip_level 0 stays raw whatever `deflate` says
    again = tmp_path / 'again.spz'
    assert ctx.dev_spz_file(dev, str(again), gzip_level=0, deflate='device') == (50_001, len(raw), raw_clamped)
    assert again.read_bytes() == raw
    # the host-table form and the .ply form give the same member
    h, p, src = tmp_path / 'host.spz', tmp_path / 'ply.spz', tmp_path / 'in.ply'
    assert ctx.spz_file(cols, [], str(h), deflate='device') == (50_001, len(member), raw_clamped)
    assert h.read_bytes() == member
    src.write_bytes(write_ply_ref.write_ply(['the input'], [('vertex', cols)]))
    assert ctx.ply_spz_file(str(src), [], str(p), deflate='device') == (50_001, len(member), raw_clamped)
    assert p.read_bytes() == member


@pytest.mark.parametrize('name', [n for n in SPZ_CASES if n in ('spz_v2_d0_n1', 'spz_v2_d2_n257', 'spz_v2_d3_n300')])
def test_fixture_tables_as_gzipped_files(ctx, tmp_path, name):
    file_raw, cols = fixture(name)
    dev = to_dev(cols)
    raw_path, gz_path = tmp_path / 'raw.spz', tmp_path / 'gz.spz'
    rows, raw_size, clamped = ctx.dev_spz_file(dev, str(raw_path), fractional_bits=file_raw[13], gzip_level=0)
    assert ctx.dev_spz_file(dev, str(gz_path), fractional_bits=file_raw[13], deflate='device') == \
        (rows, gz_path.stat().st_size, clamped)
    assert gzip.decompress(gz_path.read_bytes()) == raw_path.read_bytes()
    got, want = ctx.read_spz(str(gz_path)), oracle_readers.read_spz(raw_path.read_bytes())[0]
    for k, w in zip(got, want):
        assert np.array_equal(got[k].view(np.uint32), w.view(np.uint32)), k
    # one action through both one-call forms
    acts = [{'kind': 'scale', 'value': 2}]
    a, b = tmp_path / 'a.spz', tmp_path / 'b.spz'
    ra = ctx.spz_file(cols, acts, str(a), fractional_bits=8, gzip_level=0)
    rb = ctx.spz_file(cols, acts, str(b), fractional_bits=8, deflate='device')
    assert (ra[0], ra[2]) == (rb[0], rb[2]) and rb[1] == b.stat().st_size
    assert gzip.decompress(b.read_bytes()) == a.read_bytes()


@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_device_forms_refuse_descriptor(ctx, tmp_path, flags):
    cols = ordinary(np.random.default_rng(3), 100, 3)
    dev = to_dev(cols)
    p, src = tmp_path / 'keep.bin', tmp_path / 'in.ply'
    p.write_bytes(b'keep')
    src.write_bytes(write_ply_ref.write_ply([], [('vertex', cols)]))
    fd = os.open(str(p), flags)
    try:
        for call in (lambda: ctx.dev_spz_file(dev, fd, deflate='device'),
                     lambda: ctx.spz_file(cols, [], fd, deflate='device'),
                     lambda: ctx.ply_spz_file(str(src), [], fd, deflate='device')):
            with pytest.raises(sh.StError) as e:
                call()
            assert e.value.code == sh.ST_ERR_ARG
    finally:
        os.close(fd)
    assert p.read_bytes() == b'keep'
    with pytest.raises(sh.StError) as e:
        ctx.dev_spz_file([c for c in dev if c[0] != 'rot_3'], str(p), deflate='device')
    assert e.value.code == sh.ST_ERR_ARG and 'missing column rot_3' in str(e.value)
    with pytest.raises(ValueError):
        ctx.dev_spz_file(dev, str(p), deflate='gpu')
    assert p.read_bytes() == b'keep'


# ---- size ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_rows', [False, True])
def test_member_is_no_larger_than_zlib_level_1(ctx, zero_rows, tmp_path):
    """200,000 SH-3 rows (12.8 MB of image) of the benchmark's distributions, and the same with every
    harmonic of half the rows exactly 0: the device member against zlib.compress(raw, 1), the fastest
    the host path offers"""
    dev = to_dev(dc.size_table(zero_rows))
    image = torch.empty(sh.spz_image_size(200_000, 15), dtype=torch.uint8, device='cuda')
    assert ctx.dev_spz_image(dev, image, 12)[0] == image.numel()
    out = torch.empty(sh.gzip_bound(image.numel()), dtype=torch.uint8, device='cuda')
    size = ctx.dev_gzip(image, out)
    raw, member = image.cpu().numpy().tobytes(), out[:size].cpu().numpy().tobytes()
    level1, level6 = len(zlib.compress(raw, 1)), len(zlib.compress(raw, 6))
    print('zero_rows', zero_rows, 'raw', len(raw), 'device member', size, 'zlib 1', level1, 'zlib 6', level6)
    assert gzip.decompress(member) == raw
    assert member == dc.native('gzip', raw, tmp_path)[0]
    assert size <= level1
