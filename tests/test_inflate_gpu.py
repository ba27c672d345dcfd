"""INFLATE on the device (st_inflate.hip; include/st_abi.h, "inflating a gzip member on the
device"): st_dev_inflate and st_dev_gunzip give zlib's bytes on every stream of
tests/inflate_cases.py at chunk sizes 256, 1,024 and the default, with the statistics of
st_inflate.h's serial form run on the host (tests/native/inflate_cpu_check.cpp, checked against
zlib in tests/test_inflate_cpu.py), with inputs and outputs at every offset modulo 4 between
sentinels; the streams that must be declined are, with the sentinels intact; and
read_spz / read_spz_dev with inflate='device' give the columns of inflate='host' bit for bit, or
raise what it raises."""
import numpy as np
import pytest
import torch

import inflate_cases as ic
import splat_hip as sh
from golden_io import Golden
from test_write_ply_gpu import to_dev
from test_write_splat_spz_cpu import ordinary

pytestmark = pytest.mark.gpu

GUARD = 32
FILL = 0xA5
CASES = sorted(ic.cases())
DECLINED = sorted(ic.declined())
CHUNKS = [256, 1024, 0]
G = Golden('readers')
SPZ_FILES = [c['name'] for c in G.meta['cases'] if c['format'] == 'spz']


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def on_device(data, offset):
    """the bytes in a device tensor that starts `offset` bytes past a 256-byte boundary, between
    bytes that belong to no stream"""
    buf = torch.full((offset + len(data) + 8,), 0x5A, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + len(data)]
    if len(data):
        view.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    return view


def guarded(nbytes, offset):
    """(buffer of FILL, the view of nbytes at GUARD + offset inside it): sentinels on either side"""
    buf = torch.full((GUARD + offset + nbytes + GUARD + 4,), FILL, dtype=torch.uint8, device='cuda')
    return buf, buf[GUARD + offset:GUARD + offset + nbytes]


def run(ctx, kind, blob, expect, chunk, in_off, out_off):
    """(the statistics or None, the output bytes); the sentinels are checked"""
    src = on_device(blob, in_off)
    buf, view = guarded(expect, out_off)
    call = ctx.dev_inflate if kind == 'raw' else ctx.dev_gunzip
    st = call(src, view, chunk_bytes=chunk)
    host = buf.cpu().numpy()
    lo, hi = GUARD + out_off, GUARD + out_off + expect
    assert (host[:lo] == FILL).all() and (host[hi:] == FILL).all(), 'a byte outside the output was written'
    return st, host[lo:hi].tobytes()


@pytest.mark.parametrize('name', CASES)
def test_device_gives_zlibs_bytes_and_the_host_forms_statistics(ctx, name, tmp_path):
    kind, blob, data = ic.cases()[name]
    want = ic.native_cached(name, CHUNKS, tmp_path)
    k = CASES.index(name)
    for j, chunk in enumerate(CHUNKS):
        st, got = run(ctx, kind, blob, len(data), chunk, (k + j) % 4, (k // 4 + j) % 4)
        assert st is not None, (name, chunk, 'declined', ctx.last_inflate_stats)
        assert got == data, (name, chunk)
        assert st == want[chunk], (name, chunk)


def test_every_pair_of_offsets(ctx, tmp_path):
    kind, blob, data = ic.cases()['plane_ml1']
    want = ic.native_cached('plane_ml1', CHUNKS, tmp_path)[1024]
    for i in range(4):
        for o in range(4):
            st, got = run(ctx, kind, blob, len(data), 1024, i, o)
            assert got == data and st == want


def test_two_calls_give_equal_bytes(ctx):
    kind, blob, data = ic.cases()['chain']
    assert run(ctx, kind, blob, len(data), 256, 1, 2) == run(ctx, kind, blob, len(data), 256, 1, 2)


@pytest.mark.parametrize('name', DECLINED)
def test_declined_streams_are_declined(ctx, name):
    kind, blob, expect = ic.declined()[name]
    for j, chunk in enumerate(CHUNKS):
        st, _ = run(ctx, kind, blob, expect, chunk, j % 4, (j + 1) % 4)
        assert st is None, (name, chunk)


def test_a_chunk_size_below_256_is_an_argument_error(ctx):
    kind, blob, data = ic.cases()['bytes_3']
    with pytest.raises(sh.StError) as e:
        run(ctx, kind, blob, len(data), 255, 0, 0)
    assert e.value.code == sh.ST_ERR_ARG


# ---- the reader ---------------------------------------------------------------------------------------------
def same_columns(got, want):
    assert list(got) == list(want)
    for k in want:
        g, w = (a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in (got[k], want[k]))
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), k


def both_ways(ctx, path, chunk_bytes=0):
    """the host columns of inflate='host'; inflate='device' must give the same through both forms, or
    raise the same.  Returns the way the device reads went."""
    try:
        want = ctx.read_spz(path)
    except Exception as e:  # noqa: BLE001 -- whatever the host path raises is the reference here
        assert ctx.last_inflate == 'host'
        for read in (ctx.read_spz, ctx.read_spz_dev):
            with pytest.raises(type(e)) as got:
                read(path, inflate='device', chunk_bytes=chunk_bytes)
            assert str(got.value) == str(e) and ctx.last_inflate == 'host'
        return 'host'
    assert ctx.last_inflate == 'host'
    same_columns(ctx.read_spz(path, inflate='device', chunk_bytes=chunk_bytes), want)
    way = ctx.last_inflate
    dev = ctx.read_spz_dev(path, inflate='device', chunk_bytes=chunk_bytes)
    ctx.synchronize()
    same_columns(dev, want)
    assert ctx.last_inflate == way
    same_columns(ctx.read_spz_dev(path), want)
    assert ctx.last_inflate == 'host'
    return way


@pytest.mark.parametrize('name', SPZ_FILES)
def test_fixture_files_read_with_device_inflate(ctx, tmp_path, name):
    p = tmp_path / f'{name}.spz'
    blob = G[name + '_file'].tobytes()
    p.write_bytes(blob)
    way = both_ways(ctx, str(p))
    if 'fixture_' + name in ic.cases() and len(ic.cases()['fixture_' + name][2]) >= 16:
        try:
            sh.spz_layout(ic.cases()['fixture_' + name][2])
        except sh.StError:
            return  # the image itself is refused: the host path words it
        assert way == 'device'


@pytest.fixture(scope='module')
def table():
    return ordinary(np.random.default_rng(50_001), 50_001, 15)


@pytest.mark.parametrize('deflate', ['host', 'device'])
def test_50001_rows_written_both_ways(ctx, tmp_path, table, deflate):
    """3.2 MB of image: a zlib stream in 8 MiB host segments (one here), and the device writer's
    64 KiB segments; read at the default chunk size and at 4 KiB"""
    p = tmp_path / 'table.spz'
    rows, size, _ = ctx.dev_spz_file(to_dev(table), str(p), deflate=deflate)
    assert rows == 50_001 and size == p.stat().st_size
    assert both_ways(ctx, str(p)) == 'device'
    assert ctx.last_inflate_stats is not None
    assert both_ways(ctx, str(p), chunk_bytes=4096) == 'device'
    ctx.read_spz(str(p), inflate='device', chunk_bytes=4096)
    st = ctx.last_inflate_stats
    print(deflate, st)
    assert st['kept'] > 10 and st['chunks'] == -(-(size - 18) // 4096)


@pytest.mark.parametrize('damage', ['flip', 'truncate', 'append'])
def test_a_corrupted_file_raises_what_the_host_path_raises(ctx, tmp_path, table, damage):
    p = tmp_path / 'table.spz'
    ctx.dev_spz_file(to_dev(table), str(p), deflate='device')
    blob = bytearray(p.read_bytes())
    if damage == 'flip':
        blob[len(blob) // 2] ^= 0x40
    elif damage == 'truncate':
        blob = blob[:len(blob) - 5]
    else:
        blob += b'\x1f\x8b\x08 not a member'
    p.write_bytes(bytes(blob))
    with pytest.raises(Exception):
        ctx.read_spz(str(p))
    assert both_ways(ctx, str(p)) == 'host'


def test_inflate_argument(ctx, tmp_path):
    p = tmp_path / 'x.spz'
    p.write_bytes(G['spz_v2_d0_n4_file'].tobytes())
    with pytest.raises(ValueError):
        ctx.read_spz(str(p), inflate='gpu')
