"""The .splat / .ksplat / .spz readers on the GPU against the reference's own readers
(tests/golden/readers.*): every fixture file through the host-column and the device-column form,
every column bit-equal; a ~1M-row .splat through several pinned chunks; and the device columns of
read_spz_dev fed on to the compressed-PLY writer.
"""
import numpy as np
import pytest

import splat_hip as sh
from golden_io import Golden
from test_ply_cpu import same

pytestmark = pytest.mark.gpu

G = Golden('readers')
CASES = {c['name']: c for c in G.meta['cases']}


@pytest.fixture(scope='module')
def ctx():
    import torch  # noqa: F401
    c = sh.Context(0)
    yield c
    c.close()


def write_case(tmp_path, name):
    p = tmp_path / f'{name}.{CASES[name]["format"]}'
    p.write_bytes(G[name + '_file'].tobytes())
    return str(p)


def expect(name):
    c = CASES[name]
    want = G[name + '_cols']
    assert want.shape == (14 + c['nsh'], c['n'])
    return dict(zip(c['columns'], want))


def check_columns(got, want, what):
    assert list(got) == list(want), what
    for k, w in want.items():
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k)
        if not same(g, w):
            i = int(np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))[0])
            raise AssertionError(f'{what}: {k}[{i}] = {g.view(np.uint32)[i]:#010x}, the reference has '
                                 f'{w.view(np.uint32)[i]:#010x}')


@pytest.mark.parametrize('name', list(CASES))
def test_reader_matches_reference(ctx, tmp_path, name):
    path = write_case(tmp_path, name)
    fmt = CASES[name]['format']
    want = expect(name)
    check_columns(getattr(ctx, f'read_{fmt}')(path), want, f'{name} host columns')
    dev = getattr(ctx, f'read_{fmt}_dev')(path)
    ctx.synchronize()
    check_columns(dev, want, f'{name} device columns')
    check_columns(ctx.read_table(path), want, f'{name} read_table')


def test_splat_1m_rows_in_several_chunks(ctx, tmp_path, monkeypatch):
    """the 1025 fixture rows repeated to 1,000,001 rows, read through 4 MiB pinned chunks (eight of
    them): the rows are independent, so the columns are the fixture's tiled"""
    n = 1_000_001
    rows = G['splat_n1025_file'].reshape(1025, 32)
    reps = -(-n // 1025)
    p = tmp_path / 'big.splat'
    p.write_bytes(np.tile(rows, (reps, 1))[:n].tobytes())
    want = {k: np.tile(v, reps)[:n] for k, v in expect('splat_n1025').items()}
    monkeypatch.setenv('ST_PLY_CHUNK', str(4 << 20))
    check_columns(ctx.read_splat(str(p)), want, 'host columns')
    dev = ctx.read_splat_dev(str(p))
    ctx.synchronize()
    check_columns(dev, want, 'device columns')


def test_spz_device_columns_feed_the_compressed_ply_writer(ctx, tmp_path):
    """read_spz_dev's tensors go straight into st_dev_compressed_ply: the same bytes as the
    reference reader's columns uploaded and fed the same way"""
    import torch
    name = 'spz_v2_d3_n300'
    n = CASES[name]['n']
    acts = [{'kind': 'filterNaN'}]

    def pack(cols):
        chunk = torch.full(((n + 255) // 256 * 18,), 7.0, device='cuda')
        vertex = torch.zeros(n * 4, dtype=torch.int32, device='cuda')
        shb = torch.zeros(n * 45, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()  # the fills run on torch's stream, the writer on the context's
        m, C = ctx.dev_compressed_ply(list(cols.items()), acts, chunk, vertex, shb)
        ctx.synchronize()
        return m, C, chunk.cpu().numpy(), vertex.cpu().numpy(), shb.cpu().numpy()

    got = pack(ctx.read_spz_dev(write_case(tmp_path, name)))
    want = pack({k: torch.from_numpy(v.copy()).cuda() for k, v in expect(name).items()})
    assert got[:2] == want[:2] == (n, 15)
    for g, w, what in zip(got[2:], want[2:], ('chunk', 'vertex', 'sh')):
        assert same(g, w), what


def _device_out(nsh, n):
    import torch
    out = {k: torch.full((n,), 7.0, device='cuda') for k in sh.reader_columns(nsh)}
    torch.cuda.synchronize()  # the fills run on torch's stream, the decode on the context's
    return out


def _device_bytes(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


@pytest.mark.parametrize('name', ['splat_n257', 'ksplat_two_sections', 'ksplat_partial_walk', 'ksplat_m2_d1',
                                  'spz_v3_d3_n300'])
def test_decode_of_bytes_already_in_hbm(ctx, name):
    """st_dev_*_decode: the record bytes uploaded by the caller; for .ksplat once with a host copy of
    the whole file and once with the headers alone (the partial bucket sizes then come down from HBM)"""
    c = CASES[name]
    data = G[name + '_file'].tobytes()
    want = expect(name)
    if c['format'] == 'splat':
        out = _device_out(0, c['n'])
        ctx.dev_splat_decode(_device_bytes(data), out)
        ctx.synchronize()
        check_columns(out, want, name)
    elif c['format'] == 'spz':
        out = _device_out(c['nsh'], c['n'])
        ctx.dev_spz_decode(_device_bytes(sh.spz_inflate(data)), out)
        ctx.synchronize()
        check_columns(out, want, name)
    else:
        sections = int.from_bytes(data[4:8], 'little')
        for host in (data, data[:4096 + 1024 * sections]):
            out = _device_out(c['nsh'], c['n'])
            ctx.dev_ksplat_decode(host, _device_bytes(data), out)
            ctx.synchronize()
            check_columns(out, want, f'{name} with {len(host)} host bytes')
