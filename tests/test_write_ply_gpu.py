"""The PLY writer on the GPU (k_ply_rows, the file-streaming forms, st_ply_file / st_ply_ply_file)
against the reference's own writePly output (tests/golden/write_ply.*, the mixed-type file of
tests/golden/ply_io.*) and its numpy restatement (tests/write_ply_ref.py).  Every byte equal."""
import os

import numpy as np
import pytest
import torch

import splat_hip as sh
import write_ply_ref as ref
from golden_io import Golden, gs_column_names
from test_ply_cpu import compressed_file, same
from test_write_ply_cpu import G, W, case_elements

pytestmark = pytest.mark.gpu

READERS = Golden('readers')
LDS_ROWS_BYTES = 48 * 1024


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def rows_per_block(R):
    return min(256, (LDS_ROWS_BYTES // R) & ~3)


def random_columns(rng, schema, n):
    """columns of random bytes (every bit pattern, NaNs included): [(name, numpy array)]"""
    return [(k, rng.integers(0, 256, n * np.dtype(t).itemsize, dtype=np.uint8).view(t)) for k, t in schema]


def to_dev(cols):
    return [(k, torch.from_numpy(a).cuda()) for k, a in cols]


MIXED = [(k, np.dtype(t)) for k, t in G.meta['mixed']['elements'][0]['columns']]
SCHEMAS = {
    5: [('v', np.float32), ('k', np.uint8)],                       # block and tail no multiples of 4
    11: [('a', np.uint8), ('b', np.float64), ('c', np.int16)],     # an 8-byte field at offset 1
    30: MIXED,                                                     # all eight types
    104: [(f'f{i}', np.float32) for i in range(26)],               # RB * R = 26 KiB: the last 256-thread launch
    108: [(f'f{i}', np.float32) for i in range(27)],               # 27 KiB, above 160 KiB / 6: 512 threads
    248: [(f'f{i}', np.float32) for i in range(62)],               # SH-3, RB = 196
    249: [(f'f{i}', np.float32) for i in range(62)] + [('k', np.uint8)],
    256: [(f'f{i}', np.float32) for i in range(64)],               # a whole number of LDS bank rows
    12000: [(f'd{i}', np.float64) for i in range(1500)],           # RB = 4
    12288: [(f'd{i}', np.float64) for i in range(1536)],           # the longest row
}


@pytest.mark.parametrize('R', list(SCHEMAS))
def test_dev_ply_rows_matches_restatement(ctx, R):
    """every row count around the workgroup's block, from row 0 and from inside the table, into a
    buffer with a guard tail"""
    schema = SCHEMAS[R]
    assert sum(np.dtype(t).itemsize for _, t in schema) == R
    RB = rows_per_block(R)
    assert {248: 196, 12000: 4, 12288: 4, 5: 256}.get(R, RB) == RB
    n = 2 * RB + 4
    cols = random_columns(np.random.default_rng(R), schema, n)
    want = np.frombuffer(ref.rows(cols), np.uint8).reshape(n, R)
    dev = to_dev(cols)
    guard = 64
    for row0, nrows in [(0, 1), (0, 3), (0, RB - 1), (0, RB), (0, RB + 1), (0, 2 * RB + 1), (2, RB + 1), (3, 0),
                        (n - 1, 1)]:
        out = torch.full((nrows * R + guard,), 0xA5, dtype=torch.uint8, device='cuda')
        ctx.dev_ply_rows(dev, out, row0, nrows)
        got = out.cpu().numpy()
        assert np.array_equal(got[:nrows * R], want[row0:row0 + nrows].ravel()), (R, row0, nrows)
        assert (got[nrows * R:] == 0xA5).all(), (R, row0, nrows)


def test_dev_ply_rows_argument_checks(ctx):
    out = torch.zeros(64 * 1024, dtype=torch.uint8, device='cuda')
    wide = to_dev(random_columns(np.random.default_rng(1), [(f'd{i}', np.float64) for i in range(1537)], 4))
    with pytest.raises(sh.StError) as e:   # R = 12,296
        ctx.dev_ply_rows(wide, out)
    assert e.value.code == sh.ST_ERR_UNSUPPORTED
    cols = to_dev(random_columns(np.random.default_rng(2), SCHEMAS[5], 10))
    with pytest.raises(sh.StError) as e:   # rows outside the table
        ctx.dev_ply_rows(cols, out, 8, 3)
    assert e.value.code == sh.ST_ERR_ARG
    with pytest.raises(sh.StError) as e:   # output not 4-byte aligned
        ctx.dev_ply_rows(cols, out[1:])
    assert e.value.code == sh.ST_ERR_ARG
    # no columns: nothing is written
    out.fill_(7)
    ctx.dev_ply_rows([], out, 0, 0)
    assert int(out.min()) == 7


# ---- the reference's files -----------------------------------------------------------------------
@pytest.mark.parametrize('name', list(W.meta))
def test_dev_ply_file_matches_reference(ctx, tmp_path, name):
    p = tmp_path / 'out.ply'
    size = ctx.dev_ply_file([(el, to_dev(cols), n) for el, cols, n in case_elements(name)], str(p),
                            W.meta[name]['comments'])
    assert p.read_bytes() == W[f'{name}_file'].tobytes()
    assert size == len(W[f'{name}_file'])


def test_mixed_file_round_trip(ctx, tmp_path):
    """writePly(readPly(f)) == f: both elements of the mixed-type file, from device columns"""
    src = tmp_path / 'mixed.ply'
    src.write_bytes(G['mixed_file'].tobytes())
    comments, els = ctx.read_ply_dev(str(src))
    out = tmp_path / 'again.ply'
    size = ctx.dev_ply_file([(name, list(cols.items())) for name, cols in els], str(out), comments)
    assert out.read_bytes() == G['mixed_file'].tobytes()
    assert size == len(G['mixed_file'])


@pytest.mark.parametrize('name', ['cli', 'sh1', 'types8', 'empty'])
def test_ply_file_without_actions_matches_reference(ctx, tmp_path, name):
    (el, cols, n), = case_elements(name)
    p = tmp_path / 'out.ply'
    m, size = ctx.ply_file(cols, [], str(p), W.meta[name]['comments'])
    assert (m, size) == (n, len(W[f'{name}_file']))
    assert p.read_bytes() == W[f'{name}_file'].tobytes()


# ---- streaming -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stream_case():
    n = 50_001
    cols = random_columns(np.random.default_rng(249), SCHEMAS[249], n)
    return cols, ref.rows(cols)


def test_rows_file_streams_through_the_ring(ctx, tmp_path, monkeypatch, stream_case):
    """50,001 rows of 249 bytes through 1 MiB slots: 13 pieces, three times round the ring"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols, want = stream_case
    dev = to_dev(cols)
    # a longer file is cut at the end of the rows
    p = tmp_path / 'rows.bin'
    p.write_bytes(b'\xee' * (len(want) + 4097))
    assert ctx.ply_rows_file(dev, str(p)) == len(want)
    assert p.read_bytes() == want
    # from a descriptor's position: the bytes before it stay, the position ends after the rows
    q = tmp_path / 'at.bin'
    fd = os.open(str(q), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.write(fd, b'P' * 37)
        assert ctx.ply_rows_file(dev, fd) == len(want)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want)
    finally:
        os.close(fd)
    assert q.read_bytes() == b'P' * 37 + want
    # the host table form
    h = tmp_path / 'host.bin'
    assert ctx.ply_rows_file(cols, str(h)) == len(want)
    assert h.read_bytes() == want


@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_rows_file_refuses_descriptor(ctx, tmp_path, flags):
    cols = random_columns(np.random.default_rng(3), SCHEMAS[5], 100)
    p = tmp_path / 'keep.bin'
    p.write_bytes(b'keep')
    for table in (cols, to_dev(cols)):
        fd = os.open(str(p), flags)
        try:
            with pytest.raises(sh.StError) as e:
                ctx.ply_rows_file(table, fd)
            assert e.value.code == sh.ST_ERR_ARG
            with pytest.raises(sh.StError) as e:
                ctx.ply_file(cols, [], fd)
            assert e.value.code == sh.ST_ERR_ARG
        finally:
            os.close(fd)
    assert p.read_bytes() == b'keep'


# ---- processDataTable + writePly -------------------------------------------------------------------
def gs_table(rng, n, coeffs):
    return [(k, rng.normal(0, 1, n).astype(np.float32)) for k in gs_column_names(coeffs)]


def typed_table(rng, n):
    cols = dict(gs_table(rng, n, 0))
    cols['x'] = cols['x'].astype(np.float64)
    cols['y'] = (cols['y'] * 100).astype(np.int16)
    cols['z'] = (cols['z'] * 1000).astype(np.int32)
    cols['rot_0'] = cols['rot_0'].astype(np.float64)
    cols['id'] = np.arange(n, dtype=np.uint32)
    cols['flag'] = rng.integers(0, 256, n, dtype=np.uint8)
    return list(cols.items())


def sh3_with_nans(rng, n):
    cols = gs_table(rng, n, 15)
    for j, (k, a) in enumerate(cols):
        a[(7 * j + 3) % n::97] = np.nan if j % 3 else np.inf
    return cols


CHAINS = {
    # BASELINE config 1: -s 0.5 -t 0,0,10
    'config1': (lambda rng: gs_table(rng, 1000, 0),
                [{'kind': 'scale', 'value': 0.5}, {'kind': 'translate', 'value': (0, 0, 10)}]),
    'filters_sh3': (lambda rng: sh3_with_nans(rng, 777),
                    [{'kind': 'rotate', 'value': (0, 90, 0)}, {'kind': 'filterNaN'},
                     {'kind': 'filterByValue', 'columnName': 'opacity', 'comparator': 'gt', 'value': -0.5},
                     {'kind': 'filterBands', 'value': 1}]),
    'typed': (lambda rng: typed_table(rng, 513),
              [{'kind': 'translate', 'value': (1, -2, 0.5)}, {'kind': 'rotate', 'value': (10, 20, 30)},
               {'kind': 'scale', 'value': 2}]),
}


@pytest.mark.parametrize('case', list(CHAINS))
def test_ply_file_and_ply_ply_file_with_actions(ctx, tmp_path, case):
    """the expectation: the restatement applied to ctx.process's table (pinned by the process_chain
    tests) -- its columns, order, names and types"""
    make, acts = CHAINS[case]
    cols = make(np.random.default_rng(len(case)))
    processed = ctx.process([(k, a.copy()) for k, a in cols], acts)
    comments = ['written by the test'] if case == 'typed' else []
    want = ref.write_ply(comments, [('vertex', processed, len(processed[0][1]))])
    if case == 'filters_sh3':
        assert 0 < len(processed[0][1]) < 777 and len(processed) == len(cols) - 36
    keep = [(k, a.copy()) for k, a in cols]
    out = tmp_path / 'host.ply'
    m, size = ctx.ply_file(cols, acts, str(out), comments)
    assert (m, size) == (len(processed[0][1]), len(want))
    assert out.read_bytes() == want
    assert all(same(a, b) for (_, a), (_, b) in zip(cols, keep))
    # the CLI's in.ply [actions] out.ply
    src = tmp_path / 'in.ply'
    src.write_bytes(ref.write_ply(['the input'], [('vertex', cols)]))
    before = src.read_bytes()
    out2 = tmp_path / 'file.ply'
    assert ctx.ply_ply_file(str(src), acts, str(out2), comments) == (m, size)
    assert out2.read_bytes() == want
    assert src.read_bytes() == before


# ---- round trips across formats ------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in READERS.meta['cases']])
def test_reader_to_ply_round_trip(ctx, tmp_path, name):
    case = next(c for c in READERS.meta['cases'] if c['name'] == name)
    src = tmp_path / f'{name}.{case["format"]}'
    src.write_bytes(READERS[name + '_file'].tobytes())
    dev = getattr(ctx, f'read_{case["format"]}_dev')(str(src))
    out = tmp_path / 'out.ply'
    ctx.dev_ply_file(dev, str(out))
    comments, els = ctx.read_ply(str(out))
    assert comments == [] and [e for e, _ in els] == ['vertex']
    got = els[0][1]
    assert list(got) == list(dev) == case['columns']
    for (k, a), w in zip(got.items(), READERS[name + '_cols']):
        assert a.dtype == np.float32 and same(a, w), (name, k)
        assert same(a, dev[k].cpu().numpy()), (name, k)


@pytest.mark.parametrize('name', [c['name'] for c in G.meta['compressed']])
def test_compressed_ply_to_ply_round_trip(ctx, tmp_path, name):
    src = tmp_path / f'{name}.compressed.ply'
    src.write_bytes(compressed_file(name))
    table = ctx.read_table(str(src))
    out = tmp_path / 'out.ply'
    m, _ = ctx.ply_file(table, [], str(out))
    _, els = ctx.read_ply(str(out))
    got = els[0][1]
    assert m == len(table['x']) and list(got) == list(table)
    for k, a in got.items():
        assert same(a, table[k]), (name, k)
