"""The CSV writer on the GPU (k_csv_len, the scan, k_csv_rows, the file-streaming forms,
st_csv_file / st_ply_csv_file) against the reference's own writeCsv files (tests/golden/write_csv.*)
and the Python restatement pinned to them (tests/write_csv_ref.py).  Every byte equal."""
import os

import numpy as np
import pytest
import torch

import splat_hip as sh
import write_csv_ref as ref
from golden_io import Golden
from test_write_csv_cpu import C, CASES, case_columns, case_file
from test_write_ply_gpu import CHAINS, random_columns, to_dev

pytestmark = pytest.mark.gpu

PLY = Golden('ply_io')
CSV_LDS_BYTES = 48 * 1024
GUARD = 64


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def max_row_bytes(schema):
    return sum(ref.MAX_CELL[np.dtype(t).str[1:]] + 1 for _, t in schema)


def rows_per_block(schema):
    """the rows one workgroup of k_csv_rows takes: as many as fit its LDS image by the worst-case width"""
    return min(256, CSV_LDS_BYTES // max_row_bytes(schema))


def row_texts(cols):
    """every row's bytes, separator and newline included: list of bytes"""
    with np.errstate(invalid='ignore'):
        texts = [ref.column_text(a) for _, a in cols]
    return [(','.join(cells) + '\n').encode() for cells in zip(*texts)]


def csv_rows(ctx, dev, row0, nrows, want):
    """dev_csv_rows into a buffer of exactly the bytes wanted plus a guard tail: the size is exact,
    the bytes are equal, the tail is untouched"""
    out = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    size = ctx.dev_csv_rows(dev, out[:len(want)] if len(want) else out[:0], row0, nrows)
    got = out.cpu().numpy()
    assert size == len(want), (row0, nrows, size, len(want))
    assert got[:size].tobytes() == want, (row0, nrows)
    assert (got[size:] == 0xA5).all(), (row0, nrows)


# ---- the reference's files ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_dev_csv_rows_matches_reference(ctx, name):
    cols = case_columns(name)
    file = case_file(name)
    head = len(ref.header([k for k, _ in cols]))
    csv_rows(ctx, to_dev(cols), 0, C.meta[name]['rows'], file[head:])
    if name == 'empty':
        assert file[head:] == b''


@pytest.mark.parametrize('name', CASES)
def test_dev_csv_file_matches_reference(ctx, tmp_path, name):
    p = tmp_path / 'out.csv'
    assert ctx.dev_csv_file(to_dev(case_columns(name)), str(p)) == len(case_file(name))
    assert p.read_bytes() == case_file(name)


# ---- block edges ---------------------------------------------------------------------------------
F64_25 = -0.0000012345678901234567   # 25 bytes of text
MIXED8 = [('c', np.int8), ('uc', np.uint8), ('s', np.int16), ('us', np.uint16), ('i', np.int32), ('ui', np.uint32),
          ('f', np.float32), ('d', np.float64)]
SCHEMAS = {
    'u8': [('k', np.uint8)],                                                    # rows of 2 to 4 bytes
    'f32x14': [(f'f{i}', np.float32) for i in range(14)],
    'f32x62_u8': [(f'f{i}', np.float32) for i in range(62)] + [('k', np.uint8)],
    'mixed8': MIXED8,
    'f64x1500': [(f'd{i}', np.float64) for i in range(1500)],                   # one row per workgroup
}


@pytest.mark.parametrize('name', list(SCHEMAS))
def test_dev_csv_rows_block_edges(ctx, name):
    """every row count around the workgroup's block, from row 0 and from inside the table"""
    schema = SCHEMAS[name]
    RB = rows_per_block(schema)
    assert RB == {'u8': 256, 'f32x14': 135, 'f32x62_u8': 30, 'mixed8': 256, 'f64x1500': 1}[name]
    n = 2 * RB + 4
    if name == 'f64x1500':   # every cell at its longest: the widest admitted row at its bound
        cols = [(k, np.full(n, F64_25)) for k, _ in schema]
    else:
        cols = random_columns(np.random.default_rng(len(name)), schema, n)
    rows = row_texts(cols)
    if name == 'f64x1500':
        assert all(len(r) == max_row_bytes(schema) == 39000 for r in rows)
    dev = to_dev(cols)
    for row0, nrows in [(0, 1), (0, 3), (0, RB - 1), (0, RB), (0, RB + 1), (0, 2 * RB + 1), (2, RB + 1), (3, 0),
                        (1, 2 * RB + 1), (n - 1, 1)]:
        csv_rows(ctx, dev, row0, nrows, b''.join(rows[row0:row0 + nrows]))


def test_row_width_limit(ctx):
    most = CSV_LDS_BYTES // 26   # float64 columns
    out = torch.zeros(2 * CSV_LDS_BYTES, dtype=torch.uint8, device='cuda')
    cols = [(f'd{i}', np.full(1, F64_25)) for i in range(most + 1)]
    assert ctx.dev_csv_rows(to_dev(cols[:most]), out) == most * 26
    assert out[:most * 26].cpu().numpy().tobytes() == row_texts(cols[:most])[0]
    out.fill_(7)
    with pytest.raises(sh.StError) as e:
        ctx.dev_csv_rows(to_dev(cols), out)
    assert e.value.code == sh.ST_ERR_UNSUPPORTED
    assert int(out.min()) == 7 == int(out.max())


def test_unequal_rows_in_one_block(ctx):
    """rows of all-'0' cells between rows of all 25-byte cells, and a column of NaN: a row's place
    comes from the scan of the real lengths"""
    n = 601
    long = np.where(np.arange(n) % 2 == 1, F64_25, 0.0)
    cols = [(f'd{i}', long.copy()) for i in range(20)] + [('nan', np.full(n, np.nan, np.float32))]
    rows = row_texts(cols)
    assert {len(r) for r in rows} == {20 * 2 + 4, 20 * 26 + 4}
    assert 1 < rows_per_block([(k, a.dtype) for k, a in cols]) < n // 2
    dev = to_dev(cols)
    csv_rows(ctx, dev, 0, n, b''.join(rows))
    csv_rows(ctx, dev, 1, n - 2, b''.join(rows[1:n - 1]))


def test_random_bit_patterns(ctx):
    schema = MIXED8 + [('g', np.float32)]
    cols = random_columns(np.random.default_rng(4099), schema, 4099)
    csv_rows(ctx, to_dev(cols), 0, 4099, b''.join(row_texts(cols)))


def test_dev_csv_rows_argument_checks(ctx):
    cols = random_columns(np.random.default_rng(2), MIXED8, 100)
    want = b''.join(row_texts(cols))
    dev = to_dev(cols)
    out = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    with pytest.raises(sh.StError) as e:   # one byte short: nothing is written
        ctx.dev_csv_rows(dev, out[:len(want) - 1])
    assert e.value.code == sh.ST_ERR_ARG
    assert int(out.min()) == 0xA5 == int(out.max())
    with pytest.raises(sh.StError) as e:   # no columns
        ctx.dev_csv_rows([], out, 0, 0)
    assert e.value.code == sh.ST_ERR_ARG
    with pytest.raises(sh.StError) as e:   # rows outside the table
        ctx.dev_csv_rows(dev, out, 98, 3)
    assert e.value.code == sh.ST_ERR_ARG
    with pytest.raises(sh.StError) as e:   # output not 4-byte aligned
        ctx.dev_csv_rows(dev, out[1:])
    assert e.value.code == sh.ST_ERR_ARG
    assert int(out.min()) == 0xA5 == int(out.max())


# ---- streaming -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stream_case():
    n = 50_001
    rng = np.random.default_rng(14)
    cols = [(f'f{i}', rng.normal(0, 1, n).astype(np.float32)) for i in range(14)]
    rows = row_texts(cols)
    return cols, ref.header([k for k, _ in cols]), rows


def test_csv_file_streams_through_the_ring(ctx, tmp_path, monkeypatch, stream_case):
    """50,001 rows of 14 float32 through 1 MiB slots: 2,880 rows a piece, 18 pieces, four times round
    the ring"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols, head, rows = stream_case
    want = head + b''.join(rows)
    assert len(want) > 12 * (1 << 20)
    assert (1 << 20) // max_row_bytes([(k, a.dtype) for k, a in cols]) == 2880
    dev = to_dev(cols)
    # a longer file is cut at the end of the output
    p = tmp_path / 'rows.csv'
    p.write_bytes(b'\xee' * (len(want) + 4097))
    assert ctx.dev_csv_file(dev, str(p)) == len(want)
    assert p.read_bytes() == want
    # from a descriptor's position: the bytes before it stay, the position ends after the output
    q = tmp_path / 'at.csv'
    fd = os.open(str(q), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.write(fd, b'P' * 37)
        assert ctx.dev_csv_file(dev, fd) == len(want)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want)
    finally:
        os.close(fd)
    assert q.read_bytes() == b'P' * 37 + want
    # the host table form
    h = tmp_path / 'host.csv'
    assert ctx.csv_file(cols, [], str(h)) == (len(rows), len(want))
    assert h.read_bytes() == want


def test_csv_file_beyond_4gib(ctx, tmp_path, monkeypatch, stream_case):
    """at position 2^32 + 5 of a sparse file: offsets are 64-bit all the way"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols, head, rows = stream_case
    n = 6000   # three pieces
    want = head + b''.join(rows[:n])
    pos = (1 << 32) + 5
    p = tmp_path / 'sparse.csv'
    fd = os.open(str(p), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.lseek(fd, pos, os.SEEK_SET)
        assert ctx.dev_csv_file([(k, torch.from_numpy(a[:n]).cuda()) for k, a in cols], fd) == len(want)
        assert os.lseek(fd, 0, os.SEEK_CUR) == pos + len(want) == os.fstat(fd).st_size
        assert os.pread(fd, len(want) + 16, pos) == want
        assert os.pread(fd, 8, pos - 8) == b'\0' * 8
    finally:
        os.close(fd)


@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_csv_file_refuses_descriptor(ctx, tmp_path, flags):
    cols = random_columns(np.random.default_rng(3), MIXED8, 100)
    p = tmp_path / 'keep.csv'
    p.write_bytes(b'keep')
    fd = os.open(str(p), flags)
    try:
        with pytest.raises(sh.StError) as e:
            ctx.dev_csv_file(to_dev(cols), fd)
        assert e.value.code == sh.ST_ERR_ARG
        with pytest.raises(sh.StError) as e:
            ctx.csv_file(cols, [], fd)
        assert e.value.code == sh.ST_ERR_ARG
    finally:
        os.close(fd)
    assert p.read_bytes() == b'keep'


def test_csv_file_without_columns(ctx, tmp_path):
    p = tmp_path / 'none.csv'
    p.write_bytes(b'keep')
    with pytest.raises(sh.StError) as e:
        ctx.csv_file([], [], str(p))
    assert e.value.code == sh.ST_ERR_ARG
    assert p.read_bytes() == b'keep'


# ---- processDataTable + writeCsv -------------------------------------------------------------------
@pytest.mark.parametrize('case', ['config1', 'filters_sh3'])
def test_csv_file_with_actions(ctx, tmp_path, case):
    """the expectation: the restatement applied to ctx.process's table (pinned by the process_chain
    tests) -- its columns, order and names"""
    make, acts = CHAINS[case]
    cols = make(np.random.default_rng(len(case)))
    processed = ctx.process([(k, a.copy()) for k, a in cols], acts)
    want = ref.write_csv(processed)
    if case == 'filters_sh3':
        assert 0 < len(processed[0][1]) < 777 and len(processed) == len(cols) - 36
    keep = [(k, a.copy()) for k, a in cols]
    out = tmp_path / 'host.csv'
    assert ctx.csv_file(cols, acts, str(out)) == (len(processed[0][1]), len(want))
    assert out.read_bytes() == want
    assert all(a.tobytes() == b.tobytes() for (_, a), (_, b) in zip(cols, keep))


def test_ply_csv_file_matches_csv_file(ctx, tmp_path):
    """the CLI's in.ply out.csv on the mixed-type file of the ply_io fixtures: the vertex element"""
    src = tmp_path / 'mixed.ply'
    src.write_bytes(PLY['mixed_file'].tobytes())
    _, els = ctx.read_ply(str(src))
    name, table = els[0]
    assert name == 'vertex' and len({a.dtype for a in table.values()}) == 8
    want = ref.write_csv(list(table.items()))
    a, b = tmp_path / 'a.csv', tmp_path / 'b.csv'
    assert ctx.csv_file(table, [], str(a)) == (1500, len(want))
    assert ctx.ply_csv_file(str(src), [], str(b)) == (1500, len(want))
    assert a.read_bytes() == want == b.read_bytes()
    # the second element, by index
    extra = ref.write_csv(list(els[1][1].items()))
    assert ctx.ply_csv_file(str(src), [], str(b), element=1) == (7, len(extra))
    assert b.read_bytes() == extra
