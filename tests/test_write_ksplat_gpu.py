"""The .ksplat writer on the GPU (the plan kernels, k_ksplat_records, the image and file forms, the
one-call chain forms) against the numpy restatement of its rules (tests/write_ksplat_ref.py), byte for
byte, and the reference's fixture files under the conditions of tests/test_write_ksplat_cpu.py."""
import os

import numpy as np
import pytest
import torch

import oracle_typed as ot
import readers as oracle_readers
import splat_hip as sh
import write_ksplat_cases as kc
import write_ksplat_ref as ref
import write_ply_ref
from test_write_ply_gpu import CHAINS, to_dev
from test_write_splat_spz_cpu import first_difference

pytestmark = pytest.mark.gpu

GUARD = 32
FILL = 0xA5
COEFFS = [0, 3, 8, 15]


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


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- whole images ------------------------------------------------------------------------------------
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 255, 256, 257, 258, 259, 513])
def test_dev_ksplat_image_matches_restatement(ctx, n, mode, degree):
    """several cells, from 257 rows on one of more than 256 rows (kc.image_table); the output buffer at
    offsets 0-3 modulo 4 over the cases, all four at the sizes with a last tile of 1-3 records"""
    cols = kc.image_table(n, COEFFS[degree])
    want, want_clamped = ref.image(cols, mode, -1, 5.0, -1.25, 2.0)
    dev = to_dev(cols)
    for offset in (range(4) if n in (3, 257, 259) else [(n + mode + degree) % 4]):
        buf, view = guarded(len(want), offset)
        size, clamped = ctx.dev_ksplat_image(dev, view, mode, -1, 5.0, -1.25, 2.0)
        assert size == len(want) and clamped == want_clamped == 0
        assert first_difference(view.cpu().numpy().tobytes(), want) is None, offset
        assert guards_intact(buf, offset, len(want)), offset


@pytest.mark.parametrize('mode,degree,table_degree', [(2, 1, 3), (1, 0, 2), (0, 2, 3), (2, 3, 3)])
def test_dev_ksplat_image_drops_bands_and_takes_mixed_types(ctx, mode, degree, table_degree):
    cols = kc.image_table(300, COEFFS[table_degree], dtype=np.float64)
    cols = [(k, a.astype(np.float32) if i % 3 == 0 else a) for i, (k, a) in enumerate(cols)]
    want, _ = ref.image(cols, mode, degree, 2.5, -0.75, 0.5)
    buf, view = guarded(len(want), 1)
    size, _ = ctx.dev_ksplat_image(to_dev(cols), view, mode, degree, 2.5, -0.75, 0.5)
    assert size == len(want) and first_difference(view.cpu().numpy().tobytes(), want) is None
    assert guards_intact(buf, 1, len(want))


# ---- records from inside a table ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode,degree', [(2, 1), (2, 3), (1, 2), (0, 1)])   # strides 33, 69, 72, 80
@pytest.mark.parametrize('rec0', [3, 256, 257])
def test_dev_ksplat_records_from_inside_the_table(ctx, rec0, mode, degree):
    """separate guarded buffers at offsets 0-3; 515 rows leave last tiles of 1-3 records"""
    n, C = 515, COEFFS[degree]
    cols = kc.image_table(n, C)
    p = ref.plan(cols, 5.0)
    want = ref.records(cols, mode, p['order'], p['bucket'], p['centres'])
    dev = to_dev(cols)
    order, bucket, centres = i32(p['order']), i32(p['bucket']), torch.from_numpy(p['centres']).cuda()
    for shift in range(4):
        for nrec in (n - rec0, n - rec0 - 1 - shift % 2):
            w = want[rec0:rec0 + nrec].tobytes()
            buf, view = guarded(len(w), shift)
            ctx.dev_ksplat_records(dev, view, mode, order, bucket, centres, rec0=rec0, nrec=nrec)
            assert first_difference(view.cpu().numpy().tobytes(), w) is None, (shift, nrec)
            assert guards_intact(buf, shift, len(w)), (shift, nrec)
    # the identity order
    w = ref.records(cols, mode, None, p['bucket'], p['centres'])[rec0:].tobytes()
    buf, view = guarded(len(w), 3)
    ctx.dev_ksplat_records(dev, view, mode, None, bucket, centres, rec0=rec0)
    assert first_difference(view.cpu().numpy().tobytes(), w) is None and guards_intact(buf, 3, len(w))


# ---- plans ---------------------------------------------------------------------------------------------------
PLAN_TABLES = kc.plan_tables()


def check_plan(ctx, cols, block):
    want = ref.plan(cols, block)
    got = ctx.dev_ksplat_plan(to_dev(cols), block)
    assert (got['full'], got['partial'], got['clamped']) == (want['full'], want['partial'], want['clamped'])
    assert np.array_equal(u32(got['order']), want['order'])
    assert np.array_equal(u32(got['bucket']), want['bucket'])
    assert np.array_equal(got['centres'].cpu().numpy().view(np.uint32), want['centres'].view(np.uint32))
    assert np.array_equal(u32(got['partial_sizes']), want['partial_sizes'])
    return want


@pytest.mark.parametrize('name', list(PLAN_TABLES))
def test_dev_ksplat_plan_known_tables(ctx, name):
    cols, block, expected = PLAN_TABLES[name]
    want = check_plan(ctx, cols, block)
    if expected:
        assert (want['full'], want['partial'], want['partial_sizes'].tolist(), want['clamped']) == expected


def test_dev_ksplat_plan_many_tiles(ctx):
    """70,000 rows in 300 cells: more than one sort tile, multi-block scans, all three key ranges"""
    rng = np.random.default_rng(70)
    n = 70_000
    cell = rng.integers(0, 300, n)
    xyz = np.stack([cell % 10, (cell // 10) % 6, cell // 60], 1) * 2.0 + rng.uniform(0.01, 1.99, (n, 3))
    xyz[0] = 0.0
    cols = kc.with_positions(n, xyz[:, 0], xyz[:, 1], xyz[:, 2])
    want = check_plan(ctx, cols, 2.0)
    assert want['full'] + want['partial'] > 300 and want['partial'] <= 300
    # float64 and integer position columns take the same path
    cols2 = [(k, a.astype(np.float64) if k == 'x' else np.floor(a * 3).astype(np.int32) if k == 'y' else a) for k, a in cols]
    check_plan(ctx, cols2, 2.0)


# ---- the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('set_name,name', kc.KSPLAT_CASES, ids=[n for _, n in kc.KSPLAT_CASES])
def test_fixture_read_and_reencoded_on_the_device(ctx, tmp_path, set_name, name):
    """read_ksplat_dev's columns re-encoded on the device through the file's own bucket table: equal to
    the restatement, whose bytes tests/test_write_ksplat_cpu.py ties to the file's outside the classes"""
    data, cols, _ = kc.fixture(set_name, name)
    path = tmp_path / 'in.ksplat'
    path.write_bytes(data)
    dev = ctx.read_ksplat_dev(str(path))
    for sec in kc.sections(data, cols):
        m = len(sec['records'])
        finite = np.isfinite(sec['sh_min']) and np.isfinite(sec['sh_max']) and sec['sh_min'] < sec['sh_max']
        if sec['mode'] == 2 and not finite:
            continue  # a range the writer refuses (its harmonics are the class sh_range)
        table = [(k, dev[k][sec['row0']:sec['row0'] + m]) for k, _ in sec['table']]
        for (k, a), (_, t) in zip(sec['table'], table):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), k
        want = kc.restated(sec)
        buf, view = guarded(want.size, 1)
        ctx.dev_ksplat_records(table, view, sec['mode'], None, i32(sec['bucket']), torch.from_numpy(sec['centres']).cuda(),
                               block_size=sec['block'], quant_range=sec['quant'],
                               sh_min=sec['sh_min'] if sec['mode'] == 2 else -1.5, sh_max=sec['sh_max'] if sec['mode'] == 2 else 1.5)
        assert first_difference(view.cpu().numpy().tobytes(), want.tobytes()) is None
        assert guards_intact(buf, 1, want.size)
        allowed = np.zeros(want.shape, bool)
        for m_ in kc.excused(sec).values():
            allowed |= m_
        assert not ((want != sec['records']) & ~allowed).any()


# ---- round trip on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_written_file_reads_back_on_the_device(ctx, tmp_path, mode):
    cols = kc.image_table(700, 8, seed=41)
    path = tmp_path / 'out.ksplat'
    rows, size, clamped = ctx.dev_ksplat_file(to_dev(cols), str(path), mode, -1, 5.0, -1.0, 1.25)
    want, _ = ref.image(cols, mode, -1, 5.0, -1.0, 1.25)
    assert (rows, size, clamped) == (700, len(want), 0) and path.read_bytes() == want
    back, n, nsh = oracle_readers.read_ksplat(want)      # what the rules predict, through the oracle reader
    got = ctx.read_ksplat_dev(str(path))
    assert (n, nsh) == (700, 24) and list(got) == sh.reader_columns(24)
    for k, w in zip(got, back):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), w.view(np.uint32)), k
    p = ref.plan(cols, 5.0)
    t = dict(cols)
    if mode == 0:
        assert np.array_equal(got['x'].cpu().numpy(), t['x'][p['order']])
    else:
        c = np.abs(p['centres'][p['bucket'], 0].astype(np.float64))
        x = got['x'].cpu().numpy().astype(np.float64)
        assert (np.abs(x - t['x'][p['order']]) <= 5.0 / 2 / 32767 / 2 + c * 2.0 ** -23 + np.abs(x) * 2.0 ** -23).all()


# ---- the ring and the one-call forms -------------------------------------------------------------------------------
def test_ksplat_file_streams_through_the_ring(ctx, tmp_path, monkeypatch):
    """50,001 rows at degree 3, mode 1 (5.7 MB of image) through 1 MiB slots, from a descriptor's position"""
    monkeypatch.setenv('ST_CPF_SLOT_MB', '1')
    cols = kc.ordinary(np.random.default_rng(50), 50_001, 15, spread=10.0)
    want, want_clamped = ref.image(cols, 1)
    assert len(want) > 5 << 20
    p = tmp_path / 'out.ksplat'
    fd = os.open(str(p), os.O_RDWR | os.O_CREAT, 0o644)
    try:
        os.write(fd, b'P' * 37 + b'\xee' * (len(want) + 4097))   # a longer file is cut
        os.lseek(fd, 37, os.SEEK_SET)
        assert ctx.dev_ksplat_file(to_dev(cols), fd) == (50_001, len(want), want_clamped)
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want) == os.fstat(fd).st_size
    finally:
        os.close(fd)
    assert p.read_bytes()[:37] == b'P' * 37 and first_difference(p.read_bytes()[37:], want) is None
    buf, view = guarded(len(want))
    assert ctx.dev_ksplat_image(to_dev(cols), view) == (len(want), want_clamped)
    assert first_difference(view.cpu().numpy().tobytes(), want) is None


@pytest.mark.parametrize('case', ['config1', 'filters_sh3'])
def test_one_call_forms_with_actions(ctx, tmp_path, case):
    """the expectation: the restatement applied to ctx.process's table; from a host table and a .ply file"""
    make, acts = CHAINS[case]
    cols = make(np.random.default_rng(len(case)))
    processed = ctx.process([(k, a.copy()) for k, a in cols], acts)
    m = len(processed[0][1])
    C = ot.band_coeffs({k for k, _ in processed})
    src = tmp_path / 'in.ply'
    src.write_bytes(write_ply_ref.write_ply(['the input'], [('vertex', cols)]))
    keep = [(k, a.copy()) for k, a in cols]
    for mode, degree in ((1, -1), (2, 0), (0, -1)):
        want, want_clamped = ref.image(processed, mode, degree, 5.0, -1.5, 1.5)
        a, b = tmp_path / f'a{mode}.ksplat', tmp_path / f'b{mode}.ksplat'
        assert ctx.ksplat_file(cols, acts, str(a), mode, degree) == (m, len(want), want_clamped)
        assert ctx.ply_ksplat_file(str(src), acts, str(b), mode, degree) == (m, len(want), want_clamped)
        assert a.read_bytes() == want == b.read_bytes()
        assert sh.ksplat_layout(want) == (m, 0 if degree == 0 else 3 * C)
    assert all(x.tobytes() == y.tobytes() for (_, x), (_, y) in zip(cols, keep))


# ---- refusals, each of which leaves the output untouched --------------------------------------------------------------
@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_file_forms_refuse_descriptor(ctx, tmp_path, flags):
    cols = kc.image_table(100, 3)
    p = tmp_path / 'keep.bin'
    p.write_bytes(b'keep')
    fd = os.open(str(p), flags)
    try:
        for call in (lambda: ctx.dev_ksplat_file(to_dev(cols), fd), lambda: ctx.ksplat_file(cols, [], fd)):
            with pytest.raises(sh.StError) as e:
                call()
            assert e.value.code == sh.ST_ERR_ARG
    finally:
        os.close(fd)
    assert p.read_bytes() == b'keep'


def test_argument_errors_leave_the_output_untouched(ctx, tmp_path):
    cols = kc.image_table(100, 3)
    dev = to_dev(cols)
    want, _ = ref.image(cols, 1)
    buf, view = guarded(len(want) + 64)
    p = tmp_path / 'keep.bin'
    p.write_bytes(b'keep')
    plan = ref.plan(cols)
    order, bucket, centres = i32(plan['order']), i32(plan['bucket']), torch.from_numpy(plan['centres']).cuda()

    def refused(call, text, code=sh.ST_ERR_ARG):
        with pytest.raises(sh.StError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert int(buf.min()) == FILL == int(buf.max())
        assert p.read_bytes() == b'keep'

    def every_form(text, cols=cols, dev=dev, **kw):
        refused(lambda: ctx.dev_ksplat_image(dev, view, **kw), text)
        refused(lambda: ctx.dev_ksplat_file(dev, str(p), **kw), text)
        refused(lambda: ctx.ksplat_file(cols, [], str(p), **kw), text)
    for missing in ('z', 'scale_1', 'rot_3'):
        every_form('missing column ' + missing, [c for c in cols if c[0] != missing], [c for c in dev if c[0] != missing])
        refused(lambda: ctx.dev_ksplat_plan([c for c in dev if c[0] != missing]), 'missing column ' + missing)
    every_form('mode', mode=3)
    every_form('mode', mode=-1)
    every_form('degree', degree=2)
    every_form('degree', degree=-2)
    for b in (0.0, -1.0, float('inf'), float('nan'), 1e-60):
        every_form('block_size', block_size=b)
        refused(lambda: ctx.dev_ksplat_plan(dev, b), 'block_size')
    for lo, hi in ((0.0, 1.5), (-1.5, 0.0), (2.0, 1.0), (float('nan'), 1.0), (-1.0, float('inf'))):
        every_form('sh_min', mode=2, sh_min=lo, sh_max=hi)
    empty = [(k, a[:0]) for k, a in cols]
    dempty = to_dev(empty)
    refused(lambda: ctx.dev_ksplat_image(dempty, view), 'no rows')
    refused(lambda: ctx.dev_ksplat_file(dempty, str(p)), 'no rows')
    refused(lambda: ctx.dev_ksplat_plan(dempty), 'no rows')
    refused(lambda: ctx.ksplat_file(empty, [], str(p)), '')
    refused(lambda: ctx.ksplat_file(cols, [{'kind': 'filterByValue', 'columnName': 'x', 'comparator': 'gt', 'value': 1e9}],
                                    str(p)), 'no rows')
    refused(lambda: ctx.dev_ksplat_image(dev, view[:len(want) - 1]), 'too small')      # a cap one byte short
    refused(lambda: ctx.dev_ksplat_records(dev, view, 1, order, bucket, centres, rec0=98, nrec=3), 'outside the table')
    refused(lambda: ctx.dev_ksplat_records(dev, view, 1, order, None, None), 'bucket tables')
    refused(lambda: ctx.dev_ksplat_records(dev, view, 1, order, bucket, centres, quant_range=0), 'quant_range')
    refused(lambda: ctx.dev_ksplat_records(dev, view, 3, order, bucket, centres), 'mode')
    # the file's own range stands in for mode 2 only
    size, _ = ctx.dev_ksplat_image(dev, view, 1, sh_min=0.0, sh_max=0.0)
    assert size == len(want) and first_difference(view[:size].cpu().numpy().tobytes(), want) is None
