"""The column summary on the GPU (st_dev_summary, st_summary; include/st_abi.h, "column summary")
against the restatement of tests/summary_ref.py on every table of tests/summary_cases.py: field by
field as uint64 bit patterns (NaN as NaN, the sign of zero counts).  Every case runs three ways --
the defaults, ST_SUM_EXACT=1 (every column down the superaccumulator) and ST_SUM_FLUSH=64 (a
normalisation every 64 additions) -- and the path counters show which way it went.  Device columns
start one element past a 256-byte boundary as well as on one (the vector loads' heads and tails).
The whole path: a seeded 100,000-row SH-1 table with NaN / Infinity rows gives the same bits from the
device columns of its .ply file, from the host columns, and from the rows in Morton order."""
import numpy as np
import pytest
import torch

import splat_hip as sh
import summary_cases as sc
import summary_ref as ref
import write_ply_ref

pytestmark = pytest.mark.gpu

CASES = sorted(sc.tables())


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch copies are ordered with the library's kernels
    yield c
    c.close()


@pytest.fixture(params=sc.MODES, ids=[m[0] for m in sc.MODES])
def mode(request, monkeypatch):
    name, exact, flush = request.param
    monkeypatch.delenv('ST_SUM_EXACT', raising=False)
    monkeypatch.delenv('ST_SUM_FLUSH', raising=False)
    if exact:
        monkeypatch.setenv('ST_SUM_EXACT', exact)
    if flush:
        monkeypatch.setenv('ST_SUM_FLUSH', flush)
    return name


def to_dev(cols, offset=0):
    """[(name, tensor)]: each column `offset` elements past the start of an allocation of its own"""
    out = []
    for k, a in cols:
        a = np.ascontiguousarray(a)
        shift = offset * a.itemsize
        raw = torch.empty(a.nbytes + shift, dtype=torch.uint8, device='cuda')
        assert raw.data_ptr() % 256 == 0
        raw[shift:].copy_(torch.from_numpy(a.view(np.uint8)))
        out.append((k, raw[shift:].view(TORCH_TYPE[a.dtype])))
    return out


TORCH_TYPE = {np.dtype(n): t for n, t in (
    (np.int8, torch.int8), (np.uint8, torch.uint8), (np.int16, torch.int16), (np.uint16, torch.uint16),
    (np.int32, torch.int32), (np.uint32, torch.uint32), (np.float32, torch.float32), (np.float64, torch.float64))}


def as_list(cols, got):
    return got if isinstance(got, list) else [got[k] for k, _ in cols]


def groups(case):
    """a case's columns as tables: [(columns of one length, their expected summaries)], in column order"""
    by_len = {}
    for col, want in zip(sc.tables()[case], sc.expected(case)):
        cols, wants = by_len.setdefault(len(col[1]), ([], []))
        cols.append(col)
        wants.append(want)
    return list(by_len.values())


def check(case, cols, wants, got, what):
    got = as_list(cols, got)
    assert len(got) == len(cols)
    for (name, _), g, w in zip(cols, got, wants):
        print(what, case, name, g)
        bad = ref.same(g, w)
        assert bad is None, (what, case, name, bad)


def check_stats(ctx, cols, mode):
    st = ctx.summary_stats()
    print(st)
    fast = sum(ref.fast_path(a) for _, a in cols)
    assert st['columns'] == len(cols) and st['fast'] + st['general'] == len(cols)
    if mode == 'exact':
        assert st['general'] == len(cols)
    else:
        assert st['fast'] == fast
    assert st['flush'] == (64 if mode == 'flush64' else 1 << 30)
    if mode != 'flush64':
        assert st['normalisations'] == 0
    return st


@pytest.mark.parametrize('case', CASES)
def test_summaries_equal_the_restatement(ctx, case, mode):
    offsets = (0, 1) if case.startswith('len_') or case in ('sum', 'median') else (1,)
    norms = 0
    for cols, wants in groups(case):
        for offset in offsets:
            check(case, cols, wants, ctx.dev_summary(to_dev(cols, offset)), f'dev+{offset}')
            norms += check_stats(ctx, cols, mode)['normalisations']
        check(case, cols, wants, ctx.summary(cols), 'host')
        check_stats(ctx, cols, mode)
    if mode == 'flush64' and case in ('len_4097', 'sum_u32_max', 'median'):
        assert norms > 0


def test_duplicate_names_give_a_list(ctx):
    cols = sc.tables()['same_name']
    got = ctx.dev_summary(to_dev(cols))
    assert isinstance(got, list) and len(got) == 2
    assert isinstance(ctx.dev_summary(to_dev(sc.tables()['len_3'])), dict)
    text = sh.summary_text(cols, got)
    assert text == ref.text([k for k, _ in cols], sc.expected('same_name'))


# ---- the whole path ----------------------------------------------------------------------------------
def scene():
    if not _SCENE:
        rng = np.random.default_rng(100_000)
        n = 100_000
        names = ['x', 'y', 'z', 'f_dc_0', 'f_dc_1', 'f_dc_2'] + [f'f_rest_{i}' for i in range(9)] + \
            ['opacity', 'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3']
        cols = [(k, rng.normal(0, 1 if k[0] != 's' else 4, n).astype(np.float32)) for k in names]
        bad = rng.choice(n, n // 1000, replace=False)  # 0.1 % of the rows: NaN of both signs, +-Infinity
        fill = sc.f32_bits([0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000])
        for i, r in enumerate(bad):
            for k, a in cols[3 + i % 5::5]:  # the positions stay finite: the rows are ordered by them below
                a[r] = fill[(i + len(k)) % 4]
        _SCENE.append(cols)
    return _SCENE[0]


_SCENE = []


def test_file_host_and_morton_order_agree(ctx, tmp_path, mode):
    """dev_summary of the .ply file's device columns == summary of the host columns == dev_summary of
    the same rows in Morton order, bit for bit: no result depends on the rows' order"""
    cols = scene()
    src = tmp_path / 'scene.ply'
    src.write_bytes(write_ply_ref.write_ply([], [('vertex', cols)]))
    _, els = ctx.read_ply_dev(str(src))
    (_, dev), = els
    assert list(dev) == [k for k, _ in cols]
    from_file = ctx.dev_summary(dev)
    st = check_stats(ctx, cols, mode)
    if mode == 'flush64':
        assert st['normalisations'] > 1000
    from_host = ctx.summary(cols)
    d = dict(cols)
    order = torch.from_numpy(ctx.morton_order(d['x'], d['y'], d['z']).astype(np.int64)).cuda()
    assert not np.array_equal(order.cpu().numpy(), np.arange(len(order)))
    permuted = ctx.dev_summary({k: t[order] for k, t in dev.items()})
    for k, _ in cols:
        assert from_file[k].nan_count + from_file[k].inf_count == from_file[k].rows - np.isfinite(d[k]).sum()
        assert ref.same(from_host[k], from_file[k]) is None, ('host', k, ref.same(from_host[k], from_file[k]))
        assert ref.same(permuted[k], from_file[k]) is None, ('morton', k, ref.same(permuted[k], from_file[k]))
    assert sum(from_file[k].nan_count + from_file[k].inf_count for k, _ in cols) >= 100
    for k in ('x', 'opacity', 'f_rest_3'):  # and the restatement on three of the columns
        assert ref.same(from_file[k], ref.summarize(d[k])) is None, (k, ref.same(from_file[k], ref.summarize(d[k])))


# ---- errors ------------------------------------------------------------------------------------------
class Shifted:
    """a device column whose pointer is `shift` bytes past a tensor's"""

    def __init__(self, t, shift):
        self.t, self.dtype, self.shift = t, t.dtype, shift

    def data_ptr(self):
        return self.t.data_ptr() + self.shift

    def __len__(self):
        return len(self.t) - 1


def test_errors(ctx):
    with pytest.raises(sh.StError) as e:
        ctx.dev_summary([])
    assert e.value.code == sh.ST_ERR_ARG
    with pytest.raises(sh.StError) as e:
        ctx.summary([])
    assert e.value.code == sh.ST_ERR_ARG
    good = torch.zeros(16, dtype=torch.float32, device='cuda')
    for dtype, shift in ((torch.float32, 2), (torch.float64, 4), (torch.int16, 1)):
        t = torch.zeros(16, dtype=dtype, device='cuda')
        with pytest.raises(sh.StError) as e:
            ctx.dev_summary([('fine', good), ('the_odd_one', Shifted(t, shift))])
        assert e.value.code == sh.ST_ERR_ARG and 'the_odd_one' in str(e.value) and 'fine' not in str(e.value)
    host = np.zeros(67, np.uint8)[3:].view(np.float32)
    if host.ctypes.data % 4:
        with pytest.raises(sh.StError) as e:
            ctx.summary([('host_odd', host)])
        assert e.value.code == sh.ST_ERR_ARG and 'host_odd' in str(e.value)
    # a one-byte type is aligned anywhere
    one = torch.arange(40, dtype=torch.uint8, device='cuda')
    assert ctx.dev_summary([('b', one[3:])])['b'].median == 21.0
