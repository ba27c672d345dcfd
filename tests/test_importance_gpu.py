"""include/st_abi.h's "importance, decimation and crops" on the GPU against the restatement of
tests/importance_ref.py on every table of tests/importance_cases.py: scores as uint64 bit patterns,
row indices and processed columns exactly.  Device columns start one element past a 256-byte
boundary (the general kernels) as well as on one (the 16-byte loads).  Then each action through
Context.process, decimate after a transform and a filterNaN, one end-to-end form per family, the
group's per-rank slices (box and sphere run there, decimate and orderByImportance are refused), and
the argument errors."""
import numpy as np
import pytest
import torch

import importance_cases as ic
import importance_ref as ref
import oracle
import splat_hip as sh
import write_ply_ref

pytestmark = pytest.mark.gpu

SCORE_CASES = sorted(ic.score_cases())
CROP_CASES = sorted(ic.crop_cases())
TORCH_TYPE = {np.dtype(n): t for n, t in (
    (np.int8, torch.int8), (np.uint8, torch.uint8), (np.int16, torch.int16), (np.uint16, torch.uint16),
    (np.int32, torch.int32), (np.uint32, torch.uint32), (np.float32, torch.float32), (np.float64, torch.float64))}


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch copies are ordered with the library's kernels
    yield c
    c.close()


def to_dev(cols, offset=0):
    """[(name, tensor)]: each column `offset` elements past the start of an allocation of its own"""
    out = []
    for k, a in cols:
        a = np.ascontiguousarray(a)
        shift = offset * a.itemsize
        raw = torch.empty(a.nbytes + shift, dtype=torch.uint8, device='cuda')
        assert raw.data_ptr() % 256 == 0
        raw[shift:].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
        out.append((k, raw[shift:].view(TORCH_TYPE[a.dtype])))
    return out


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('case', SCORE_CASES)
def test_scores_order_and_top(ctx, case, offset):
    c, want = ic.score_cases()[case], ic.expected(case)
    dev = to_dev(c['cols'], offset)
    n = len(c['cols'][0][1])
    got = ctx.dev_importance(dev).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want['scores'].view(np.uint64))
    assert np.array_equal(u32(ctx.dev_importance_order(dev)), want['order'])
    for m in c['counts']:  # counts beyond n are cut to n
        rows = u32(ctx.dev_importance_top(dev, m))
        print(case, offset, m, len(rows))
        assert np.array_equal(rows, want['top'][min(m, n)]), (case, m)
    for f in c['fractions']:
        m = ref.decimate_rows(n, fraction=f)
        assert np.array_equal(u32(ctx.dev_importance_top(dev, m)), want['top'][m]), (case, f)


def test_host_column_forms(ctx):
    c, want = ic.score_cases()['mixed_types'], ic.expected('mixed_types')
    assert np.array_equal(ctx.importance(c['cols']).view(np.uint64), want['scores'].view(np.uint64))
    assert np.array_equal(ctx.importance_order(dict(c['cols'])), want['order'])


def full_table(cols, seed):
    """the case's columns among others the actions must carry along"""
    rng = np.random.default_rng(seed)
    n = len(cols[0][1])
    return [('id', np.arange(n, dtype=np.uint32))] + list(cols) + [('f_dc_0', rng.normal(0, 1, n).astype(np.float32)),
                                                                   ('w', rng.normal(0, 1, n))]


def same_table(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize('case', [c for c in SCORE_CASES if c != ic.BIG])
def test_decimate_and_order_through_process(ctx, case):
    c, want = ic.score_cases()[case], ic.expected(case)
    n = len(c['cols'][0][1])
    if n == 0:  # a DataTable has rows; the device calls above cover n = 0
        return
    cols = full_table(c['cols'], 5)
    acts = [{'kind': 'decimate', 'count': m} for m in c['counts'][:4]] + [{'kind': 'decimate', 'fraction': f} for f in c['fractions']]
    for act in acts:
        m = ref.decimate_rows(n, act.get('count'), act.get('fraction'))
        rows = want['top'][m]
        same_table(ctx.process(cols, [act]), [(k, a[rows]) for k, a in cols])
    same_table(ctx.process(cols, [{'kind': 'orderByImportance'}]), [(k, a[want['order']]) for k, a in cols])


@pytest.mark.parametrize('twin', ['as_given', 'float64'])
@pytest.mark.parametrize('case', CROP_CASES)
def test_box_and_sphere(ctx, case, twin):
    """each box and sphere through Context.process.  The chain uploads host columns onto 16-byte
    boundaries, so float32 x / y / z take the wide kernel; their float64 twin (the same JS numbers,
    hence the same verdicts) and the mixed-type table take the general one"""
    c, want = ic.crop_cases()[case], ic.expected_crop(case)
    n = c['n']
    if n == 0:  # a DataTable has rows
        return
    cols = [('id', np.arange(n, dtype=np.uint32))] + [
        (k, a.astype(np.float64) if twin == 'float64' and a.dtype == np.float32 else a) for k, a in c['cols']]
    for (lo, hi), rows in zip(c['boxes'], want['boxes']):
        got = ctx.process(cols, [{'kind': 'filterBox', 'min': lo, 'max': hi}])
        assert np.array_equal(got[0][1], rows), (case, lo, hi)
        same_table(got, [(k, a[rows]) for k, a in cols])
    for (ce, r), rows in zip(c['spheres'], want['spheres']):
        got = ctx.process(cols, [{'kind': 'filterSphere', 'center': ce, 'radius': r}])
        assert np.array_equal(got[0][1], rows), (case, ce, r)


def sh1_table(n, seed):
    """an SH-1 splat table with NaN rows (in opacity and a scale: the positions stay unique)"""
    rng = np.random.default_rng(seed)
    cols = {a: rng.normal(0, 3, n).astype(np.float32) for a in 'xyz'}
    for i in range(3):
        cols[f'f_dc_{i}'] = rng.normal(0, 1, n).astype(np.float32)
    for i in range(9):
        cols[f'f_rest_{i}'] = rng.normal(0, 0.1, n).astype(np.float32)
    cols['opacity'] = rng.normal(0, 2, n).astype(np.float32)
    for i in range(3):
        cols[f'scale_{i}'] = (rng.random(n) * 5 - 7).astype(np.float32)
    for i in range(4):
        cols[f'rot_{i}'] = rng.normal(0, 1, n).astype(np.float32)
    cols['opacity'][rng.permutation(n)[:300]] = np.nan
    cols['scale_1'][rng.permutation(n)[:200]] = np.nan
    return cols


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    cols = sh1_table(20_000, 51)
    path = tmp_path_factory.mktemp('importance') / 'in.ply'
    path.write_bytes(write_ply_ref.write_ply([], [('vertex', list(cols.items()))]))
    return cols, str(path)


def test_decimate_after_transform_and_filter_nan(ctx, scene):
    """the fraction is taken of the rows at that point in the chain"""
    cols, _ = scene
    head = [{'kind': 'scale', 'value': 2.0}, {'kind': 'filterNaN'}]
    mid = oracle.process(list(cols.items()), head)
    assert len(mid[0][1]) < 20_000
    for act in ({'kind': 'decimate', 'fraction': 0.25}, {'kind': 'decimate', 'count': 19_000}):
        want = ref.apply(mid, act)
        assert len(want[0][1]) == ref.decimate_rows(len(mid[0][1]), act.get('count'), act.get('fraction'))
        same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], head + [act]), want)
    # and one list with every new kind in it
    acts = [{'kind': 'filterBox', 'min': (-4, -4, -4), 'max': (4, 4, 4)}, {'kind': 'filterSphere', 'center': (0, 0, 0), 'radius': 4.5},
            {'kind': 'decimate', 'fraction': 0.5}, {'kind': 'orderByImportance'}]
    want = list(cols.items())
    for act in acts:
        want = ref.apply(want, act)
    assert 0 < len(want[0][1]) < 10_000
    same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], acts), want)


def test_ply_to_splat_in_importance_order(ctx, scene, tmp_path):
    """`in.ply --orderByImportance out.splat`: .splat keeps x / y / z exactly, so each written row is
    found in the input; the rows are in importance order, judged on the scores of the rows written"""
    cols, path = scene
    out = str(tmp_path / 'out.splat')
    m, _ = ctx.ply_splat_file(path, [{'kind': 'orderByImportance'}], out)
    assert m == 20_000
    back = ctx.read_splat(out)
    at = {(x.tobytes(), y.tobytes(), z.tobytes()): i for i, (x, y, z) in enumerate(zip(cols['x'], cols['y'], cols['z']))}
    assert len(at) == 20_000
    written = np.array([at[(x.tobytes(), y.tobytes(), z.tobytes())] for x, y, z in zip(back['x'], back['y'], back['z'])], np.uint32)
    assert np.array_equal(written, ref.order(ref.scores(cols)))


def test_ply_to_compressed_ply_with_sphere_and_decimate(ctx, scene):
    cols, path = scene
    acts = [{'kind': 'filterSphere', 'center': (0.5, 0, 0), 'radius': 5.0}, {'kind': 'decimate', 'fraction': 0.5}]
    want = list(cols.items())
    for act in acts:
        want = ref.apply(want, act)
    m, chunk, vertex, shb = ctx.ply_compressed_ply(path, acts)
    wm, wchunk, wvertex, wsh = ctx.compressed_ply(want, [])
    assert m == wm == len(want[0][1]) and 1000 < m < 10_000
    assert chunk.tobytes() == wchunk.tobytes() and vertex.tobytes() == wvertex.tobytes() and shb.tobytes() == wsh.tobytes()


def test_sog_bundle_with_box_and_decimate(ctx, scene):
    cols, _ = scene
    acts = [{'kind': 'filterBox', 'min': (-3, -3, -3), 'max': (3, 3, 3)}, {'kind': 'decimate', 'count': 4000}]
    want = list(cols.items())
    for act in acts:
        want = ref.apply(want, act)
    assert len(want[0][1]) == 4000
    draws = np.random.default_rng(13).random(1 << 18)
    got, used = ctx.sog_bundle_process(list(cols.items()), acts, 2, draws, 0x6000, 0x5a21)
    wbytes, wused = ctx.sog_bundle(dict(want), 2, draws, 0x6000, 0x5a21)
    assert used == wused and got == wbytes


def test_group_runs_the_crops_per_rank_and_refuses_the_global_kinds(ctx):
    a, b = sh1_table(6_000, 61), sh1_table(5_001, 62)
    for t in (a, b):  # writeSog's k-means refuses non-finite rows
        t['opacity'] = np.nan_to_num(t['opacity'])
        t['scale_1'] = np.nan_to_num(t['scale_1'], nan=-3.0)
    acts = [[{'kind': 'filterBox', 'min': (-4, -4, -4), 'max': (4, 4, 4)}],
            [{'kind': 'translate', 'value': (0.5, 0, 0)}, {'kind': 'filterSphere', 'center': (0.5, 0, 0), 'radius': 5.0}]]
    draws = np.random.default_rng(14).random(1 << 18)
    pa = ctx.process([(k, v.copy()) for k, v in a.items()], acts[0])
    pb = ctx.process([(k, v.copy()) for k, v in b.items()], acts[1])
    same_table(pa, ref.apply(list(a.items()), acts[0][0]))
    assert 0 < len(pb[0][1]) < 5_001
    want, wused = ctx.sog_bundle(dict(oracle.combine([pa, pb])), 2, draws, 0x6000, 0x5a21)
    g = sh.Group([0] * 2, host_staged=True)
    try:
        got, used = g.sog_bundle_process([a, b], acts, 2, draws, 0x6000, 0x5a21)
        assert used == wused and got == want
        for bad in ({'kind': 'decimate', 'count': 100}, {'kind': 'orderByImportance'}):
            with pytest.raises(sh.StError) as e:
                g.sog_bundle_process([a, b], [acts[0], [bad]], 2, draws, 0x6000, 0x5a21)
            assert e.value.code == sh.ST_ERR_UNSUPPORTED
    finally:
        g.close()


def test_argument_errors(ctx):
    cols = full_table(ic.score_cases()['len_257']['cols'], 7)
    for act in ({'kind': 'decimate', 'count': 2.5}, {'kind': 'decimate', 'count': -1}, {'kind': 'decimate', 'count': float('nan')},
                {'kind': 'decimate', 'count': 2.0 ** 53}, {'kind': 'decimate', 'fraction': 1.0000001},
                {'kind': 'decimate', 'fraction': float('nan')}, {'kind': 'decimate', 'fraction': -0.1}):
        with pytest.raises(sh.StError) as e:
            ctx.process(cols, [act])
        assert e.value.code == sh.ST_ERR_ARG, act
    bare = [(k, a) for k, a in cols if k != 'opacity']
    for act in ({'kind': 'decimate', 'count': 10}, {'kind': 'orderByImportance'}):
        with pytest.raises(sh.StError) as e:
            ctx.process(bare, [act])
        assert e.value.code == sh.ST_ERR_ARG and 'opacity' in str(e.value)
    dev = to_dev(bare)
    for call in (ctx.dev_importance, ctx.dev_importance_order, lambda d: ctx.dev_importance_top(d, 5)):
        with pytest.raises(sh.StError) as e:
            call(dev)
        assert e.value.code == sh.ST_ERR_ARG
    # the context still works
    same_table(ctx.process(cols, [{'kind': 'decimate', 'count': 257}]), cols)
