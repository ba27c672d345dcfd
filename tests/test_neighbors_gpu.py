"""include/st_abi.h's "neighbour distances and outliers" on the GPU against the restatement of
tests/neighbors_ref.py on every table of tests/neighbors_cases.py: dist_k as uint64 bit patterns for
k in {1, 8, 32} (every k on the lattice), device columns on a 256-byte boundary and one element past
it, 64-row leaves and ST_KNN_LEAF=4 (deep trees over small tables).  Then filterOutliers through
Context.process in both modes, after a transform and a filterNaN, the scene with floaters, one
end-to-end form per family, the group's refusal, the argument errors and the search's statistics."""
import math

import numpy as np
import pytest
import torch

import neighbors_cases as nc
import neighbors_ref as ref
import oracle
import splat_hip as sh
import write_ply_ref

pytestmark = pytest.mark.gpu

CASES = sorted(nc.cases())
TORCH_TYPE = {np.dtype(n): t for n, t in (
    (np.int8, torch.int8), (np.uint8, torch.uint8), (np.int16, torch.int16), (np.uint16, torch.uint16),
    (np.int32, torch.int32), (np.uint32, torch.uint32), (np.float32, torch.float32), (np.float64, torch.float64))}
INF, NAN = math.inf, math.nan


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


def set_leaf(monkeypatch, leaf):
    if leaf:
        monkeypatch.setenv('ST_KNN_LEAF', str(leaf))
    else:
        monkeypatch.delenv('ST_KNN_LEAF', raising=False)
    return leaf or 64


@pytest.mark.parametrize('leaf', [0, 4])
@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('case', CASES)
def test_distances(ctx, case, offset, leaf, monkeypatch):
    c, want = nc.cases()[case], nc.expected(case)
    L = set_leaf(monkeypatch, leaf)
    dev = to_dev(c['cols'], offset)
    placed = int(ref.placed(c['cols']).sum())
    for k in c['ks']:
        got = ctx.dev_neighbor_dist(dev, k).cpu().numpy()
        st = ctx.last_neighbor_stats()
        bad = np.flatnonzero(got.view(np.uint64) != want[k].view(np.uint64))
        print(case, offset, L, k, st, 'rows that differ:', len(bad), bad[:5], got[bad[:5]], want[k][bad[:5]])
        assert len(bad) == 0, (case, k)
        assert (st['rows'], st['placed'], st['leaves']) == (c['n'], placed, (placed + L - 1) // L)


def test_an_invalid_leaf_size_falls_back_to_the_default(ctx, monkeypatch):
    c, want = nc.cases()['levels_513'], nc.expected('levels_513')
    dev = to_dev(c['cols'])
    for text in ('3', '65', '0', '-4', 'abc', '16x', ''):
        monkeypatch.setenv('ST_KNN_LEAF', text)
        got = ctx.dev_neighbor_dist(dev, 8).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want[8].view(np.uint64))
        assert ctx.last_neighbor_stats()['leaves'] == 9, text
    monkeypatch.setenv('ST_KNN_LEAF', '16')
    ctx.dev_neighbor_dist(dev, 8)
    assert ctx.last_neighbor_stats()['leaves'] == 33


def test_host_column_forms(ctx):
    c, want = nc.cases()['mixed_types'], nc.expected('mixed_types')
    for k in nc.KS:
        assert np.array_equal(ctx.neighbor_dist(c['cols'], k).view(np.uint64), want[k].view(np.uint64))
    c, want = nc.cases()['nonfinite'], nc.expected('nonfinite')
    assert np.array_equal(ctx.neighbor_dist(dict(c['cols']), 8).view(np.uint64), want[8].view(np.uint64))


def test_stats_show_pruning(ctx):
    c = nc.cases()[nc.BIG]
    n = c['n']
    dev = to_dev(c['cols'])
    for k in nc.KS:
        ctx.dev_neighbor_dist(dev, k)
        st = ctx.last_neighbor_stats()
        print(k, st, 'pairs per query', st['pairs'] / n, 'nodes per leaf', st['nodes'] / st['leaves'])
        assert st['pairs'] < n * (n - 1)
        assert (st['rows'], st['placed'], st['leaves']) == (n, n, (n + 63) // 64)


def full_table(cols, seed):
    """the case's columns among others the action must carry along"""
    rng = np.random.default_rng(seed)
    n = len(cols[0][1])
    return [('id', np.arange(n, dtype=np.uint32))] + list(cols) + [('f_dc_0', rng.normal(0, 1, n).astype(np.float32)),
                                                                   ('w', rng.normal(0, 1, n))]


def same_table(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def actions_for(dist, k):
    fin = dist[np.isfinite(dist)]
    mid = float(np.median(fin)) if len(fin) else 1.0
    return [{'kind': 'filterOutliers', 'k': k, 'sigma': s} for s in (1.0, 0.0, -0.5, INF)] + \
           [{'kind': 'filterOutliers', 'k': k, 'distance': d} for d in (mid, math.nextafter(mid, -INF), 0.0, INF, -INF)]


@pytest.mark.parametrize('case', [c for c in CASES if c not in (nc.BIG, 'lattice', 'levels_4097')])
def test_filter_outliers_through_process(ctx, case):
    c, want = nc.cases()[case], nc.expected(case)
    if c['n'] == 0:  # a DataTable has rows; the device call above covers n = 0
        return
    first = {}
    for k, a in c['cols']:
        first.setdefault(k, a)
    cols = full_table([(k, first[k]) for k in 'xyz'], 5)
    for k in (8, 32):
        for act in actions_for(want[k], k):
            rows = ref.kept(want[k], ref.SIGMA, act['sigma']) if 'sigma' in act else ref.kept(want[k], ref.DISTANCE, act['distance'])
            got = ctx.process(cols, [act])
            assert np.array_equal(got[0][1], rows), (case, act)
            same_table(got, [(name, a[rows]) for name, a in cols])
    # k defaults to 8
    rows = ref.kept(want[8], ref.SIGMA, 0.5)
    assert np.array_equal(ctx.process(cols, [{'kind': 'filterOutliers', 'sigma': 0.5}])[0][1], rows)


def splat_table(seed):
    """the scene's positions in a table every writer takes, with NaN rows (in x and in opacity)"""
    cols, cluster = nc.scene()
    rng = np.random.default_rng(seed)
    n = len(cluster)
    t = dict(cols)
    for i in range(3):
        t[f'f_dc_{i}'] = rng.normal(0, 1, n).astype(np.float32)
    t['opacity'] = rng.normal(0, 2, n).astype(np.float32)
    for i in range(3):
        t[f'scale_{i}'] = (rng.random(n) * 5 - 7).astype(np.float32)
    for i in range(4):
        t[f'rot_{i}'] = rng.normal(0, 1, n).astype(np.float32)
    t['opacity'][rng.permutation(n)[:150]] = np.nan
    t['x'] = t['x'].copy()
    t['x'][rng.permutation(n)[:100]] = np.nan
    return t


@pytest.fixture(scope='module')
def scene_file(tmp_path_factory):
    cols = splat_table(81)
    path = tmp_path_factory.mktemp('neighbors') / 'in.ply'
    path.write_bytes(write_ply_ref.write_ply([], [('vertex', list(cols.items()))]))
    return cols, str(path)


def test_scene_with_floaters(ctx):
    """4,000 cluster rows and 40 floaters: k = 8, sigma = 1 keeps exactly the cluster"""
    cols, cluster = nc.scene()
    table = full_table(cols, 9)
    d = ref.dist_k(cols, 8)
    assert np.array_equal(ctx.neighbor_dist(cols, 8).view(np.uint64), d.view(np.uint64))
    rows = ref.kept(d, ref.SIGMA, 1.0)
    assert np.array_equal(rows, np.flatnonzero(cluster)) and len(rows) == 4000
    same_table(ctx.process(table, [{'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}]), [(k, a[rows]) for k, a in table])


def test_after_a_transform_and_filter_nan(ctx, scene_file):
    """the statistics are those of the rows at that point in the chain"""
    cols, _ = scene_file
    head = [{'kind': 'scale', 'value': 2.0}, {'kind': 'translate', 'value': (0.5, 0, -1)}, {'kind': 'filterNaN'}]
    mid = oracle.process(list(cols.items()), head)
    assert len(mid[0][1]) == 4040 - 250 + len(np.flatnonzero(np.isnan(cols['x']) & np.isnan(cols['opacity'])))
    for act in ({'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}, {'kind': 'filterOutliers', 'k': 3, 'distance': 0.4}):
        want = ref.apply(mid, act)
        assert 1000 < len(want[0][1]) < len(mid[0][1])
        same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], head + [act]), want)
    # without the filterNaN the rows without a position go too, the other NaN rows stay
    act = {'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}
    want = ref.apply(list(cols.items()), act)
    assert np.isnan(want[6][1]).sum() > 100 and not np.isnan(want[0][1]).any()
    same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], [act]), want)
    # two in a row: the second sees the first's survivors
    acts = [act, {'kind': 'filterOutliers', 'k': 4, 'sigma': 2.0}]
    want = ref.apply(ref.apply(list(cols.items()), acts[0]), acts[1])
    same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], acts), want)


def test_ply_to_compressed_ply_and_splat(ctx, scene_file, tmp_path):
    cols, path = scene_file
    acts = [{'kind': 'filterNaN'}, {'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}]
    want = ref.apply(oracle.process(list(cols.items()), acts[:1]), acts[1])
    m, chunk, vertex, shb = ctx.ply_compressed_ply(path, acts)
    wm, wchunk, wvertex, wsh = ctx.compressed_ply(want, [])
    assert m == wm == len(want[0][1]) and 3000 < m < 4000
    assert chunk.tobytes() == wchunk.tobytes() and vertex.tobytes() == wvertex.tobytes() and shb.tobytes() == wsh.tobytes()
    a, b = str(tmp_path / 'a.splat'), str(tmp_path / 'b.splat')
    ma, _ = ctx.ply_splat_file(path, acts, a)
    mb, _ = ctx.splat_file(want, [], b)
    assert ma == mb == m
    with open(a, 'rb') as fa, open(b, 'rb') as fb:
        assert fa.read() == fb.read()


def test_group_refuses_the_kind(ctx):
    rng = np.random.default_rng(91)
    tabs = []
    for n in (3000, 2001):
        t = {k: rng.normal(0, 1, n).astype(np.float32) for k in ('x', 'y', 'z', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
                                                                   'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3')}
        tabs.append(t)
    draws = np.random.default_rng(14).random(1 << 16)
    g = sh.Group([0] * 2, host_staged=True)
    try:
        for bad in ({'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}, {'kind': 'filterOutliers', 'distance': 0.5}):
            with pytest.raises(sh.StError) as e:
                g.sog_bundle_process(tabs, [[{'kind': 'filterNaN'}], [bad]], 2, draws, 0x6000, 0x5a21)
            assert e.value.code == sh.ST_ERR_UNSUPPORTED
    finally:
        g.close()


def test_argument_errors(ctx):
    cols = full_table(nc.cases()['len_257']['cols'], 7)
    for act in ({'kind': 'filterOutliers', 'k': 0, 'sigma': 1.0}, {'kind': 'filterOutliers', 'k': 33, 'sigma': 1.0},
                {'kind': 'filterOutliers', 'k': -1, 'distance': 1.0}, {'kind': 'filterOutliers', 'k': 2.5, 'sigma': 1.0},
                {'kind': 'filterOutliers', 'k': 8, 'sigma': NAN}, {'kind': 'filterOutliers', 'k': 8, 'distance': NAN}):
        with pytest.raises(sh.StError) as e:
            ctx.process(cols, [{'kind': 'filterNaN'}, act])
        assert e.value.code == sh.ST_ERR_ARG, act
    bare = [(k, a) for k, a in cols if k != 'z']
    with pytest.raises(sh.StError) as e:
        ctx.process(bare, [{'kind': 'filterOutliers', 'sigma': 1.0}])
    assert e.value.code == sh.ST_ERR_ARG and 'column z' in str(e.value)
    dev = to_dev(bare)
    with pytest.raises(sh.StError) as e:
        ctx.dev_neighbor_dist(dev, 8)
    assert e.value.code == sh.ST_ERR_ARG and 'column z' in str(e.value)
    dev = to_dev(cols)
    for k in (0, 33, -5):
        with pytest.raises(sh.StError) as e:
            ctx.dev_neighbor_dist(dev, k)
        assert e.value.code == sh.ST_ERR_ARG
    # the context still works
    want = nc.expected('len_257')[8]
    assert np.array_equal(ctx.dev_neighbor_dist(dev, 8).cpu().numpy().view(np.uint64), want.view(np.uint64))
    same_table(ctx.process(cols, [{'kind': 'filterOutliers', 'k': 8, 'distance': INF}]), cols)
