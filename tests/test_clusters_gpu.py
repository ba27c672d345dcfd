"""include/st_abi.h's "clusters" on the GPU against the restatement of tests/clusters_ref.py (the
stand-alone program of st_clusters.h's serial form for the 20,000-row lines) on every table of
tests/clusters_cases.py: labels and sizes as uint32, equal bit for bit, with 64-row leaves and
ST_KNN_LEAF=4 (deep trees over small tables).  Then the independence of the result from the tree, the
row order and the call, the cost guard of the clique path, filterClusters through Context.process in
both modes, in a chain, a one-call file form, the group's refusal and the argument errors."""
import math

import numpy as np
import pytest
import torch

import clusters_cases as cc
import clusters_ref as ref
import neighbors_cases as nc
import neighbors_ref as nref
import oracle
import splat_hip as sh
import write_ply_ref

pytestmark = pytest.mark.gpu

CASES = sorted(cc.cases())
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


def to_dev(cols):
    out = []
    for k, a in cols:
        a = np.ascontiguousarray(a)
        raw = torch.empty(max(a.nbytes, 1), dtype=torch.uint8, device='cuda')[:a.nbytes]
        raw.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)))
        out.append((k, raw.view(TORCH_TYPE[a.dtype])))
    return out


def host(t):
    return t.cpu().numpy().view(np.uint32)


def set_leaf(monkeypatch, leaf):
    if leaf:
        monkeypatch.setenv('ST_KNN_LEAF', str(leaf))
    else:
        monkeypatch.delenv('ST_KNN_LEAF', raising=False)
    return leaf or 64


def check(ctx, dev, radius, want, what, L=None):
    label, size = (host(t) for t in ctx.dev_clusters(dev, radius))
    st = ctx.last_cluster_stats()
    bad = np.flatnonzero((label != want[0]) | (size != want[1]))
    print(what, radius, st, 'rows that differ:', len(bad), bad[:5], label[bad[:5]], want[0][bad[:5]], size[bad[:5]],
          want[1][bad[:5]])
    assert len(bad) == 0, (what, radius)
    placed = int((want[0] != ref.NONE).sum())
    assert (st['rows'], st['placed']) == (len(label), placed)
    assert st['components'] == len(np.unique(want[0][want[0] != ref.NONE])) and st['largest'] == (want[1].max() if len(label) else 0)
    assert st['unions'] == placed - st['components']  # every successful hook takes one tree away
    if L:
        assert st['leaves'] == (placed + L - 1) // L
    return st


@pytest.mark.parametrize('leaf', [0, 4])
@pytest.mark.parametrize('case', CASES)
def test_labels_and_sizes(ctx, case, leaf, monkeypatch):
    """every size and every special table at L = 64, and at L = 4 (len_257: four box levels)"""
    c, want = cc.cases()[case], cc.expected(case)
    L = set_leaf(monkeypatch, leaf)
    dev = to_dev(c['cols'])
    for r in c['radii']:
        st = check(ctx, dev, r, want[r], (case, L), L)
        if case == 'len_257_all_placed' and leaf == 4:
            assert st['levels'] == 4
        if r == INF and st['placed']:
            assert st['pairs'] == 0 and st['nodes'] == st['leaves']  # the root is a clique: one box test a wave


def test_independent_of_the_tree_the_row_order_and_the_call(ctx, monkeypatch):
    cols, _ = nc.scene()
    want = cc.scene_expected()
    dev = to_dev(cols)
    for leaf in (4, 16, 64):
        set_leaf(monkeypatch, leaf)
        check(ctx, dev, cc.SCENE_RADIUS, want, ('scene', leaf), leaf)
    check(ctx, dev, cc.SCENE_RADIUS, want, 'scene again', 64)  # a second call on the same context
    perm = np.random.default_rng(87).permutation(len(cols[0][1]))
    label, size = ctx.clusters([(k, a[perm]) for k, a in cols], cc.SCENE_RADIUS)
    assert np.array_equal(size, want[1][perm])  # size permutes with the rows
    moved = {frozenset(int(perm[i]) for i in s) for s in ref.partition(label)}
    assert moved == ref.partition(want[0])  # the partition is equal as a set of sets
    assert np.array_equal(label, np.array([np.flatnonzero(label == v)[0] if v != ref.NONE else v for v in label], np.uint32))


def test_host_column_forms(ctx):
    for case in ('mixed_types', 'len_65'):
        c, want = cc.cases()[case], cc.expected(case)
        r = c['radii'][0]
        label, size = ctx.clusters(c['cols'] if case == 'mixed_types' else dict(c['cols']), r)
        assert label.dtype == np.uint32 and np.array_equal(label, want[r][0]) and np.array_equal(size, want[r][1])
    # either output may be NULL
    c, want = cc.cases()['len_513'], cc.expected('len_513')
    r = c['radii'][0]
    t = sh.make_ttable(to_dev(c['cols']))
    import ctypes
    for which in (0, 1):
        out = torch.empty(c['n'], dtype=torch.uint32, device='cuda')
        args = [None, None]
        args[which] = sh._ptr(out)
        sh.check(sh.lib().st_dev_clusters(ctx.h, ctypes.byref(t), ctypes.c_double(r), *args))
        assert np.array_equal(host(out), want[r][which])


def test_cost_guard_of_the_clique_path(ctx):
    """65,536 coincident rows are one clique: every wave tests the root once and no pair at all.  A
    quadratic path (4.3e9 pairs) or a leaf-only shortcut (about 18 box tests a row) fails the cap"""
    n = 65_536
    dev = to_dev(nc.table(np.tile([0.5, -0.25, 2.0], (n, 1))))
    for radius in (0.0, 1.0):
        label, size = (host(t) for t in ctx.dev_clusters(dev, radius))
        st = ctx.last_cluster_stats()
        print(radius, st)
        assert np.all(label == 0) and np.all(size == n)
        assert (st['placed'], st['components'], st['largest'], st['leaves']) == (n, 1, n, 1024)
        assert st['pairs'] + st['nodes'] <= 8 * st['placed']
        assert (st['pairs'], st['nodes']) == (0, 1024)


def full_table(cols, seed):
    """the case's columns among others the action must carry along"""
    rng = np.random.default_rng(seed)
    first = {}
    for k, a in cols:
        first.setdefault(k, a)
    n = len(first['x'])
    return [('id', np.arange(n, dtype=np.uint32)), ('x', first['x']), ('flag', rng.integers(-100, 100, n).astype(np.int8)),
            ('y', first['y']), ('z', first['z']), ('f_dc_0', rng.normal(0, 1, n).astype(np.float32)), ('w', rng.normal(0, 1, n))]


def same_table(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def actions_for(size, radius):
    big = int(size.max())
    return [{'kind': 'filterClusters', 'radius': radius, 'minSize': m} for m in (0, 1, 2, big, big + 1)] + \
           [{'kind': 'filterClusters', 'radius': radius, 'keep': 'largest'}]


def tie_table():
    """two components of 50 rows tie for the largest, one of 20 and 30 singletons, shuffled"""
    rng = np.random.default_rng(89)
    p = np.concatenate([rng.normal(0, 0.01, (50, 3)), [10, 0, 0] + rng.normal(0, 0.01, (50, 3)),
                        [0, 10, 0] + rng.normal(0, 0.01, (20, 3)), 100.0 + 5.0 * np.arange(30)[:, None] * np.ones((1, 3))])
    return nc.table(rng.permutation(p)), 0.2


@pytest.mark.parametrize('case', ['len_2', 'len_65', 'len_513', 'lattice', 'coincident_groups', 'mixed_types', 'none_placed',
                                  'tie', 'scene'])
def test_filter_clusters_through_process(ctx, case):
    if case == 'tie':
        cols, r = tie_table()
        size = ref.clusters(cols, r)[1]
        assert sorted(np.unique(size, return_counts=True)[1].tolist()) == [20, 30, 100]
        assert len(ref.kept(size, ref.LARGEST)) == 100  # both tied components
    elif case == 'scene':
        cols, r = nc.scene()[0], cc.SCENE_RADIUS
        size = cc.scene_expected()[1]
    else:
        cols, r = cc.cases()[case]['cols'], cc.cases()[case]['radii'][0]
        size = cc.expected(case)[r][1]
    table = full_table(cols, 5)
    for act in actions_for(size, r):
        rows = ref.kept_for(size, act)
        got = ctx.process(table, [act])
        assert np.array_equal(got[0][1], rows), (case, act)
        same_table(got, [(name, a[rows]) for name, a in table])


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
    path = tmp_path_factory.mktemp('clusters') / 'in.ply'
    path.write_bytes(write_ply_ref.write_ply([], [('vertex', list(cols.items()))]))
    return cols, str(path)


def test_in_a_chain(ctx, scene_file):
    """after translate and filterNaN, then after filterOutliers: the components are those of the rows at
    that point of the chain"""
    cols, _ = scene_file
    head = [{'kind': 'scale', 'value': 2.0}, {'kind': 'translate', 'value': (0.5, 0, -1)}, {'kind': 'filterNaN'}]
    mid = oracle.process(list(cols.items()), head)
    for act in ({'kind': 'filterClusters', 'radius': 0.6, 'keep': 'largest'}, {'kind': 'filterClusters', 'radius': 0.5, 'minSize': 4}):
        want = ref.apply(mid, act)
        assert 1000 < len(want[0][1]) < len(mid[0][1])
        same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], head + [act]), want)
    # without the filterNaN the rows without a position go too, the other NaN rows stay
    act = {'kind': 'filterClusters', 'radius': 0.3, 'minSize': 2}
    want = ref.apply(list(cols.items()), act)
    assert np.isnan(want[6][1]).sum() > 50 and not np.isnan(want[0][1]).any()
    same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], [act]), want)
    # filterOutliers, then filterClusters on its survivors
    acts = [{'kind': 'filterNaN'}, {'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0},
            {'kind': 'filterClusters', 'radius': 0.25, 'keep': 'largest'}]
    step = nref.apply(oracle.process(list(cols.items()), acts[:1]), acts[1])
    want = ref.apply(step, acts[2])
    assert 500 < len(want[0][1]) < len(step[0][1])
    same_table(ctx.process([(k, a.copy()) for k, a in cols.items()], acts), want)


def test_ply_to_splat_file(ctx, scene_file, tmp_path):
    cols, path = scene_file
    acts = [{'kind': 'filterNaN'}, {'kind': 'filterClusters', 'radius': 0.3, 'keep': 'largest'}]
    want = ref.apply(oracle.process(list(cols.items()), acts[:1]), acts[1])
    got = ctx.process([(k, a.copy()) for k, a in cols.items()], acts)
    same_table(got, want)
    a, b = str(tmp_path / 'a.splat'), str(tmp_path / 'b.splat')
    ma, _ = ctx.ply_splat_file(path, acts, a)
    mb, _ = ctx.splat_file(got, [], b)
    assert ma == mb == len(want[0][1]) and 1000 < ma < 3800
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
        for bad in ({'kind': 'filterClusters', 'radius': 0.5, 'minSize': 3}, {'kind': 'filterClusters', 'radius': 0.5, 'keep': 'largest'}):
            with pytest.raises(sh.StError) as e:
                g.sog_bundle_process(tabs, [[{'kind': 'filterNaN'}], [bad]], 2, draws, 0x6000, 0x5a21)
            assert e.value.code == sh.ST_ERR_UNSUPPORTED
    finally:
        g.close()


def test_argument_errors(ctx):
    cols = full_table(cc.cases()['len_257']['cols'], 7)
    before = [(k, a.copy()) for k, a in cols]

    def raw(radius, mode, cluster_min):  # what make_actions cannot spell: another mode
        acts = sh.make_actions([{'kind': 'filterClusters', 'radius': radius, 'minSize': 0}])
        acts[0].cluster_mode, acts[0].cluster_min = mode, cluster_min
        return acts
    assert sh.make_actions([{'kind': 'filterClusters', 'radius': 1.0, 'minSize': 2.5}])[0].cluster_min == 2.5
    for act in ({'kind': 'filterClusters', 'radius': NAN, 'minSize': 1}, {'kind': 'filterClusters', 'radius': -1.0, 'minSize': 1},
                {'kind': 'filterClusters', 'radius': -INF, 'keep': 'largest'}, {'kind': 'filterClusters', 'radius': NAN, 'keep': 'largest'},
                {'kind': 'filterClusters', 'radius': 1.0, 'minSize': 2.5}, {'kind': 'filterClusters', 'radius': 1.0, 'minSize': -1},
                {'kind': 'filterClusters', 'radius': 1.0, 'minSize': NAN}, {'kind': 'filterClusters', 'radius': 1.0, 'minSize': INF},
                {'kind': 'filterClusters', 'radius': 1.0, 'minSize': 2.0 ** 53}):
        with pytest.raises(sh.StError) as e:
            ctx.process(cols, [{'kind': 'filterNaN'}, act])
        assert e.value.code == sh.ST_ERR_ARG, act
        same_table(cols, before)
    dev = to_dev(cols)
    import ctypes
    n = len(cols[0][1])
    out = [(k, np.empty(n, a.dtype)) for k, a in cols]
    ts, td, m = sh.make_ttable(cols), sh.make_ttable(out, n), ctypes.c_uint64(0)
    for mode in (2, -1):
        with pytest.raises(sh.StError) as e:
            sh.check(sh.lib().st_process(ctx.h, ctypes.byref(ts), raw(1.0, mode, 1.0), ctypes.c_int32(1), ctypes.byref(td),
                                         ctypes.byref(m)))
        assert e.value.code == sh.ST_ERR_ARG, mode
        same_table(cols, before)
    bare = [(k, a) for k, a in cols if k != 'z']
    with pytest.raises(sh.StError) as e:
        ctx.process(bare, [{'kind': 'filterClusters', 'radius': 1.0, 'keep': 'largest'}])
    assert e.value.code == sh.ST_ERR_ARG and 'column z' in str(e.value)
    with pytest.raises(sh.StError) as e:
        ctx.dev_clusters(to_dev(bare), 1.0)
    assert e.value.code == sh.ST_ERR_ARG and 'column z' in str(e.value)
    for radius in (NAN, -0.5, -INF):
        with pytest.raises(sh.StError) as e:
            ctx.dev_clusters(dev, radius)
        assert e.value.code == sh.ST_ERR_ARG
    same_table(cols, before)
    # the context still works; every row kept: the table stays as it is
    want = cc.expected('len_257')
    r = cc.cases()['len_257']['radii'][0]
    check(ctx, dev, r, want[r], 'after the errors')
    placed_only = [(k, a[want[r][0] != ref.NONE]) for k, a in cols]
    same_table(ctx.process(placed_only, [{'kind': 'filterClusters', 'radius': INF, 'minSize': 1}]), placed_only)
    same_table(ctx.process(placed_only, [{'kind': 'filterClusters', 'radius': 0.0, 'minSize': 0}]), placed_only)
