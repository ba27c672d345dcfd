"""include/st_abi.h's "clusters" without a GPU: st_clusters.h's serial host form -- placed, d2, link, the
sequential union-find, the verdicts, the argument rules and the two bounds the kernels call, in a
stand-alone program (tests/native/clusters_cpu_check.cpp, built plainly and with AddressSanitizer and
UndefinedBehaviorSanitizer, and run directly) -- against the restatement of tests/clusters_ref.py on
every small table of tests/clusters_cases.py.  Labels, sizes and rows are compared exactly.  The device
must give the same (tests/test_clusters_gpu.py)."""
import math

import numpy as np
import pytest

import clusters_cases as cc
import clusters_ref as ref
import neighbors_cases as nc
import splat_hip as sh

SMALL = sorted(c for c in cc.cases() if c not in cc.BIG)
INF, NAN = math.inf, math.nan


def filters(size):
    """(mode, cluster_min) pairs around a size column"""
    big = int(size.max()) if len(size) else 0
    return [(ref.MIN_SIZE, float(m)) for m in (0, 1, 2, big, big + 1)] + [(ref.LARGEST, 0.0), (ref.LARGEST, NAN)]


@pytest.mark.parametrize('case', SMALL)
def test_labels_sizes_and_kept_rows_equal_the_restatement(case, tmp_path):
    c, want = cc.cases()[case], cc.expected(case)
    queries = []
    for r in c['radii']:
        queries.append(('clusters', r))
        queries += [('filter', r, mode, m) for mode, m in filters(want[r][1])]
    for sanitize in ((False,) if c['n'] > 1000 else (True, False)):  # 8 x 10^6 pairs a radius: the optimised build only
        got = iter(cc.native(c['cols'], queries, tmp_path, sanitize))
        for r in c['radii']:
            label, size = next(got)
            assert np.array_equal(label, want[r][0]) and np.array_equal(size, want[r][1]), (case, r)
            for mode, m in filters(want[r][1]):
                assert np.array_equal(next(got), ref.kept(want[r][1], mode, m)), (case, r, mode, m)


def test_the_line_cases():
    """the 20,000-row expectations are the native program's: what they must be by construction"""
    label, size = cc.expected('line')[cc.LINE_RADIUS]
    assert np.all(label == 0) and np.all(size == 20_000)
    for case in ('line_gap', 'line_gap_bent'):
        c = cc.cases()[case]
        label, size = cc.expected(case)[cc.LINE_RADIUS]
        assert np.all(size == 10_000) and len(ref.partition(label)) == 2
        first = dict(c['cols'])
        side = (first['x'] < 2500.0) if case == 'line_gap' else (first['x'] < 0.0)
        assert len(set(label[side])) == 1 and len(set(label[~side])) == 1
        assert label[side][0] == np.flatnonzero(side)[0] and label[~side][0] == np.flatnonzero(~side)[0]
    # the gap of the straight line is float32's next value after the radius, the bent line's is float64's
    x = np.sort(dict(cc.cases()['line_gap']['cols'])['x'])
    steps = np.diff(x)
    assert steps.max() == float(np.nextafter(np.float32(0.25), np.float32(INF))) and (steps == 0.25).sum() == 19_998
    assert -dict(cc.cases()['line_gap_bent']['cols'])['x'].min() == math.nextafter(0.25, INF)


def test_a_twin_of_another_type_gives_the_same_labels():
    a, b = cc.expected('len_513_f64twin'), cc.expected('len_513')
    for r in cc.cases()['len_513']['radii']:
        assert np.array_equal(a[r][0], b[r][0]) and np.array_equal(a[r][1], b[r][1])


def test_argument_rules(tmp_path):
    """radius >= 0 and no NaN; the two modes only; cluster_min as decimate's count; x, y and z present"""
    cols = cc.cases()['len_65']['cols']
    queries, want = [], []
    for radius, ok in ((NAN, False), (-1.0, False), (-INF, False), (-1e-300, False), (0.0, True), (-0.0, True),
                       (INF, True), (1e-200, True), (1e200, True)):
        queries += [('clusters', radius), ('filter', radius, ref.MIN_SIZE, 2.0), ('filter', radius, ref.LARGEST, 0.0)]
        want += [ok] * 3
    for m, ok in ((2.5, False), (-1.0, False), (NAN, False), (INF, False), (2.0 ** 53, False), (2.0 ** 53 - 1, True),
                  (0.0, True), (-0.0, True), (65.0, True)):
        queries.append(('filter', 0.5, ref.MIN_SIZE, m))
        want.append(ok)
    for mode in (2, -1, 2 ** 31 - 1):
        queries.append(('filter', 0.5, mode, 1.0))
        want.append(False)
    queries.append(('filter', 0.5, ref.LARGEST, 2.5))  # the largest mode does not read cluster_min
    want.append(True)
    for sanitize in (True, False):
        got = cc.native(cols, queries, tmp_path, sanitize)
        assert [not isinstance(g, int) for g in got] == want
    for missing in 'xyz':
        bare = [(k, a) for k, a in cols if k != missing]
        got = cc.native(bare, [('clusters', 0.5), ('filter', 0.5, ref.MIN_SIZE, 1.0), ('filter', INF, ref.LARGEST, 0.0)],
                        tmp_path, True)
        assert got == [cc.REFUSED] * 3, missing


def bound_triples(rng, m):
    """m x (node min, node max, query min, query max, a point of the node, a point of the query) over
    magnitudes where squares overflow (1e154) and underflow (1e-160), ordinary ones and mixtures, with
    degenerate boxes (a point, a flat box) among them"""
    scale = rng.choice([1e154, 1e-160, 1.0, 1e-3, 3e38, 1e300], (m, 1))
    mix = rng.random((m, 1)) < 0.2  # per-axis magnitudes: one axis overflows, another underflows
    scale = np.where(mix, rng.choice([1e154, 1e-160, 1.0], (m, 3)), scale)

    def boxes():
        a, b = rng.normal(0, 1, (m, 3)) * scale, rng.normal(0, 1, (m, 3)) * scale
        flat = rng.random((m, 3)) < 0.25
        b = np.where(flat, a, b)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        f = rng.random((m, 3))
        f = np.where(rng.random((m, 3)) < 0.3, np.round(f), f)  # often a corner
        p = np.clip(lo + (hi - lo) * f, lo, hi)
        p = np.where(np.isfinite(p), p, lo)
        return lo, hi, p
    nlo, nhi, pn = boxes()
    qlo, qhi, pq = boxes()
    near = rng.random((m, 1)) < 0.3  # overlapping and touching boxes
    shift = np.where(near, (nlo - qlo) * np.round(rng.random((m, 3))), 0.0)
    qlo, qhi, pq = qlo + shift, qhi + shift, pq + shift
    lo, hi = np.minimum(qlo, qhi), np.maximum(qlo, qhi)
    return np.concatenate([nlo, nhi, lo, hi], 1), pn, np.clip(pq, lo, hi)


def test_far_bound_is_an_upper_and_box_bound_a_lower_bound_of_the_computed_d2(tmp_path):
    rng = np.random.default_rng(85)
    b, pn, pq = bound_triples(rng, 100_000)
    assert np.all(pn >= b[:, 0:3]) and np.all(pn <= b[:, 3:6]) and np.all(pq >= b[:, 6:9]) and np.all(pq <= b[:, 9:12])
    (got,) = cc.native(cc.cases()['len_1']['cols'], [('bounds', b)], tmp_path, True)
    far, near = got[:, 0], got[:, 1]
    with np.errstate(all='ignore'):
        d = pq - pn
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert not np.isnan(far).any() and not np.isnan(near).any() and not np.isnan(d2).any()
    assert np.all(near >= 0) and np.all(near <= d2) and np.all(d2 <= far)
    # the hard magnitudes are there: overflowed and underflowed squares, and bounds that are attained
    tiny = (d2 > 0) & (d2 < 2.2250738585072014e-308)  # a subnormal sum of squares
    assert (d2 == INF).sum() > 1000 and (far == INF).sum() > 1000 and tiny.sum() > 1000
    assert (near == d2).sum() > 1000 and (far == d2).sum() > 1000 and ((near > 0) & (near < INF)).sum() > 10_000
    # a box against itself: the clique test's bound covers every pair inside
    self_b = np.concatenate([b[:, 0:6], b[:, 0:6]], 1)
    (got,) = cc.native(cc.cases()['len_1']['cols'], [('bounds', self_b)], tmp_path, False)
    lo, hi = b[:, 0:3], b[:, 3:6]
    with np.errstate(all='ignore'):
        d = hi - lo
        diag = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.array_equal(got[:, 0], diag) and np.all(got[:, 1] == 0)


def test_expected_values_the_rules_name():
    """the restatement itself on the values the rules spell out"""
    two = cc.expected('len_2_linked')
    assert two[5.0][0].tolist() == [0, 0] and two[5.0][1].tolist() == [2, 2]  # at exactly the radius: linked
    assert two[math.nextafter(5.0, 0)][0].tolist() == [0, 1] and two[0.0][1].tolist() == [1, 1]
    one = cc.expected('len_2_one_placed')[1.0]
    assert one[0].tolist() == [ref.NONE, 1] and one[1].tolist() == [0, 1]
    for r, (label, size) in cc.expected('none_placed').items():
        assert np.all(label == ref.NONE) and np.all(size == 0) and len(ref.kept(size, ref.LARGEST)) == 0
        assert len(ref.kept(size, ref.MIN_SIZE, 0)) == 0
    la = cc.expected('lattice')
    placed = la[0.125][0] != ref.NONE
    assert len(set(la[0.125][0][placed])) == 1 and placed.sum() == 216 - 27
    assert np.all(la[math.nextafter(0.125, 0)][1][placed] == 1)
    co = cc.expected('coincident_groups')[0.0][1]
    assert sorted(np.unique(co).tolist()) == [1, 2, 64, 65, 200] and (co == 1).sum() == 101
    ov = cc.expected('overflow_f64')
    n_placed = int((ov[INF][0] != ref.NONE).sum())
    assert np.all(ov[INF][1][ov[INF][0] != ref.NONE] == n_placed)
    x, y, z = (np.abs(a) for _, a in cc.cases()['overflow_f64']['cols'])
    far = (np.maximum(np.maximum(x, y), z) > 1e100) & (ov[INF][0] != ref.NONE)
    assert far.sum() > 20 and ov[1.0][1][far].max() == 2 and ov[1e150][1][far].max() == 2  # two of them coincide
    assert np.array_equal(ov[1.7e308][1], ov[INF][1])  # r2 overflows: as +Infinity
    # min-index labels; ties for the largest keep every tied component
    size = np.array([2, 3, 0, 3, 2, 3, 3, 3, 3], np.uint32)
    assert ref.kept(size, ref.LARGEST).tolist() == [1, 3, 5, 6, 7, 8] and ref.kept(size, ref.MIN_SIZE, 3).tolist() == [1, 3, 5, 6, 7, 8]
    assert ref.kept(size, ref.MIN_SIZE, 0).tolist() == [0, 1, 3, 4, 5, 6, 7, 8] and len(ref.kept(size, ref.MIN_SIZE, 4)) == 0


def test_scene_radius_leaves_the_cluster_and_debris():
    """the scene of the GPU tests at radius 0.3: one large component, small ones and singletons"""
    label, size = cc.scene_expected()
    _, cluster = nc.scene()
    assert size.max() > 2000 and (size == 1).sum() > 40 and len(ref.partition(label)) > 50
    assert np.all(cluster[ref.kept(size, ref.LARGEST)])


def test_make_actions_and_exports():
    a = sh.make_actions([{'kind': 'filterClusters', 'radius': 0.5, 'minSize': 10},
                         {'kind': 'filterClusters', 'radius': INF, 'keep': 'largest'}, {'kind': 'filterNaN'}])
    assert [x.kind for x in a] == [sh.ACTION_FILTER_CLUSTERS] * 2 + [sh.ACTION_FILTER_NAN]
    assert (a[0].cluster_radius, a[0].cluster_mode, a[0].cluster_min) == (0.5, sh.CLUSTER_MIN_SIZE, 10.0)
    assert (a[1].cluster_radius, a[1].cluster_mode) == (INF, sh.CLUSTER_LARGEST)
    assert (sh.ACTION_FILTER_CLUSTERS, sh.CLUSTER_MIN_SIZE, sh.CLUSTER_LARGEST) == (11, 0, 1)
    for bad in ({'kind': 'filterClusters', 'radius': 1.0}, {'kind': 'filterClusters', 'minSize': 2},
                {'kind': 'filterClusters', 'radius': 1.0, 'minSize': 2, 'keep': 'largest'},
                {'kind': 'filterClusters', 'radius': 1.0, 'keep': 'smallest'}):
        with pytest.raises(ValueError):
            sh.make_actions([bad])
    assert 'filterClusters' in sh.FILTER_KINDS
    # a zero-filled action of an older kind is what it was: the new fields come last
    z = sh.make_actions([{'kind': 'filterOutliers', 'sigma': 1.0}])[0]
    assert (z.cluster_radius, z.cluster_mode, z.cluster_min) == (0.0, 0, 0.0)
    assert sh.Action.cluster_radius.offset > sh.Action.outlier_value.offset
    for name in ('st_dev_clusters', 'st_ctx_last_cluster_stats'):
        assert name in sh.EXPORTS and getattr(sh.lib(), name)
    for name in ('dev_clusters', 'clusters', 'last_cluster_stats'):
        assert callable(getattr(sh.Context, name))
