"""include/st_abi.h's "neighbour distances and outliers" without a GPU: st_neighbors.h's serial host form
-- placed, d2, the k best, the threshold, the verdict and the argument rules the kernels call, in a
stand-alone program (tests/native/neighbors_cpu_check.cpp, built plainly and with AddressSanitizer
and UndefinedBehaviorSanitizer, and run directly) -- against the restatement of tests/neighbors_ref.py
on every table of tests/neighbors_cases.py.  Distances are compared as uint64 bit patterns, rows
exactly.  The device must give the same (tests/test_neighbors_gpu.py)."""
import math

import numpy as np
import pytest

import neighbors_cases as nc
import neighbors_ref as ref
import splat_hip as sh

CASES = sorted(nc.cases())
INF, NAN = math.inf, math.nan


def thresholds(dist):
    """(mode, value) pairs around a distance column: sigmas of either sign and size, distances on,
    below and above the values"""
    fin = dist[np.isfinite(dist)]
    mid = float(np.median(fin)) if len(fin) else 1.0
    return [(ref.SIGMA, s) for s in (1.0, 0.0, -0.5, 3.0, INF, -INF)] + \
           [(ref.DISTANCE, d) for d in (mid, math.nextafter(mid, -INF), 0.0, -1.0, INF, -INF)]


@pytest.mark.parametrize('case', CASES)
def test_distances_and_kept_rows_equal_the_restatement(case, tmp_path):
    c, want = nc.cases()[case], nc.expected(case)
    ks = [k for k in c['ks'] if k in (1, 8, 32)] if case != 'lattice' else c['ks']
    queries = []
    for k in ks:
        queries.append(('dist', k))
        queries += [('outliers', k, mode, v) for mode, v in thresholds(want[k])]
    for sanitize in ((False,) if case == nc.BIG else (True, False)):  # 4 x 10^8 pairs a k: the optimised build only
        got = iter(nc.native(c['cols'], queries, tmp_path, sanitize))
        for k in ks:
            d = next(got)
            assert np.array_equal(d.view(np.uint64), want[k].view(np.uint64)), (case, k)
            for mode, v in thresholds(want[k]):
                rows = next(got)
                assert np.array_equal(rows, ref.kept(want[k], mode, v)), (case, k, mode, v)


def test_big_equals_numpy_on_a_sample():
    """BIG's expectation is the native program's; 500 of its rows against numpy (the rows' pairs with
    all 20,000), beside the small cases where the two agree on every row"""
    c, want = nc.cases()[nc.BIG], nc.expected(nc.BIG)
    x, y, z = ref.xyz(c['cols'])
    rows = np.random.default_rng(72).permutation(c['n'])[:500]
    dx, dy, dz = x[rows, None] - x[None, :], y[rows, None] - y[None, :], z[rows, None] - z[None, :]
    d2 = (dx * dx + dy * dy) + dz * dz
    d2[np.arange(500), rows] = np.inf
    for k in c['ks']:
        assert np.array_equal(np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1]).view(np.uint64),
                              want[k][rows].view(np.uint64)), k


def test_a_twin_of_another_type_gives_the_same_bits():
    twins = [(case, c['twin']) for case, c in nc.cases().items() if 'twin' in c]
    assert len(twins) == 2
    for case, of in twins:
        a, b = nc.expected(case), nc.expected(of)
        assert all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in nc.KS), case


def test_argument_rules(tmp_path):
    """k in 1..32; sigma and distance anything but NaN; the two modes only"""
    cols = nc.cases()['len_65']['cols']
    queries, want = [], []
    for k in (0, -1, 33, 2 ** 31 - 1, -2 ** 31):
        queries.append(('outliers', k, ref.SIGMA, 1.0))
        want.append(False)
    for k in (1, 32):
        queries.append(('outliers', k, ref.DISTANCE, 0.5))
        want.append(True)
    for mode in (ref.SIGMA, ref.DISTANCE):
        queries.append(('outliers', 8, mode, NAN))
        want.append(False)
        for v in (INF, -INF, -0.0, 1e308, -3.5):
            queries.append(('outliers', 8, mode, v))
            want.append(True)
    for mode in (2, -1):
        queries.append(('outliers', 8, mode, 1.0))
        want.append(False)
    for sanitize in (True, False):
        got = nc.native(cols, queries, tmp_path, sanitize)
        assert [not isinstance(g, int) for g in got] == want


def test_box_bound_is_a_lower_bound_of_the_computed_d2(tmp_path):
    """the prune's claim, on the tables where rounding is hardest: for boxes cut from a table, no
    computed d2 between a row of one and a row of the other is below the bound the program computes"""
    rng = np.random.default_rng(73)
    for case in ('near_f32_max', 'subnormal_f32', 'dense_beside_far', 'overflow_f64', 'lattice'):
        x, y, z = ref.xyz(nc.cases()[case]['cols'])
        p = np.stack([x, y, z], 1)
        n = len(p)
        groups = []
        for _ in range(40):
            a, b = (rng.permutation(n)[:rng.integers(1, 9)] for _ in range(2))
            groups.append((a, b))
        queries = [('bound', [*p[a].min(0), *p[a].max(0), *p[b].min(0), *p[b].max(0)]) for a, b in groups]
        for (a, b), lb in zip(groups, nc.native(nc.cases()[case]['cols'], queries, tmp_path, True)):
            with np.errstate(all='ignore'):
                d = p[b][:, None, :] - p[a][None, :, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert not math.isnan(lb) and lb >= 0 and np.all(d2 >= lb), (case, lb, d2.min())


def test_expected_values_the_rules_name():
    """the restatement itself on the values the rules spell out"""
    two = [('x', np.array([0, 3], np.float32)), ('y', np.array([0, 4], np.float32)), ('z', np.zeros(2, np.float32))]
    assert list(ref.dist_k(two, 1)) == [5.0, 5.0]
    three = nc.table(np.tile([1.5, -2.0, 0.25], (3, 1)))
    d = ref.dist_k(three, 2)
    assert np.all(d == 0) and not np.any(np.signbit(d))
    assert np.all(ref.dist_k(three, 3) == INF)
    # a row that is not placed: the one quiet NaN; it is nobody's neighbour
    c = nc.cases()['few_placed']
    d1, d8 = nc.expected('few_placed')[1], nc.expected('few_placed')[8]
    assert ref.placed(c['cols']).sum() == 5
    assert np.all(d1.view(np.uint64)[5:] == ref.NAN_BITS) and np.all(np.isfinite(d1[:5])) and np.all(d8[:5] == INF)
    assert np.all(nc.expected('none_placed')[1].view(np.uint64) == ref.NAN_BITS)
    # more than k coincident rows: distance 0 for each of them, whatever k
    co = nc.expected('coincident_in_cloud')
    assert all((co[k] == 0).sum() in (40, 41) for k in nc.KS)
    # d2 beyond the float32 range, and beyond float64's
    assert np.all(np.isfinite(nc.expected('near_f32_max')[32])) and nc.expected('near_f32_max')[1].max() > 1e37
    ov = nc.expected('overflow_f64')
    assert (ov[1] == INF).sum() == 20 and (ov[32] == INF).sum() == 20 and not np.any(np.isnan(ov[32]))
    # the lattice: the nearest is at 1, the 7th of an inner point at sqrt(2)
    la = nc.expected('lattice')
    assert np.all(la[1] == 1.0) and la[7].min() == math.sqrt(2.0) and len(np.unique(la[32])) < 12
    # the verdicts: not placed goes, +Infinity goes unless t is +Infinity, no finite value keeps nothing
    assert len(ref.kept(d8, ref.SIGMA, 1.0)) == 0 and len(ref.kept(d8, ref.DISTANCE, 1e300)) == 0
    assert list(ref.kept(d8, ref.DISTANCE, INF)) == [0, 1, 2, 3, 4]
    assert math.isnan(ref.threshold(d8, ref.SIGMA, 0.0))
    m, s = ref.mean_std([1.0, 2.0, 3.0, 4.0, NAN, INF])
    assert (m, s) == (2.5, math.sqrt(1.25))


def test_scene_keeps_the_cluster():
    """the scene of the GPU test: k = 8, sigma = 1 keeps exactly the 4,000 cluster rows"""
    cols, cluster = nc.scene()
    d = ref.dist_k(cols, 8)
    assert np.array_equal(ref.kept(d, ref.SIGMA, 1.0), np.flatnonzero(cluster))


def test_make_actions_and_exports():
    a = sh.make_actions([{'kind': 'filterOutliers', 'sigma': 1.5}, {'kind': 'filterOutliers', 'k': 12, 'distance': 0.25},
                         {'kind': 'filterOutliers', 'k': 2.5, 'sigma': 1.0}, {'kind': 'filterNaN'}])
    assert [x.kind for x in a] == [sh.ACTION_FILTER_OUTLIERS] * 3 + [sh.ACTION_FILTER_NAN]
    assert (a[0].neighbors, a[0].outlier_mode, a[0].outlier_value) == (8, sh.OUTLIER_SIGMA, 1.5)
    assert (a[1].neighbors, a[1].outlier_mode, a[1].outlier_value) == (12, sh.OUTLIER_DISTANCE, 0.25)
    assert a[2].neighbors == 0  # no integer: a k the library refuses
    assert (sh.ACTION_FILTER_OUTLIERS, sh.OUTLIER_SIGMA, sh.OUTLIER_DISTANCE) == (10, 0, 1)
    for bad in ({'kind': 'filterOutliers'}, {'kind': 'filterOutliers', 'k': 8}, {'kind': 'filterOutliers', 'sigma': 1, 'distance': 1}):
        with pytest.raises(ValueError):
            sh.make_actions([bad])
    assert 'filterOutliers' in sh.FILTER_KINDS
    # a zero-filled action of an older kind is what it was: the new fields come last
    z = sh.make_actions([{'kind': 'decimate', 'count': 3}])[0]
    assert (z.neighbors, z.outlier_mode, z.outlier_value) == (0, 0, 0.0)
    assert sh.Action.neighbors.offset > sh.Action.amount_mode.offset
    for name in ('st_dev_neighbor_dist', 'st_ctx_last_neighbor_stats'):
        assert name in sh.EXPORTS and getattr(sh.lib(), name)
    for name in ('dev_neighbor_dist', 'neighbor_dist', 'last_neighbor_stats'):
        assert callable(getattr(sh.Context, name))
