"""The exact-tie cases of assign_tie_cases.py, checked without a GPU: each case's preconditions
(conditions on its inputs, computed in numpy), the oracle's labels being exact f64 argmins, and
the oracle's tie-break being the KdTree's (kd-tree.ts:39-68) rather than "lowest index" -- so a
device that took the smallest tied index would fail test_assign_ties_gpu.py on every case."""
import numpy as np
import pytest

import assign_tie_cases as tc
import oracle


def oracle_labels(case):
    if case.loop:
        rc, _, labels, _ = oracle.kmeans(case.cols, case.k, 1, case.draws)
    else:
        rc, labels = oracle.kmeans_assign(case.cols, case.cen)
    assert rc == 0
    return labels


@pytest.mark.parametrize('name', tc.NAMES)
def test_tie_case_preconditions_and_oracle_tie_break(name):
    case, st = tc.build(name), tc.stats(name)
    print(f"{name}: d={case.d} k={case.k} n={case.n} tied={st['ntied']} distinct tied rows={st['distinct_tied']} "
          f"listed for the walk={st['walk_tied']} (distinct rows {st['walk_distinct']}) "
          f"distinct rows={st['distinct_rows']} largest multiplicity={st['max_mult']} walk={tc.walk_branch(st)}")
    for a in case.cols + [case.cen]:
        assert a.dtype == np.float32 and np.isfinite(a).all()
    tc.check_preconditions(case, st)
    want = oracle_labels(case)
    assert tc.not_argmin(case, want, st) == 0
    untied = ~st['tied']
    assert np.array_equal(want[untied], st['lowest'][untied])
    higher = int((want[st['tied']] != st['lowest'][st['tied']]).sum())
    print(f'{name}: tied points the tree gives to a higher index than the lowest minimiser: {higher}')
    assert higher > 0


def test_loop_cases_draw_their_centroids_in_index_order():
    """the k-means-loop cases' init (k-means.ts:8-20) draws rows 0..k-1 in order, and those rows
    are the case's centroids: one iteration's labels are the assign against them"""
    for name in tc.NAMES:
        case = tc.build(name)
        if not case.loop:
            continue
        rows = np.floor(case.draws[:case.k] * case.n).astype(np.int64)
        assert np.array_equal(rows, np.arange(case.k))
        assert np.array_equal(np.stack([c[:case.k] for c in case.cols]), case.cen)
        _, want = oracle.kmeans_assign(case.cols, case.cen)
        assert np.array_equal(oracle_labels(case), want)


def _tree_labels(case, right_if=lambda dist: dist > 0, better=lambda d, best: d < best, stable=True,
                 node_first=False):
    """The device's build and walk (st_kdtree.hip: seg_split, k_kd_walk) restated in plain Python,
    with the choices a kernel could get subtly wrong as parameters: which side is near at
    equality, strict or non-strict improvement, the order among equal coordinates in the build,
    and whether a node is tried before or after its near subtree."""
    cen = case.cen.astype(np.float64)
    pts = np.stack(case.cols, axis=1).astype(np.float64)
    d = case.d

    def build(idx, depth):
        if not idx:
            return None
        # a stable sort of the order the level above left (-0.0 == 0.0: one value)
        idx = sorted(idx if stable else idx[::-1], key=lambda i: cen[depth % d, i])
        if len(idx) <= 2:
            return (idx[0], None, build(idx[1:], depth + 1))
        mid = len(idx) >> 1
        return (idx[mid], build(idx[:mid], depth + 1), build(idx[mid + 1:], depth + 1))

    root = build(list(range(case.k)), 0)
    out = np.empty(case.n, np.uint32)
    for p in range(case.n):
        best = [np.inf, -1]

        def visit(i):
            dist = 0.0
            for j in range(d):
                dist += (cen[j, i] - pts[p, j]) ** 2
            if better(dist, best[0]):
                best[:] = dist, i

        def walk(node, depth):
            if node is None:
                return
            i, left, right = node
            delta = pts[p, depth % d] - cen[depth % d, i]
            near, far = (right, left) if right_if(delta) else (left, right)
            if node_first:
                visit(i)
            walk(near, depth + 1)
            if not node_first:
                visit(i)
            if delta * delta < best[0]:
                walk(far, depth + 1)

        walk(root, 0)
        out[p] = best[1]
    return out


def test_cases_tell_a_subtly_wrong_walk_from_the_reference():
    """the restated walk gives the oracle's labels on a shallow case, and each single deviation --
    right at equality, non-strict improvement, another order among equal coordinates, the node
    before its near subtree -- gives other labels that are still exact argmins: the comparison
    of test_assign_ties_gpu.py would catch it"""
    case = tc.build('shallow-d2-k100')
    st = tc.stats(case.name)
    want = oracle_labels(case)
    assert np.array_equal(_tree_labels(case), want)
    for mutant in (dict(right_if=lambda dist: dist >= 0), dict(better=lambda d, best: d <= best),
                   dict(stable=False), dict(node_first=True)):
        got = _tree_labels(case, **mutant)
        assert tc.not_argmin(case, got, st) == 0
        assert (got != want).sum() > 0, sorted(mutant)


def test_exactness_of_the_tie_arithmetic():
    """every squared difference of a case fits f64's 53 bits with room for the sum: computing the
    distances with the dimensions reversed gives the same bits (the first 2,000 points)"""
    m = 2000
    for name in ('offset-1000', 'scaled-down', 'embedded-d45'):
        case = tc.build(name)
        st = tc.stats(name)
        rev = tc.tie_stats([c[:m] for c in case.cols[::-1]], np.ascontiguousarray(case.cen[::-1]))
        assert np.array_equal(st['dmin'][:m], rev['dmin']) and np.array_equal(st['mult'][:m], rev['mult'])
