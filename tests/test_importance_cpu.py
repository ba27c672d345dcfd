"""include/st_abi.h's "importance, decimation and crops" without a GPU: st_importance.h's serial host
form -- the score, key, predicate and row-count functions the kernels call, in a stand-alone program
(tests/native/importance_cpu_check.cpp, built plainly and with AddressSanitizer and
UndefinedBehaviorSanitizer, and run directly) -- against the restatement of tests/importance_ref.py
on every table of tests/importance_cases.py.  Scores are compared as uint64 bit patterns, rows
exactly.  The device must give the same (tests/test_importance_gpu.py)."""
import math

import numpy as np
import pytest

import importance_cases as ic
import importance_ref as ref
import splat_hip as sh

SCORE_CASES = sorted(ic.score_cases())
CROP_CASES = sorted(ic.crop_cases())


@pytest.mark.parametrize('case', SCORE_CASES)
def test_scores_order_and_top_equal_the_restatement(case, tmp_path):
    c, want = ic.score_cases()[case], ic.expected(case)
    ms = ic.rows_of(case)
    for sanitize in ((False,) if case == ic.BIG else (True, False)):  # two million rows: the optimised build only
        scores, order, tops = ic.native(c['cols'], [('top', m) for m in ms], tmp_path, sanitize)
        assert np.array_equal(scores.view(np.uint64), want['scores'].view(np.uint64))
        assert np.array_equal(order, want['order'])
        for m, rows in zip(ms, tops):
            assert np.array_equal(rows, want['top'][m]), (case, m)


@pytest.mark.parametrize('case', CROP_CASES)
def test_box_and_sphere_equal_the_restatement(case, tmp_path):
    c, want = ic.crop_cases()[case], ic.expected_crop(case)
    queries = [('box', lo, hi) for lo, hi in c['boxes']] + [('sphere', ce, r) for ce, r in c['spheres']]
    for sanitize in ((False,) if case == ic.BIG else (True, False)):
        _, _, got = ic.native(c['cols'], queries, tmp_path, sanitize)
        for q, rows, w in zip(queries, got, want['boxes'] + want['spheres']):
            assert np.array_equal(rows, w), (case, q)


def test_decimate_row_counts(tmp_path):
    """count: a finite non-negative integer below 2^53, cut to n; fraction: [0, 1], floor(f * n) in f64"""
    n = 70_001
    queries, want = [], []
    for count, m in [(0.0, 0), (1.0, 1), (70_001.0, n), (1e15, n), (2.0 ** 53 - 1, n), (-0.0, 0)]:
        queries.append(('rows', sh.DECIMATE_COUNT, count))
        want.append(m)
    for bad in (0.5, -1.0, math.nan, math.inf, 2.0 ** 53, 1e300):
        queries.append(('rows', sh.DECIMATE_COUNT, bad))
        want.append(ic.REFUSED)
    for f in ic.FRACTIONS + [0.5, 0.999999, 1e-300, -0.0]:
        queries.append(('rows', sh.DECIMATE_FRACTION, f))
        want.append(ref.decimate_rows(n, fraction=f))
    for bad in (-1e-300, math.nextafter(1.0, 2.0), math.nan, math.inf, -math.inf):
        queries.append(('rows', sh.DECIMATE_FRACTION, bad))
        want.append(ic.REFUSED)
    queries.append(('rows', 2, 0.5))  # no such mode
    want.append(ic.REFUSED)
    cols = [('x', np.zeros(n, np.float32))]
    for sanitize in (True, False):
        _, _, got = ic.native(cols, queries, tmp_path, sanitize)
        assert got == want
    # the tiny tables: floor(f * n)
    for n, ms in ((3, [0, 3, 0, 1]), (10, [0, 10, 2, 3])):
        _, _, got = ic.native([('x', np.zeros(n, np.float32))], [('rows', sh.DECIMATE_FRACTION, f) for f in ic.FRACTIONS],
                              tmp_path)
        assert got == ms


def test_expected_values_the_rules_name():
    """the restatement itself on the values the rules spell out"""
    c, e = dict(ic.score_cases()['specials_f32']['cols']), ic.expected('specials_f32')
    s = e['scores']
    nan_rows = np.isnan(c['opacity']) | np.isnan(c['scale_0']) | np.isinf(c['scale_1']) | \
        (np.isinf(c['scale_0']) & (c['opacity'] == -np.inf))
    assert nan_rows.sum() == 160 and np.array_equal(np.isnan(s), nan_rows)
    assert np.all(s.view(np.uint64)[nan_rows] == ref.NAN_BITS)
    assert (s == np.inf).sum() == 80 and ((s == 0) & ~np.signbit(s)).sum() == 120
    sub = (s > 0) & (s < np.finfo(np.float64).tiny)
    assert sub.sum() == 80
    assert not np.any(np.signbit(s[~nan_rows])) and np.all(s[~nan_rows] >= 0)
    o = e['order']
    assert np.all(s[o[:80]] == np.inf) and np.all(np.isnan(s[o[480:]])) and not np.any(np.isnan(s[o[:480]]))
    assert np.all(np.diff(o[480:].astype(np.int64)) > 0)  # NaN among NaN: by row
    assert np.all(s[o[1:480]] <= s[o[:479]])
    # more NaN rows than dropped rows: the kept NaN rows are the lowest-numbered ones
    h, eh = ic.score_cases()['nan_heavy'], ic.expected('nan_heavy')
    nn = h['nan_rows']
    assert nn > 150
    kept = eh['top'][250]
    nan_at = np.flatnonzero(np.isnan(eh['scores']))
    assert np.array_equal(np.intersect1d(kept, nan_at), nan_at[:250 - (300 - nn)])
    # the sphere: (3, 4, 0) is on radius 5, not inside; an f32 subtraction would keep float32(0.1)
    cr, ec = ic.crop_cases()['edges_float32'], ic.expected_crop('edges_float32')
    assert 2 not in ec['spheres'][0] and 3 not in ec['spheres'][0] and 0 in ec['spheres'][0]
    assert 2 in ec['spheres'][1]  # the next radius up takes it
    assert len(ec['spheres'][2]) == 0 and np.array_equal(ec['spheres'][3], ec['spheres'][0])
    assert len(ec['spheres'][5]) == 0 and len(ec['spheres'][6]) == 0
    assert cr['cols'][0][1][6] == np.float32(0.1) and len(ec['spheres'][8]) == 0
    assert list(ic.expected_crop('edges_float64')['spheres'][8]) == [6]
    # the box: faces kept, one step outside dropped, NaN bound and min > max keep nothing
    assert set(range(7, 19, 2)) <= set(ec['boxes'][0]) and not set(range(8, 19, 2)) & set(ec['boxes'][0])
    assert list(ec['boxes'][1]) == [0, 1] and list(ec['boxes'][2]) == [0, 1]
    assert len(ec['boxes'][6]) == 0 and len(ec['boxes'][7]) == 0 and len(ec['boxes'][8]) == 0
    assert list(ec['boxes'][9]) == [4]
    finite_or_inf = ~np.isnan(np.stack([a for _, a in cr['cols']])).any(0)
    assert np.array_equal(ec['boxes'][3], np.flatnonzero(finite_or_inf))
    assert len(ic.expected_crop('missing_z')['boxes'][3]) == 0
    # thousands of verdicts near the boundary, on both sides
    es = ic.expected_crop('on_sphere')['spheres'][0]
    assert 2000 < len(es) < 8000


def test_make_actions_carries_the_new_kinds():
    a = sh.make_actions([{'kind': 'filterBox', 'min': (1, 2, 3), 'max': (4, 5, 6)},
                         {'kind': 'filterSphere', 'center': (7, 8, 9), 'radius': 2.5},
                         {'kind': 'decimate', 'count': 12}, {'kind': 'decimate', 'fraction': 0.25},
                         {'kind': 'orderByImportance'}, {'kind': 'filterNaN'}])
    assert [x.kind for x in a] == [sh.ACTION_FILTER_BOX, sh.ACTION_FILTER_SPHERE, sh.ACTION_DECIMATE, sh.ACTION_DECIMATE,
                                   sh.ACTION_ORDER_IMPORTANCE, sh.ACTION_FILTER_NAN]
    assert list(a[0].box_min) == [1, 2, 3] and list(a[0].box_max) == [4, 5, 6]
    assert list(a[1].center) == [7, 8, 9] and a[1].radius == 2.5
    assert (a[2].amount_mode, a[2].amount) == (sh.DECIMATE_COUNT, 12.0)
    assert (a[3].amount_mode, a[3].amount) == (sh.DECIMATE_FRACTION, 0.25)
    with pytest.raises(ValueError):
        sh.make_actions([{'kind': 'decimate'}])
    with pytest.raises(ValueError):
        sh.make_actions([{'kind': 'decimate', 'count': 1, 'fraction': 0.5}])
    for k in ('filterBox', 'filterSphere', 'decimate', 'orderByImportance'):
        assert k in sh.FILTER_KINDS
    # the library exports the three calls (lib() resolves every name in EXPORTS)
    for name in ('st_dev_importance', 'st_dev_importance_order', 'st_dev_importance_top'):
        assert name in sh.EXPORTS and getattr(sh.lib(), name)
