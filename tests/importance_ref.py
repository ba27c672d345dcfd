"""The rules of include/st_abi.h ("importance, decimation and crops") restated in numpy and plain
Python floats, independent of csrc/st_importance.h: the score with the oracle's V8 exp, the
importance order as a stable argsort, decimate's row count and selection, the box and the sphere.
Shared by tests/test_importance_cpu.py (the serial host form) and tests/test_importance_gpu.py."""
import math

import numpy as np

import oracle

NAN_BITS = np.uint64(0x7ff8000000000000)  # every NaN score is stored as this one (the rule's choice)
SCORE_COLS = ('scale_0', 'scale_1', 'scale_2', 'opacity')


def vexp(a):
    """oracle.exp over an array, evaluated once per distinct bit pattern"""
    a = np.ascontiguousarray(a, np.float64)
    u, inv = np.unique(a.view(np.uint64), return_inverse=True)
    vals = np.array([oracle.exp(float(x)) for x in u.view(np.float64)], np.float64)
    return vals[inv].reshape(a.shape)


def scores(cols):
    """exp((scale_0 + scale_1) + scale_2) * (1 / (1 + exp(-opacity))) per row; cols: dict or list of
    (name, array) of any of the eight types"""
    c = dict(cols)
    s0, s1, s2, o = (np.asarray(c[k]).astype(np.float64) for k in SCORE_COLS)
    with np.errstate(all='ignore'):
        s = (s0 + s1) + s2
        v = vexp(s) * (1.0 / (1.0 + vexp(-o)))
    out = v.copy()
    out.view(np.uint64)[np.isnan(v)] = NAN_BITS
    return out


def order(score):
    """descending score, NaN after every number, ties by ascending row: uint32 rows"""
    with np.errstate(all='ignore'):
        return np.argsort(-np.where(np.isnan(score), -1.0, score), kind='stable').astype(np.uint32)


def top(score, m):
    """the rows of rank < m, ascending"""
    return np.sort(order(score)[:m])


def decimate_rows(n, count=None, fraction=None):
    """decimate's m (the arguments are valid)"""
    if count is not None:
        return min(int(count), n)
    return min(n, int(math.floor(float(fraction) * float(n))))


def _column(c, k, n):
    return [float(v) for v in np.asarray(c[k]).astype(np.float64)] if k in c else [math.nan] * n


def box(cols, n, lo, hi):
    """rows inside the box, faces included, in plain Python floats; a missing column reads NaN"""
    c = dict(cols)
    xs, ys, zs = (_column(c, k, n) for k in 'xyz')
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    keep = [i for i in range(n)
            if xs[i] >= lo[0] and xs[i] <= hi[0] and ys[i] >= lo[1] and ys[i] <= hi[1] and zs[i] >= lo[2] and zs[i] <= hi[2]]
    return np.array(keep, np.uint32)


def sphere(cols, n, center, radius):
    c = dict(cols)
    xs, ys, zs = (_column(c, k, n) for k in 'xyz')
    cx, cy, cz = (float(v) for v in center)
    r = float(radius)
    keep = []
    for i in range(n):
        dx, dy, dz = xs[i] - cx, ys[i] - cy, zs[i] - cz
        if ((dx * dx + dy * dy) + dz * dz) < r * r:
            keep.append(i)
    return np.array(keep, np.uint32)


def apply(cols, action):
    """one of the four actions on a list of (name, array): the processed list"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    n = len(items[0][1]) if items else 0
    k = action['kind']
    if k == 'filterBox':
        rows = box(items, n, action['min'], action['max'])
    elif k == 'filterSphere':
        rows = sphere(items, n, action['center'], action['radius'])
    elif k == 'decimate':
        m = decimate_rows(n, action.get('count'), action.get('fraction'))
        rows = top(scores(items), m) if m < n else np.arange(n, dtype=np.uint32)
    elif k == 'orderByImportance':
        rows = order(scores(items)) if n > 1 else np.arange(n, dtype=np.uint32)
    else:
        raise ValueError(k)
    return [(name, np.ascontiguousarray(a[rows])) for name, a in items]
