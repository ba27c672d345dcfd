"""The rules of include/st_abi.h ("neighbour distances and outliers") restated in numpy, independent of
csrc/st_neighbors.h: a brute-force n x n d2 in float64 with the operations in the order the rules
write them (numpy rounds each elementwise operation once), the diagonal excluded, np.partition for
the k-th element; the threshold from math.fsum-based mean and ssd as the column-summary rules define
them.  Shared by tests/test_neighbors_cpu.py (the serial host form) and tests/test_neighbors_gpu.py."""
import math

import numpy as np

NAN_BITS = np.uint64(0x7ff8000000000000)  # dist_k of a row that is not placed
SIGMA, DISTANCE = 0, 1


def xyz(cols):
    """the first x, y, z of a dict or list of (name, array) of any of the eight types, as float64"""
    first = {}
    for k, a in (cols.items() if isinstance(cols, dict) else cols):
        first.setdefault(k, a)
    return tuple(np.asarray(first[k]).astype(np.float64) for k in 'xyz')


def placed(cols):
    x, y, z = xyz(cols)
    return np.isfinite(x) & np.isfinite(y) & np.isfinite(z)


def dist_ks(cols, ks, block=512):
    """{k: dist_k of every row as a float64 array (NaN rows carry NAN_BITS)} from one pass over the pairs"""
    x, y, z = xyz(cols)
    n = len(x)
    at = np.flatnonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    px, py, pz = x[at], y[at], z[at]
    p = len(at)
    res = {k: np.full(p, np.inf) for k in ks}  # fewer than k other placed rows: +Infinity
    with np.errstate(all='ignore'):
        for a in range(0, p, block):
            b = min(p, a + block)
            dx = px[a:b, None] - px[None, :]
            dy = py[a:b, None] - py[None, :]
            dz = pz[a:b, None] - pz[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
            # j = i is no member of the multiset.  Where at least k others are, the k-th smallest of
            # the row is theirs, an Infinity among them included
            d2[np.arange(b - a), np.arange(a, b)] = np.inf
            for k in ks:
                if p - 1 >= k:
                    res[k][a:b] = np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
    out = {}
    for k in ks:
        out[k] = np.empty(n, np.float64)
        out[k].view(np.uint64)[:] = NAN_BITS
        out[k][at] = res[k]
    return out


def dist_k(cols, k):
    return dist_ks(cols, [k])[k]


def mean_std(values):
    """the column summary's mean and std_dev over the finite values: exact sums rounded once (fsum),
    one division, d * d per element, sqrt(ssd / m); NaN, NaN without a finite value"""
    v = [float(t) for t in values if math.isfinite(t)]
    m = len(v)
    if m == 0:
        return math.nan, math.nan
    mean = math.fsum(v) / float(m)
    sq = [(t - mean) * (t - mean) for t in v]
    ssd = math.inf if any(math.isinf(t) for t in sq) else math.fsum(sq)
    return mean, math.sqrt(ssd / float(m))


def threshold(dist, mode, value):
    if mode == DISTANCE:
        return float(value)
    mean, std = mean_std(dist)
    w = float(value) * std
    return mean + w


def kept(dist, mode, value):
    """the rows filterOutliers keeps, ascending: uint32"""
    t = threshold(dist, mode, value)
    with np.errstate(all='ignore'):
        return np.flatnonzero(dist <= t).astype(np.uint32)


def apply(cols, action):
    """filterOutliers on a list of (name, array): the processed list"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    assert action['kind'] == 'filterOutliers'
    d = dist_k(items, action.get('k', 8))
    rows = kept(d, SIGMA, action['sigma']) if 'sigma' in action else kept(d, DISTANCE, action['distance'])
    return [(name, np.ascontiguousarray(a[rows])) for name, a in items]
