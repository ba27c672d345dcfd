"""The rules of include/st_abi.h ("clusters") restated in numpy, independent of csrc/st_clusters.h: the
full n x n d2 in float64 with the operations in the order the rules write them (numpy rounds each
elementwise operation once), links by d2 <= radius * radius, the components by a breadth-first search
over the boolean matrix, min-index labels and sizes.  For n <= 4,096 (4,097 in one case).  Shared by
tests/test_clusters_cpu.py (the serial host form) and tests/test_clusters_gpu.py."""
import numpy as np

import neighbors_ref as nref

NONE = 0xFFFFFFFF  # label of a row that is not placed
MIN_SIZE, LARGEST = 0, 1


def link_matrix(cols, radius):
    """(the placed rows' indices, their boolean link matrix with a False diagonal)"""
    x, y, z = nref.xyz(cols)
    at = np.flatnonzero(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
    px, py, pz = x[at], y[at], z[at]
    with np.errstate(all='ignore'):
        r2 = np.float64(radius) * np.float64(radius)  # one multiplication; +Infinity when it overflows
    p = len(at)
    a = np.zeros((p, p), bool)
    with np.errstate(all='ignore'):
        for s in range(0, p, 512):  # the same matrix, 512 rows at a time
            e = min(p, s + 512)
            dx, dy, dz = px[s:e, None] - px[None, :], py[s:e, None] - py[None, :], pz[s:e, None] - pz[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
            a[s:e] = d2 <= r2
    np.fill_diagonal(a, False)
    return at, a


def clusters(cols, radius):
    """(label, size) of every row as uint32 arrays"""
    n = len(nref.xyz(cols)[0])
    at, a = link_matrix(cols, radius)
    p = len(at)
    comp = np.full(p, -1, np.int64)  # the component's first member, as an index into `at`
    for s in range(p):
        if comp[s] >= 0:
            continue
        comp[s] = s
        seen = np.zeros(p, bool)
        seen[s] = True
        front = seen.copy()
        while front.any():
            front = a[front].any(axis=0) & ~seen
            seen |= front
        comp[seen] = s  # at is ascending: s is the smallest row of the component
    label = np.full(n, NONE, np.uint32)
    size = np.zeros(n, np.uint32)
    if p:
        label[at] = at[comp].astype(np.uint32)
        size[at] = np.bincount(comp, minlength=p)[comp].astype(np.uint32)
    return label, size


def kept(size, mode, min_size=0):
    """the rows filterClusters keeps, ascending: uint32"""
    size = np.asarray(size)
    if mode == LARGEST:
        big = size.max() if len(size) else 0
        return np.flatnonzero((size > 0) & (size == big)).astype(np.uint32)
    return np.flatnonzero((size > 0) & (size.astype(np.float64) >= float(min_size))).astype(np.uint32)


def kept_for(size, action):
    return kept(size, LARGEST) if 'keep' in action else kept(size, MIN_SIZE, action['minSize'])


def apply(cols, action):
    """filterClusters on a list of (name, array): the processed list"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    assert action['kind'] == 'filterClusters'
    rows = kept_for(clusters(items, action['radius'])[1], action)
    return [(name, np.ascontiguousarray(a[rows])) for name, a in items]


def partition(label):
    """the components as a set of frozensets of row indices (the rows that are not placed left out)"""
    label = np.asarray(label)
    out = {}
    for i in np.flatnonzero(label != NONE):
        out.setdefault(int(label[i]), []).append(int(i))
    return {frozenset(v) for v in out.values()}
