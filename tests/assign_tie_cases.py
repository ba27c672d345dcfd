"""Exact-tie inputs for the N-D assign (a plain helper, imported by test_assign_ties_cpu.py and
test_assign_ties_gpu.py).

Every centroid coordinate is a small integer times a power of two (plus, in one case, the
integer 1,000) and every point coordinate a multiple of one half times the same power, all
f32: each difference, square and partial sum of calcDistance (kd-tree.ts:26-35) is then exact in
f64, so two centroids at the same distance from a point tie in the reference's arithmetic, in
numpy's and on the device alike, and the tie statistics computed here are exact.

build(name) -> Case (memoised; nothing in a Case is written after it is built).
stats(name) -> numpy-only facts about the case: per point the minimal distance, its multiplicity
               (how many centroids sit at it) and the lowest-index minimiser.
"""
import functools
import itertools
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Case:
    name: str
    cols: list              # d float32 arrays of n points
    cen: np.ndarray         # (d, k) float32
    env: dict = field(default_factory=dict)   # environment hooks set around the assign
    pre: dict = field(default_factory=dict)   # preconditions: see check_preconditions
    min_exact: int = 0      # k_exact launches the case must show (kn.exact: 2 = a list overflowed)
    loop: bool = False      # run through the one-device k-means loop (one iteration) instead
    draws: np.ndarray = None

    @property
    def d(self):
        return len(self.cols)

    @property
    def n(self):
        return len(self.cols[0])

    @property
    def k(self):
        return self.cen.shape[1]


# ---- exact distances in the reference's summation order -------------------------------
def _dist_block(pts, cen):
    """(rows of pts) x (columns of cen) squared distances: f64 differences of the f32 values,
    squares added in dimension order"""
    acc = np.zeros((pts.shape[0], cen.shape[1]), np.float64)
    for j in range(cen.shape[0]):
        v = pts[:, j].astype(np.float64)[:, None] - cen[j].astype(np.float64)[None, :]
        acc += v * v
    return acc


def dist_to(cols, cen, labels):
    """the distance of every point to the centroid its label names"""
    acc = np.zeros(len(labels), np.float64)
    lab = np.asarray(labels, np.int64)
    for j in range(len(cols)):
        v = cols[j].astype(np.float64) - cen[j].astype(np.float64)[lab]
        acc += v * v
    return acc


def tie_stats(cols, cen):
    pts = np.stack(cols, axis=1)
    n, k = pts.shape[0], cen.shape[1]
    dmin = np.empty(n, np.float64)
    mult = np.empty(n, np.int64)
    lowest = np.empty(n, np.int64)
    step = max(1, (1 << 23) // k)
    for lo in range(0, n, step):
        D = _dist_block(pts[lo:lo + step], cen)
        m = D.min(axis=1)
        eq = D == m[:, None]
        dmin[lo:lo + step] = m
        mult[lo:lo + step] = eq.sum(axis=1)
        lowest[lo:lo + step] = eq.argmax(axis=1)
    tied = mult >= 2
    bits = np.ascontiguousarray(pts).view(np.uint32)
    return dict(dmin=dmin, mult=mult, lowest=lowest, tied=tied, ntied=int(tied.sum()),
                distinct_tied=len(np.unique(bits[tied], axis=0)) if tied.any() else 0,
                distinct_rows=len(np.unique(bits, axis=0)), max_mult=int(mult.max()))


def not_argmin(case, labels, st=None):
    """how many labels are not even an exact f64 argmin (a sweep or fix-up error, as opposed to
    a tie-break error)"""
    st = st or stats(case.name)
    lab = np.asarray(labels, np.int64)
    ok = lab < case.k
    d = dist_to(case.cols, case.cen, np.where(ok, lab, 0))
    return int((~ok | (d != st['dmin'])).sum())


def check_preconditions(case, st):
    """the case's conditions on its inputs (computed in numpy from the case alone)"""
    p = case.pre
    tied, distinct = st['walk_tied'], st['walk_distinct']  # between distinct centroid rows
    assert tied >= p.get('tied', 1), (case.name, tied)
    if 'n_below' in p:
        assert case.n < p['n_below']
    if 'distinct_tied' in p:
        assert distinct >= p['distinct_tied'], (case.name, distinct)
    if 'repeats' in p:
        assert tied - distinct >= p['repeats'], (case.name, tied, distinct)
    if 'distinct_rows_max' in p:
        assert st['distinct_rows'] <= p['distinct_rows_max'], (case.name, st['distinct_rows'])
    if 'mult_above' in p:
        assert st['max_mult'] > p['mult_above'], (case.name, st['max_mult'])


def walk_branch(st):
    """which branch of the tie walk the case's tie list takes"""
    if st['walk_tied'] < 4096:
        return 'direct'
    return 'walkers, precomputed' if st['walk_distinct'] <= 64 else 'walkers'


# ---- building blocks ----------------------------------------------------------------
def _lattice(d, side):
    return np.array(list(itertools.product(range(side), repeat=d)), np.float32)  # (side^d, d)


def _palette(rng, d, side, k=None):
    rows = _lattice(d, side)
    rows = rows[rng.permutation(len(rows))]
    return np.ascontiguousarray(rows[:k].T)


def _half_points(rng, d, side, n):
    """random points of the half-integer grid over the lattice and half a step beyond it"""
    return (rng.integers(-1, 2 * side + 1, (n, d)) * 0.5).astype(np.float32)


def _cols(pts):
    return [np.ascontiguousarray(pts[:, j], np.float32) for j in range(pts.shape[1])]


def _sign_zeros(rng, a):
    a = a.copy()
    z = a == 0
    a[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return a


# ---- the cases ----------------------------------------------------------------------
def _shallow(d, k):
    rng = np.random.default_rng(1000 + 10 * k + d)
    side = 5
    while side ** d < k:
        side *= 2
    return Case(f'shallow-d{d}-k{k}', _cols(_half_points(rng, d, side, 3000)), _palette(rng, d, side, k),
                pre=dict(n_below=4096, tied=1))


def _deep(d, side, seed=0, n=20_000):
    rng = np.random.default_rng(2000 + 100 * d + side + seed)
    return Case(f'deep-d{d}-s{side}', _cols(_half_points(rng, d, side, n)), _palette(rng, d, side),
                pre=dict(tied=4096, distinct_tied=65, repeats=1000))


def _few(d, side):
    """the deep palette against at most 48 distinct rows, at least half of them tied, repeated
    to 12,000 points in shuffled order"""
    base = _deep(d, side)
    rng = np.random.default_rng(3000 + d)
    cand = np.unique(_half_points(rng, d, side, 4000), axis=0)
    cand = cand[rng.permutation(len(cand))]
    tied = tie_stats(_cols(cand), base.cen)['tied']
    rows = np.concatenate([cand[tied][:30], cand[~tied][:18]])
    pts = rows[rng.integers(0, len(rows), 12_000)]
    return Case(f'few-d{d}-s{side}', _cols(pts), base.cen, pre=dict(tied=4096, distinct_rows_max=64))


# tied centroids A..D around the point rows below: every listed point row is at one distance from
# at least two of them, on both sides of their coordinates (the walk meets them in either order)
_TIED_ROWS = np.array([(2, 0, 0), (3, 1, 0), (2, 1, 1), (3, 0, 1)], np.float32)


def _placed(k, idx, env=None, tag='', loop=False, d=3):
    """far filler centroids (40 + i, 40, 40) and len(idx) tied ones placed at the indices idx; the
    dimensions past the third hold zero in every row"""
    rng = np.random.default_rng(4000 + k + sum(idx))
    cen = np.zeros((d, k), np.float32)
    cen[0] = 40 + np.arange(k)
    cen[1:3] = 40
    t = _TIED_ROWS[:len(idx)]
    for i, row in zip(idx, t):
        cen[:3, i] = row
    # half-integer rows around the tied centroids, those with an exact tie among them kept, each
    # repeated; the tied centroids' own rows beside them (no tie)
    grid = np.array(list(itertools.product(np.arange(-2, 11) * 0.5, repeat=3)), np.float32)
    D = _dist_block(grid, np.ascontiguousarray(t.T))
    keep = grid[(D == D.min(axis=1)[:, None]).sum(axis=1) >= 2]
    keep = keep[rng.permutation(len(keep))][:40]
    rows = np.concatenate([keep, t])
    rows = np.concatenate([rows, np.zeros((len(rows), d - 3), np.float32)], axis=1)
    pts = rows[rng.integers(0, len(rows), 3000)]
    name = f'placed-k{k}-' + '_'.join(map(str, idx)) + tag
    case = Case(name, _cols(pts), cen, env=env or {}, pre=dict(tied=1))
    return _through_loop(case, name) if loop else case


def _through_loop(case, name):
    """the case through the k-means loop: the centroids become the first k rows of the point set,
    drawn in index order by the init (draw i falls into row i), and one iteration's labels are the
    assign against them"""
    pts = np.concatenate([case.cen.T, np.stack(case.cols, axis=1)])
    draws = np.concatenate([(np.arange(case.k) + 0.5) / len(pts), np.full(4 * case.k, 0.5)])
    return Case(name, _cols(pts), case.cen, env=case.env, pre=case.pre, min_exact=case.min_exact, loop=True,
                draws=draws)


def _wide(d):
    rng = np.random.default_rng(5000 + d)
    corners = np.array(list(itertools.product((0, 1), repeat=d)), np.float32)
    if d == 9:
        filler = np.full((512, d), 100, np.float32)
        filler[:, 0] += np.arange(512)
        rows, npts, ncentre, mult = np.concatenate([corners, filler]), 2000, 64, 64
    else:
        rows, npts, ncentre, mult = corners, 3000, 40, 2048
    rows = rows[rng.permutation(len(rows))]
    pts = rng.integers(0, 3, (npts, d)) * 0.5
    extra = [np.full((ncentre, d), 0.5)]
    if d == 12:  # rows with eleven halves: a 2,048-way tie, exactly the second list's size
        e = np.full((8, d), 0.5)
        e[np.arange(8), rng.integers(0, d, 8)] = rng.integers(0, 2, 8)
        extra.append(e)
    pts = np.concatenate([pts] + extra).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return Case(f'wide-d{d}', _cols(pts), np.ascontiguousarray(rows.T), pre=dict(tied=1, mult_above=mult),
                min_exact=2)


def _coinciding(env=None, tag=''):
    """the (3, 10) lattice with 24 rows absent and the others present one to three times: 2,048
    centroids"""
    rng = np.random.default_rng(6000)
    rows = _lattice(3, 10)
    rows = rows[rng.permutation(len(rows))]
    times = np.concatenate([np.zeros(24, int), np.full(104, 1), np.full(200, 3), np.full(672, 2)])
    rows = np.repeat(rows, times, axis=0)
    assert len(rows) == 2048
    rows = rows[rng.permutation(len(rows))]
    return Case('coinciding' + tag, _cols(_half_points(rng, 3, 10, 20_000)), np.ascontiguousarray(rows.T),
                env=env or {}, pre=dict(tied=4096))


def _signed(base, name):
    rng = np.random.default_rng(7000)
    return Case(name, [_sign_zeros(rng, c) for c in base.cols], _sign_zeros(rng, base.cen), env=base.env,
                pre=base.pre)


def _mapped(name, f):
    base = _deep(3, 10)
    return Case(name, [f(c).astype(np.float32) for c in base.cols], f(base.cen).astype(np.float32), pre=base.pre)


def _embedded(d):
    """the (2, 32) lattice in two of d dimensions; the others hold 3 in every centroid and 3.5 in
    every point (a quarter each in every distance: exact)"""
    base = _deep(2, 32, seed=d, n=8000)
    ax = (d // 3, d - 1)
    cen = np.full((d, base.k), 3, np.float32)
    cols = [np.full(base.n, 3.5, np.float32) for _ in range(d)]
    for a, j in zip(ax, range(2)):
        cen[a] = base.cen[j]
        cols[a] = base.cols[j]
    return Case(f'embedded-d{d}', cols, cen, pre=dict(tied=4096, distinct_tied=65))


SHALLOW = [(d, k) for d in (2, 3) for k in (2, 3, 5, 6, 7, 12, 100)]
DEEP = [(2, 32), (3, 10), (3, 16), (5, 4)]

_BUILDERS = {}
for _d, _k in SHALLOW:
    _BUILDERS[f'shallow-d{_d}-k{_k}'] = functools.partial(_shallow, _d, _k)
for _d, _s in DEEP:
    _BUILDERS[f'deep-d{_d}-s{_s}'] = functools.partial(_deep, _d, _s)
for _d, _s in ((3, 10), (5, 4)):
    _BUILDERS[f'few-d{_d}-s{_s}'] = functools.partial(_few, _d, _s)
for _idx in ((1, 2), (1, 2, 9), (1, 2, 9, 14), (1, 40), (5, 63), (1, 40, 5, 63)):
    _BUILDERS['placed-k64-' + '_'.join(map(str, _idx))] = functools.partial(_placed, 64, _idx)
_BUILDERS['placed-k2048-3_2044'] = functools.partial(_placed, 2048, (3, 2044))
_BUILDERS['placed-k2048-3_2044-serial'] = functools.partial(_placed, 2048, (3, 2044), {'ST_FIX_SERIAL': '1'},
                                                             '-serial')
# The direct entry point always runs the side fix-ups on the context's stream (join_ties' serial
# arm).  The one-device k-means loop puts them on the side stream at the palette row widths
# (join_ties' overlap arm) unless ST_FIX_SERIAL is set: the same shape in d = 9, through the loop
_BUILDERS['placed-k2048-1_2_9_2044-loop'] = functools.partial(_placed, 2048, (1, 2, 9, 2044), None, '-loop', True, 9)
_BUILDERS['placed-k2048-1_2_9_2044-loop-serial'] = functools.partial(_placed, 2048, (1, 2, 9, 2044),
                                                                      {'ST_FIX_SERIAL': '1'}, '-loop-serial', True, 9)
_BUILDERS['wide-d9'] = functools.partial(_wide, 9)
_BUILDERS['wide-d12'] = functools.partial(_wide, 12)
# the k-means loop publishes the assign's statistics: how many lists of 64 and of 2,048 overflowed
_BUILDERS['wide-d9-loop'] = lambda: _through_loop(_wide(9), 'wide-d9-loop')
_BUILDERS['wide-d12-loop'] = lambda: _through_loop(_wide(12), 'wide-d12-loop')
_BUILDERS['coinciding'] = _coinciding
_BUILDERS['coinciding-nogroups'] = functools.partial(_coinciding, {'ST_NO_CEN_GROUPS': '1'}, '-nogroups')
_BUILDERS['signed-deep-d3-s10'] = lambda: _signed(_deep(3, 10), 'signed-deep-d3-s10')
_BUILDERS['signed-coinciding'] = lambda: _signed(_coinciding(), 'signed-coinciding')
_BUILDERS['scaled-down'] = lambda: _mapped('scaled-down', lambda a: a * np.float32(2.0 ** -12))
_BUILDERS['scaled-up'] = lambda: _mapped('scaled-up', lambda a: a * np.float32(2.0 ** 10))
_BUILDERS['offset-1000'] = lambda: _mapped('offset-1000', lambda a: a + np.float32(1000))
for _d in (9, 24, 45, 16):
    _BUILDERS[f'embedded-d{_d}'] = functools.partial(_embedded, _d)

NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    for a in c.cols + [c.cen]:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def stats(name):
    c = build(name)
    st = tie_stats(c.cols, c.cen)
    # what the tie walk sees: with coinciding centroids grouped (nd_assign), a point whose minimisers
    # all share one row is settled by the group descent and only ties between distinct rows are listed
    rows = np.unique(c.cen.T + np.float32(0), axis=0)  # -0 + 0 = +0: rows as the distance sees them
    if len(rows) < c.k and 'ST_NO_CEN_GROUPS' not in c.env:
        w = tie_stats(c.cols, np.ascontiguousarray(rows.T))
        st.update(walk_tied=w['ntied'], walk_distinct=w['distinct_tied'], groups=True)
    else:
        st.update(walk_tied=st['ntied'], walk_distinct=st['distinct_tied'], groups=False)
    return st
