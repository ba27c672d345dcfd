"""The main sweep's top-3 update under each value of ST_SWEEP_UPDATE (always | lane | wave | both)
and under the default: every label is an exact f64 argmin, and the guarded forms classify the points
exactly as the unguarded one does.

The guarded forms skip the running top-3 update of a slot unless the slot's 16-row minimum is
below a per-lane threshold (k_sweep, st_kmeans_nd.hip).  A threshold that is too tight would drop
a tile from a lane's top-3: the point may still get the right label through the ambiguous path,
so the assign's counters (pairs, ambiguous, ties, overflow) are compared as well as the labels.

Cases, all through the one-device k-means loop (one iteration; its statistics are the assign's
counters).  The loop's point set is the palette's k rows followed by the case's n points, so the
sweep runs over n + k points (never a multiple of 32 here):
* a Gaussian palette sorted by distance to the points' mean, farthest first (for the n clustered
  points the tile minima fall along the sweep: the update fires at almost every tile) and nearest
  first (it fires in the first tiles only); D = 9 / 24 / 45 (one to three MFMAs per slot),
  K = 256 / 300 / 2,048 / 4,096 (one LDS stage, a padded last tile, several stages);
* the (3, 10) lattice palette of the exact-tie tests, zero-padded to D = 9 / 24 / 45: distinct
  centroids at one distance from a point, in different 32-row tiles, so the competing keys differ
  in their tile bits alone; with points whose best score |c|^2 - 2 p.c is negative, positive
  (near and at the origin, the origin's row absent from the palette), exactly zero (the origin's
  row present: the key of a zero minimum is a denormal) and far outside the palette.
"""
import functools

import numpy as np
import pytest

import assign_tie_cases as tc
import oracle
import splat_hip as sh

pytestmark = pytest.mark.gpu

FORMS = ('always', 'lane', 'wave', 'both', None)  # None: the variable unset (the library's default)
COUNTERS = ('assigns', 'points', 'pairs', 'ambiguous', 'overflow', 'walked_overflow', 'ties')

GAUSS = [(9, 256, 1000), (9, 300, 5003), (9, 2048, 5003), (9, 4096, 1000),
         (24, 256, 5003), (24, 300, 1000), (24, 2048, 1000), (24, 4096, 5003),
         (45, 256, 1000), (45, 300, 5003), (45, 2048, 5003), (45, 4096, 1000)]
TIES = ('neg', 'pos', 'near', 'zero', 'far')


@pytest.fixture(scope='module')
def ctx():
    import torch  # noqa: F401  (torch's HIP runtime first: see splat_hip.Context)
    c = sh.Context(0)
    yield c
    c.close()


# ---- the cases ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_case(d, k, n, order):
    rng = np.random.default_rng(9000 + 100 * d + k)  # one palette and point set for both orders
    pal = rng.normal(0, 1, (k, d)).astype(np.float32)
    mean = rng.normal(0, 0.5, d)
    # clustered far tighter than the gaps between the sorted palette rows' distances to the mean
    pts = (mean + rng.normal(0, 0.002, (n, d))).astype(np.float32)
    dist = ((pal.astype(np.float64) - pts.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1)
    idx = np.argsort(dist, kind='stable')
    if order == 'falling':
        idx = idx[::-1]
    name = f'gauss-d{d}-k{k}-n{n}-{order}'
    return _frozen(tc._through_loop(tc.Case(name, tc._cols(pts), np.ascontiguousarray(pal[idx].T)), name))


@functools.lru_cache(maxsize=None)
def tie_case(kind, d):
    rng = np.random.default_rng(9500 + d)  # one permutation of the lattice per d
    rows = tc._lattice(3, 10)
    rows = rows[rng.permutation(len(rows))]
    if kind in ('pos', 'near'):
        rows = rows[(rows != 0).any(axis=1)]  # without the origin's row: k = 999
    n = 3001
    if kind == 'neg':      # over the lattice: the nearest centroid is nearer than the origin
        pts = tc._half_points(rng, 3, 10, n)
    elif kind == 'far':    # up to four lattice widths out, still on half-integers: large negative scores
        pts = tc._half_points(rng, 3, 10, n) * np.float32(4) + np.float32(0.5)
    elif kind == 'near':   # 2^-6 of a coarse half-integer grid: every score a little under |c|^2 >= 1
        pts = (rng.integers(-1, 6, (n, 3)) * 0.5).astype(np.float32) * np.float32(2.0 ** -6)
    elif kind == 'pos':    # no positive coordinate, so score = |c|^2 + 2 |p.c| >= 1
        pts = (rng.integers(-2, 1, (n, 3)) * 0.5).astype(np.float32)
    else:                  # 'zero': coordinates 0 or 1/2: every c in {0, 1}^3 under p's halves scores 0
        pts = (rng.integers(0, 2, (n, 3)) * 0.5).astype(np.float32)
    pad = lambda a: np.concatenate([a, np.zeros((len(a), d - 3), np.float32)], axis=1)  # noqa: E731
    name = f'ties-{kind}-d{d}'
    return _frozen(tc._through_loop(tc.Case(name, tc._cols(pad(pts)), np.ascontiguousarray(pad(rows).T)), name))


def _frozen(case):
    for a in case.cols + [case.cen]:
        a.setflags(write=False)
    return case


# ---- the reference: exact f64 distances in the reference's summation order -----------------
_REF = {}


def reference(case):
    """per point: the minimal distance, how many centroids sit at it, the lowest and the highest
    of them, and the number of 32-row tiles whose minimum is below every earlier tile's (torch f64
    on the device, one dimension after another as kd-tree.ts:26-35 sums them); computed once per
    case and shared by the runs under every form"""
    if case.name in _REF:
        return _REF[case.name]
    import torch
    dev = torch.device('cuda', 0)
    P = torch.from_numpy(np.stack(case.cols, axis=1)).to(dev).double()
    C = torch.from_numpy(case.cen.copy()).to(dev).double()
    k, tiles = case.k, (case.k + 31) // 32
    ar = torch.arange(k, device=dev)
    out = [[] for _ in range(5)]
    for lo in range(0, case.n, 2048):
        acc = torch.zeros((min(2048, case.n - lo), k), dtype=torch.float64, device=dev)
        for j in range(case.d):
            v = C[j][None, :] - P[lo:lo + 2048, j, None]
            acc += v * v
        m = acc.min(dim=1).values
        eq = acc == m[:, None]
        tm = torch.nn.functional.pad(acc, (0, tiles * 32 - k), value=float('inf')).view(-1, tiles, 32).min(dim=2).values
        before = torch.cummin(tm, dim=1).values[:, :-1]
        res = (m, eq.sum(dim=1), torch.where(eq, ar, k).min(dim=1).values, torch.where(eq, ar, -1).max(dim=1).values,
               1 + (tm[:, 1:] < before).sum(dim=1))
        for o, r in zip(out, res):
            o.append(r.cpu().numpy())
    dmin, mult, lowest, highest, falls = (np.concatenate(o) for o in out)
    ref = dict(dmin=dmin, mult=mult, lowest=lowest, highest=highest, falls=falls, tied=mult >= 2, want=None)
    if ref['tied'].any():  # ties go by the KdTree rule: the CPU restatement's labels
        rc, _, want, _ = oracle.kmeans(case.cols, case.k, 1, case.draws)
        assert rc == 0
        ref['want'] = want
    _REF[case.name] = ref
    return ref


def run_forms(ctx, case, ref, monkeypatch):
    """one k-means iteration under each form; labels against the reference, then labels and
    counters of every form against the unguarded one"""
    # the loop's centroids are the case's: rows 0..k-1, drawn in index order
    assert np.array_equal(np.floor(case.draws[:case.k] * case.n).astype(np.int64), np.arange(case.k))
    assert np.array_equal(np.stack([c[:case.k] for c in case.cols]), case.cen)
    runs = {}
    for form in FORMS:
        if form is None:
            monkeypatch.delenv('ST_SWEEP_UPDATE', raising=False)
        else:
            monkeypatch.setenv('ST_SWEEP_UPDATE', form)
        _, got, _ = ctx.kmeans(case.cols, case.k, 1, case.draws)
        ks = ctx.kmeans_stats()
        print(f'{case.name} {form or "default"}: {ks}')
        got = np.asarray(got, np.uint32)
        assert (got < case.k).all(), (case.name, form)
        far = tc.dist_to(case.cols, case.cen, got) != ref['dmin']
        assert not far.any(), f'{case.name} {form}: {int(far.sum())} labels are not an exact f64 argmin'
        one = ~ref['tied']
        assert np.array_equal(got[one], ref['lowest'][one]), (case.name, form)
        if ref['want'] is not None:
            bad = got != ref['want']
            assert not bad.any(), f'{case.name} {form}: {int(bad.sum())} tied points are not labelled by the KdTree rule'
        runs[form] = (got, ks)
    base_labels, base_ks = runs['always']
    assert base_ks['assigns'] == 1 and base_ks['points'] == case.n
    for form in FORMS[1:]:
        got, ks = runs[form]
        assert np.array_equal(got, base_labels), (case.name, form)
        assert {c: ks[c] for c in COUNTERS} == {c: base_ks[c] for c in COUNTERS}, (case.name, form, ks, base_ks)
    return base_ks


@pytest.mark.parametrize('order', ('falling', 'rising'))
@pytest.mark.parametrize('d,k,n', GAUSS)
def test_sorted_palette(ctx, d, k, n, order, monkeypatch):
    case = gauss_case(d, k, n, order)
    ref = reference(case)
    # the case does what it is for: along the sweep the clustered points' tile minima keep falling
    # (the update fires at most tiles) or never fall again after the first tile
    falls, tiles = ref['falls'][case.k:], (k + 31) // 32
    print(f'{case.name}: tiles {tiles}, falling tile minima per clustered point: mean {falls.mean():.2f}')
    if order == 'falling':
        assert np.median(falls) >= 0.75 * tiles
    else:
        assert np.median(falls) == 1
    run_forms(ctx, case, ref, monkeypatch)


@pytest.mark.parametrize('d', (9, 24, 45))
@pytest.mark.parametrize('kind', TIES)
def test_equal_minima_in_different_tiles(ctx, kind, d, monkeypatch):
    case = tie_case(kind, d)
    ref = reference(case)
    pts = slice(case.k, None)  # the points behind the palette's own rows
    tied = ref['tied'][pts]
    apart = tied & (ref['lowest'][pts] // 32 != ref['highest'][pts] // 32)
    # the best score's sign, exactly: score = dist - |p|^2 (every term a small dyadic number)
    pn = sum(c[pts].astype(np.float64) ** 2 for c in case.cols)
    score = ref['dmin'][pts] - pn
    print(f'{case.name}: k {case.k}, tied {int(tied.sum())}, minimisers in different tiles {int(apart.sum())}, '
          f'best score < 0: {int((score < 0).sum())}, == 0: {int((score == 0).sum())}, > 0: {int((score > 0).sum())}')
    assert apart.sum() >= 200
    if kind in ('neg', 'far'):
        assert (score[apart] < 0).sum() >= 200
    elif kind == 'zero':
        assert (score == 0).all()
    else:
        assert (score > 0).all()
    ks = run_forms(ctx, case, ref, monkeypatch)
    assert ks['ties'] > 0
