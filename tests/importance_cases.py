"""Tables shared by tests/test_importance_cpu.py and tests/test_importance_gpu.py: the smallest inputs
at which each piece of include/st_abi.h's "importance, decimation and crops" can go wrong, their
expected results by tests/importance_ref.py (computed once per process), and the stand-alone program
of st_importance.h's serial host form (tests/native/importance_cpu_check.cpp).

score_cases(): {case: {'cols': [(name, array)], 'counts': [m, ...], 'fractions': [f, ...]}}
crop_cases():  {case: {'cols': [(name, array)], 'n': rows, 'boxes': [(min, max)], 'spheres': [(centre, radius)]}}"""
import atexit
import math
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import importance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'tests', 'native', 'importance_cpu_check.cpp')
DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]
PLY_CODE = {np.dtype(d): i + 1 for i, d in enumerate(DTYPES)}
LENGTHS = [0, 1, 255, 256, 257, 4097]
FRACTIONS = [0.0, 1.0, 0.25, 1.0 / 3.0]
BIG = 'bench_2100001'
INF, NAN = math.inf, math.nan


def bench_like(rng, n):
    """bench.py's synthetic distributions: opacity ~N(0, 2^2), scale ~U(-7, -2), float32"""
    return [('scale_0', (rng.random(n) * 5 - 7).astype(np.float32)),
            ('scale_1', (rng.random(n) * 5 - 7).astype(np.float32)),
            ('scale_2', (rng.random(n) * 5 - 7).astype(np.float32)),
            ('opacity', (rng.normal(0, 2, n)).astype(np.float32))]


def table(s0, s1, s2, o):
    return [('scale_0', s0), ('scale_1', s1), ('scale_2', s2), ('opacity', o)]


def around(n, *more):
    return sorted({m for m in (0, 1, n // 4, n // 2, n - 1, n, n + 1, *more) if m >= 0})


def score_cases():
    if _SCORE:
        return _SCORE
    rng = np.random.default_rng(31)
    t = {}
    # heads and tails of the vector loads, block edges
    for n in LENGTHS:
        t[f'len_{n}'] = dict(cols=bench_like(rng, n), counts=around(n))
    # every score equal: the selection is the tie rule alone
    one = np.full(1000, -2.5, np.float32)
    t['all_equal'] = dict(cols=table(one, one, one, np.full(1000, 0.75, np.float32)),
                          counts=[0, 1, 255, 256, 257, 999, 1000, 1001])
    # five distinct scores laid cyclically over 4,097 rows: in descending order the groups end at ranks
    # 820, 1639, 2459, 3278, 4097; counts on a group's first member, inside it and on its last
    lev = np.array([-3, -1, -4, -2, -5], np.float32)[np.arange(4097) % 5]
    z = np.zeros(4097, np.float32)
    t['ties_5'] = dict(cols=table(lev, z, z, np.ones(4097, np.float32)),
                       counts=[1, 400, 820, 821, 1200, 1639, 1640, 2459, 2460, 3000, 3278, 3279, 4096])
    # scores 1 + k 2^-52 (exp of a tiny x is 1 + x, sigmoid(40) is 1): the keys differ in their lowest
    # nine bits only, so the last select rounds decide
    k = rng.permutation(301).astype(np.float64)
    z = np.zeros(301)
    t['low_digit'] = dict(cols=table(k * 2.0 ** -52, z, z, np.full(301, 40.0)), counts=[1, 44, 45, 150, 256, 300])
    # scores 16 binades apart: every key has a top digit of its own, the first round decides.  (Keys
    # that differ in nothing else cannot be made: a score's mantissa comes out of exp)
    j = rng.permutation(np.arange(-30, 31)).astype(np.float64)
    z = np.zeros(61)
    t['top_digit'] = dict(cols=table(j * (16 * math.log(2.0)), z, z, np.full(61, 40.0)), counts=[1, 2, 30, 60])
    # the special values, 40 rows of each kind among ordinary rows, shuffled
    kinds = [(0.0, 0.0, 0.0, NAN),        # NaN opacity
             (NAN, 0.0, 0.0, 1.0),        # NaN scale
             (INF, 0.0, 0.0, -INF),       # Infinity * 0: NaN
             (INF, -INF, 0.0, 0.0),       # Infinity - Infinity in the sum: NaN
             (300.0, 300.0, 200.0, 0.0),  # exp overflows: +Infinity
             (INF, 0.0, 0.0, 2.0),        # +Infinity
             (0.0, 0.0, 0.0, -INF),       # sigmoid 0: +0
             (-300.0, -300.0, -200.0, 3.0),  # exp underflows: +0
             (-250.0, -250.0, -240.0, 0.0),  # subnormal
             (-250.0, -250.0, -244.0, -1.0),  # subnormal
             (-1.0, -2.0, -3.0, 800.0),   # sigmoid exactly 1
             (-1.0, -2.0, -3.0, -800.0)]  # exp(800) overflows inside sigmoid: 1 / Infinity = +0
    rows = np.array([kd for kd in kinds for _ in range(40)], np.float64)
    ordinary = np.stack([a.astype(np.float64) for _, a in bench_like(rng, 160)], 1)
    rows = rng.permutation(np.concatenate([rows, ordinary]))
    cols32 = table(*(rows[:, c].astype(np.float32) for c in range(4)))
    n = len(rows)
    t['specials_f32'] = dict(cols=cols32, counts=[1, 79, 80, 81, 100, 200, 300, 400, 479, 480, 481, 600, n - 1])
    t['specials_f64'] = dict(cols=table(*(rows[:, c].copy() for c in range(4))), counts=[80, 81, 333, n - 1])
    # more NaN rows than dropped rows: NaN rows are kept, the lowest indices among them
    c = bench_like(rng, 300)
    c[3][1][rng.permutation(300)[:120]] = NAN
    c[1][1][rng.permutation(300)[:120]] = NAN
    nn = int(np.isnan(c[3][1]).sum() + (np.isnan(c[1][1]) & ~np.isnan(c[3][1])).sum())
    t['nan_heavy'] = dict(cols=c, counts=[300 - nn - 1, 300 - nn, 300 - nn + 1, 250, 299], nan_rows=nn)
    # fractions of tiny tables (floor(f * n): 0.25 of 3 is 0, a third of 3 is 1, a third of 10 is 3)
    for n in (3, 10):
        t[f'fraction_{n}'] = dict(cols=bench_like(rng, n), counts=[], fractions=FRACTIONS)
    # integer columns
    t['integers'] = dict(cols=table(rng.integers(0, 4, 777).astype(np.uint16), rng.integers(0, 4, 777).astype(np.uint16),
                                    rng.integers(0, 4, 777).astype(np.uint16), rng.integers(-6, 7, 777).astype(np.int8)),
                         counts=[1, 100, 388, 776])
    t['mixed_types'] = dict(cols=table((rng.random(515) * 5 - 7).astype(np.float64), rng.integers(-3, 2, 515).astype(np.int32),
                                       (rng.random(515) * 5 - 7).astype(np.float32), rng.integers(-300, 300, 515).astype(np.int16)),
                            counts=[1, 128, 514])
    # bench.py's table at 70,001 rows, and 2,100,001 rows drawn from its rows (more than the 8192 x 256
    # threads of a capped grid: the stride loops take a second trip)
    base = bench_like(rng, 70_001)
    t['bench_70001'] = dict(cols=base, counts=[1, 17_500, 35_000, 70_000], fractions=FRACTIONS)
    pick = rng.integers(0, 70_001, 2_100_001)
    t[BIG] = dict(cols=[(k, a[pick]) for k, a in base], counts=[525_000, 2_100_000])
    for v in t.values():
        v.setdefault('fractions', [])
    _SCORE.update(t)
    return _SCORE


def crop_cases():
    if _CROP:
        return _CROP
    rng = np.random.default_rng(32)
    t = {}
    lo, hi = (-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)
    boxes = [(lo, hi),
             ((-0.0, -0.0, -0.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)),
             ((-INF, -INF, -INF), (INF, INF, INF)), ((INF, -INF, -INF), (INF, INF, INF)),
             ((-INF, -2.0, -INF), (1.0, INF, INF)),
             ((NAN, -2.0, -3.0), hi), (lo, (1.0, 2.0, NAN)),
             ((1.0, -2.0, -3.0), (-1.0, 2.0, 3.0)), ((1.0, 2.0, 3.0), (1.0, 2.0, 3.0))]
    spheres = [((0.0, 0.0, 0.0), 5.0), ((0.0, 0.0, 0.0), math.nextafter(5.0, INF)), ((0.0, 0.0, 0.0), 0.0),
               ((0.0, 0.0, 0.0), -5.0), ((0.0, 0.0, 0.0), -6.0), ((0.0, 0.0, 0.0), NAN), ((NAN, 0.0, 0.0), 5.0),
               ((0.0, 0.0, 0.0), INF), ((0.1, 0.0, 0.0), 1e-9), ((1.0, 2.0, 3.0), 1e-300)]
    for dt in (np.float32, np.float64):
        up = lambda v, d=dt: float(np.nextafter(d(v), d(INF)))
        dn = lambda v, d=dt: float(np.nextafter(d(v), d(-INF)))
        pts = [(0, 0, 0), (-0.0, -0.0, -0.0), (3, 4, 0), (0, 3, 4), (1, 2, 3), (-1, -2, -3), (0.1, 0, 0)]
        for a in range(3):  # on each face, and one step outside it
            for bound, step in ((lo[a], dn), (hi[a], up)):
                p = [0.5, 0.5, 0.5]
                p[a] = bound
                pts.append(tuple(p))
                p[a] = step(bound)
                pts.append(tuple(p))
        pts += [(NAN, 0, 0), (0, NAN, 0), (0, 0, NAN), (INF, 0, 0), (0, -INF, 0), (INF, INF, INF), (-INF, -INF, -INF)]
        pts += [tuple(v) for v in rng.normal(0, 2, (230, 3))]
        a = np.array(pts, np.float64).astype(dt)
        t[f'edges_{np.dtype(dt).name}'] = dict(cols=[('x', a[:, 0].copy()), ('y', a[:, 1].copy()), ('z', a[:, 2].copy())],
                                               boxes=boxes, spheres=spheres)
    e = t['edges_float32']['cols']
    t['missing_z'] = dict(cols=e[:2], boxes=boxes[:4], spheres=spheres[:2])
    t['missing_all'] = dict(cols=[('w', e[0][1])], boxes=boxes[:1], spheres=spheres[:1])
    for n in LENGTHS:
        a = rng.normal(0, 1.5, (n, 3)).astype(np.float32)
        t[f'len_{n}'] = dict(cols=[('x', a[:, 0].copy()), ('y', a[:, 1].copy()), ('z', a[:, 2].copy())],
                             boxes=boxes[:1], spheres=[((0.25, 0.0, -0.5), 2.0)])
    t['mixed_types'] = dict(cols=[('x', rng.integers(-4, 5, 515).astype(np.int16)), ('y', rng.normal(0, 2, 515)),
                                  ('z', rng.normal(0, 2, 515).astype(np.float32)), ('x', np.zeros(515, np.float32))],
                            boxes=boxes[:1], spheres=[((0.0, 0.0, 0.0), 3.0)])
    # 10,000 float32 points rounded from a sphere of the given radius: thousands of verdicts within a
    # few ulps of the boundary
    centre, radius = (0.5, -1.25, 2.0), 1.7
    d = rng.normal(0, 1, (10_000, 3))
    d /= np.sqrt((d * d).sum(1))[:, None]
    p = (np.array(centre) + radius * d).astype(np.float32)
    t['on_sphere'] = dict(cols=[('x', p[:, 0].copy()), ('y', p[:, 1].copy()), ('z', p[:, 2].copy())],
                          boxes=[((0.5, -1.25, 2.0), (INF, INF, INF))], spheres=[(centre, radius), (centre, float(np.float32(radius)))])
    # the stride loops' second trip
    a = rng.normal(0, 1.5, (2_100_001, 3)).astype(np.float32)
    t[BIG] = dict(cols=[('x', a[:, 0].copy()), ('y', a[:, 1].copy()), ('z', a[:, 2].copy())], big=True,
                  boxes=[((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))], spheres=[((0.0, 0.0, 0.0), 1.5)])
    for v in t.values():
        v['n'] = len(v['cols'][0][1])
    _CROP.update(t)
    return _CROP


_SCORE, _CROP, _EXPECTED, _EXPECTED_CROP = {}, {}, {}, {}


def rows_of(case):
    """every decimate row count the case asks for: its counts and its fractions' m, cut to n"""
    c = score_cases()[case]
    n = len(c['cols'][0][1])
    return sorted({min(m, n) for m in c['counts']} | {ref.decimate_rows(n, fraction=f) for f in c['fractions']})


def expected(case):
    """{'scores', 'order', 'top': {m: rows}} of a score case, computed once per process"""
    if case not in _EXPECTED:
        c = score_cases()[case]
        s = ref.scores(c['cols'])
        o = ref.order(s)
        _EXPECTED[case] = dict(scores=s, order=o, top={m: np.sort(o[:m]) for m in rows_of(case)})
    return _EXPECTED[case]


def _box_big(cols, lo, hi):
    x, y, z = (a.astype(np.float64) for _, a in cols)
    return np.flatnonzero((x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])).astype(np.uint32)


def _sphere_big(cols, c, r):
    x, y, z = (a.astype(np.float64) for _, a in cols)
    dx, dy, dz = x - c[0], y - c[1], z - c[2]
    return np.flatnonzero(((dx * dx + dy * dy) + dz * dz) < r * r).astype(np.uint32)


def expected_crop(case):
    """{'boxes': [rows], 'spheres': [rows]} of a crop case.  The two-million-row case uses the same
    expressions over float64 arrays (numpy rounds each operation once, as Python floats do)"""
    if case not in _EXPECTED_CROP:
        c = crop_cases()[case]
        if c.get('big'):
            e = dict(boxes=[_box_big(c['cols'], lo, hi) for lo, hi in c['boxes']],
                     spheres=[_sphere_big(c['cols'], ce, r) for ce, r in c['spheres']])
        else:
            first = {}
            for k, a in c['cols']:  # a duplicate name: the first column of that name counts
                first.setdefault(k, a)
            e = dict(boxes=[ref.box(first, c['n'], lo, hi) for lo, hi in c['boxes']],
                     spheres=[ref.sphere(first, c['n'], ce, r) for ce, r in c['spheres']])
        _EXPECTED_CROP[case] = e
    return _EXPECTED_CROP[case]


# ---- the stand-alone program -----------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_importance_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'importance_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=off', *flags, '-o', exe,
                               SOURCE])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


NAMES = ('scale_0', 'scale_1', 'scale_2', 'opacity', 'x', 'y', 'z')
REFUSED = 2 ** 64 - 1


def native(cols, queries, tmp_path, sanitize=False):
    """the program on [(name, array)] (the first column of a name counts) and queries -- ('top', m),
    ('box', min, max), ('sphere', centre, radius), ('rows', mode, amount) -> (scores or None, order or
    None, [rows per query, or the count for 'rows'])"""
    first = {}
    for k, a in cols:
        first.setdefault(k, np.ascontiguousarray(a))
    n = len(cols[0][1]) if cols else 0
    src, out = tmp_path / 'in.bin', tmp_path / 'out.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<Q', n))
        for k in NAMES:
            if k in first:
                f.write(struct.pack('<i', PLY_CODE[first[k].dtype]) + first[k].tobytes())
            else:
                f.write(struct.pack('<i', 0))
        f.write(struct.pack('<I', len(queries)))
        for q in queries:
            if q[0] == 'top':
                f.write(struct.pack('<iQ', 1, q[1]))
            elif q[0] == 'box':
                f.write(struct.pack('<i6d', 2, *q[1], *q[2]))
            elif q[0] == 'sphere':
                f.write(struct.pack('<i4d', 3, *q[1], q[2]))
            else:
                f.write(struct.pack('<iid', 4, q[1], q[2]))
    r = subprocess.run([harness(sanitize), str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    raw = out.read_bytes()
    at = 0
    scores = order = None
    if all(k in first for k in NAMES[:4]):
        scores = np.frombuffer(raw, np.float64, n, 0)
        order = np.frombuffer(raw, np.uint32, n, 8 * n)
        at = 12 * n
    res = []
    for q in queries:
        count = struct.unpack_from('<Q', raw, at)[0]
        at += 8
        if q[0] == 'rows':
            res.append(count)
            continue
        res.append(np.frombuffer(raw, np.uint32, count, at))
        at += 4 * count
    assert at == len(raw)
    return scores, order, res
