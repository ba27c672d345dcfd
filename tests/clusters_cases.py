"""Tables shared by tests/test_clusters_cpu.py and tests/test_clusters_gpu.py: the smallest inputs at which
each piece of include/st_abi.h's "clusters" can go wrong, their expected labels and sizes by
tests/clusters_ref.py (computed once per process), and the stand-alone program of st_clusters.h's
serial host form (tests/native/clusters_cpu_check.cpp).

cases(): {case: {'cols': [(name, array)], 'radii': [radius, ...], 'n': rows}}.  The expectation of the
20,000-row cases (BIG) comes from the native program, which the other cases cross-check against numpy.

The line cases: 20,000 rows at spacing exactly `radius` (0.25, every coordinate exact), shuffled, are one
component through every leaf.  A gap of nextafter(radius, inf) in float64 cannot lie on one straight
line of exact coordinates (20,000 spacings and a 2^-54 need 67 bits), so the two-component case comes
twice: `line_gap` is the same straight line in float64 columns with one gap of float32's
nextafter(0.25, inf) = 0.25 + 2^-25, and `line_gap_bent` has the gap of float64's nextafter(0.25, inf)
exactly, between the end of the line at the origin and a second half that goes on along y from
(-gap, 0, 0), all other spacings exactly 0.25."""
import atexit
import math
import os
import pathlib
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import clusters_ref as ref
import neighbors_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'tests', 'native', 'clusters_cpu_check.cpp')
PLY_CODE = nc.PLY_CODE
INF, NAN = math.inf, math.nan
REFUSED = 2 ** 64 - 1
LENGTHS = [0, 1, 2, 63, 64, 65, 257, 513, 4097]  # the edges of a 64-row leaf, one to three levels above it
BIG = ('line', 'line_gap', 'line_gap_bent')
LINE_RADIUS = 0.25
SCENE_RADIUS = 0.3

table = nc.table


def scatter_nonfinite(a, rng):
    """NaN, +Infinity and -Infinity, each in one coordinate of about n / 24 rows of their own"""
    n = len(a)
    if n < 8:
        return a
    rows = rng.permutation(n)[:3 * max(1, n // 24)].reshape(3, -1)
    for v, r in zip((NAN, INF, -INF), rows):
        a[r, rng.integers(0, 3, len(r))] = v
    return a


def cases():
    if _CASES:
        return _CASES
    rng = np.random.default_rng(83)
    t = {}
    for n in LENGTHS:
        mid = 1.4 * max(n, 1) ** (-1 / 3)  # about the nearest-neighbour distance at the centre of N(0, 1)
        t[f'len_{n}'] = dict(cols=table(scatter_nonfinite(rng.normal(0, 1, (n, 3)), rng)), radii=[mid, 2 * mid, 0.0, INF])
    # 257 placed rows: 65 four-row leaves, four box levels (len_257's rows without a position leave three)
    t['len_257_all_placed'] = dict(cols=table(rng.normal(0, 1, (257, 3))), radii=[0.22, 0.44])
    t['len_1_not_placed'] = dict(cols=table([[0.5, NAN, 1.0]]), radii=[1.0, INF])
    t['len_2_one_placed'] = dict(cols=table([[INF, 0.0, 1.0], [0.5, 0.25, 1.0]]), radii=[1.0, INF])
    t['len_2_linked'] = dict(cols=table([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]]), radii=[5.0, math.nextafter(5.0, 0), 0.0])
    t['none_placed'] = dict(cols=table(np.full((70, 3), NAN)), radii=[1.0, 0.0, INF])
    # exact ties: a 6 x 6 x 6 integer lattice scaled by 2^-3, shuffled.  At radius = the spacing the axis
    # neighbours sit at exactly d2 == r2 and link into one component; one ulp less and every row is alone
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing='ij'), -1).reshape(-1, 3)
    g = scatter_nonfinite(rng.permutation(g) * 0.125, rng)
    t['lattice'] = dict(cols=table(g), radii=[0.125, math.nextafter(0.125, 0), 0.125 * math.sqrt(2.0)])
    # radius 0: coincident groups of 1, 2, 64, 65 and 200 rows (they cross leaf boundaries: equal keys
    # are neighbours in sorted order) inside a cloud
    pts = rng.normal(0, 1, (5, 3))
    co = np.concatenate([np.tile(p, (m, 1)) for p, m in zip(pts, (1, 2, 64, 65, 200))] + [rng.normal(0, 1, (100, 3))])
    t['coincident_groups'] = dict(cols=table(rng.permutation(co)), radii=[0.0, 1e-30])
    # d2 overflows to +Infinity between the far rows: nothing links them at a finite radius; at
    # radius = inf every placed row is in the one component
    far = rng.normal(0, 1, (120, 3))
    far[rng.permutation(120)[:20]] *= 1e200
    far[:6] = [[1e200, 0, 0], [-1e200, 0, 0], [1e200, 0, 0], [0, 1e200, -1e200], [NAN, 0, 0], [1e200, 1e200, 1e200]]
    t['overflow_f64'] = dict(cols=table(rng.permutation(far), np.float64), radii=[1.0, 1e150, 1.7e308, INF])
    # other column types: float64 twins, and int16 / float64 / uint8 / float32 among columns the search
    # does not read (a second x: the first one counts)
    t['len_513_f64twin'] = dict(cols=[(k, a.astype(np.float64)) for k, a in t['len_513']['cols']],
                                radii=t['len_513']['radii'], twin='len_513')
    t['mixed_types'] = dict(cols=[('w', rng.normal(0, 1, 515).astype(np.float32)),
                                  ('x', rng.integers(-300, 300, 515).astype(np.int16)),
                                  ('y', rng.normal(0, 100, 515).astype(np.float32)),
                                  ('z', rng.integers(0, 256, 515).astype(np.uint8)), ('x', np.zeros(515, np.float32))],
                            radii=[20.0, 45.0, 0.0])
    t['mixed_types_f64'] = dict(cols=[('x', rng.integers(-300, 300, 515).astype(np.int32)), ('y', rng.normal(0, 100, 515)),
                                      ('z', rng.integers(0, 60000, 515).astype(np.uint16))], radii=[60.0, 3000.0])
    # the deep-tree cases of the union-find
    m = 20_000
    line = np.zeros((m, 3))
    line[:, 0] = np.arange(m) * LINE_RADIUS
    perm = rng.permutation(m)
    t['line'] = dict(cols=table(line[perm]), radii=[LINE_RADIUS])
    gap32 = float(np.nextafter(np.float32(LINE_RADIUS), np.float32(INF)))
    cut = line.copy()
    cut[m // 2:, 0] += gap32 - LINE_RADIUS  # 2^-25: exact in float64 at these magnitudes
    t['line_gap'] = dict(cols=table(cut[perm], np.float64), radii=[LINE_RADIUS])
    bent = np.zeros((m, 3))
    bent[:m // 2, 0] = np.arange(m // 2) * LINE_RADIUS
    bent[m // 2:, 0] = -math.nextafter(LINE_RADIUS, INF)
    bent[m // 2:, 1] = np.arange(m - m // 2) * LINE_RADIUS
    t['line_gap_bent'] = dict(cols=table(bent[perm], np.float64), radii=[LINE_RADIUS])
    for v in t.values():
        v['n'] = len(v['cols'][0][1])
    _CASES.update(t)
    return _CASES


_CASES, _EXPECTED = {}, {}


def expected(case):
    """{radius: (label, size) as uint32 arrays} of a case, computed once per process and read-only"""
    if case not in _EXPECTED:
        c = cases()[case]
        if case in BIG:
            d = tempfile.mkdtemp(prefix='st_clusters_big_')
            try:
                got = native(c['cols'], [('clusters', r) for r in c['radii']], pathlib.Path(d))
            finally:
                shutil.rmtree(d, ignore_errors=True)
        else:
            got = [ref.clusters(c['cols'], r) for r in c['radii']]
        for label, size in got:
            label.flags.writeable = False
            size.flags.writeable = False
        _EXPECTED[case] = dict(zip(c['radii'], got))
    return _EXPECTED[case]


def scene_expected():
    """(label, size) of neighbors_cases.scene() at SCENE_RADIUS"""
    if 'scene' not in _EXPECTED:
        _EXPECTED['scene'] = ref.clusters(nc.scene()[0], SCENE_RADIUS)
    return _EXPECTED['scene']


# ---- the stand-alone program -----------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_clusters_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'clusters_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=off', *flags, '-o', exe,
                               SOURCE])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def native(cols, queries, tmp_path, sanitize=False):
    """the program on [(name, array)] (the first column of a name counts; a missing x, y or z is told
    as such) and queries -- ('clusters', radius), ('filter', radius, mode, cluster_min), ('bounds', an
    array of shape (m, 12)) -> [(label, size) or REFUSED | rows or REFUSED | an (m, 2) array of
    far_bound and box_bound]"""
    first = {}
    for k, a in cols:
        first.setdefault(k, np.ascontiguousarray(a))
    n = len(next(iter(first.values()))) if first else 0
    src, out = tmp_path / 'in.bin', tmp_path / 'out.bin'
    count = 0
    with open(src, 'wb') as f:
        f.write(struct.pack('<Q', n))
        for k in 'xyz':
            if k in first:
                f.write(struct.pack('<i', PLY_CODE[first[k].dtype]) + first[k].tobytes())
            else:
                f.write(struct.pack('<i', 0))
        body = []
        for q in queries:
            if q[0] == 'clusters':
                body.append(struct.pack('<id', 1, q[1]))
                count += 1
            elif q[0] == 'filter':
                body.append(struct.pack('<idid', 2, q[1], q[2], q[3]))
                count += 1
            else:
                b = np.zeros(len(q[1]), np.dtype([('k', '<i4'), ('b', '<f8', (12,))]))
                b['k'], b['b'] = 3, q[1]
                body.append(b.tobytes())
                count += len(b)
        f.write(struct.pack('<I', count) + b''.join(body))
    r = subprocess.run([harness(sanitize), str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    raw = out.read_bytes()
    at = 0
    res = []
    for q in queries:
        if q[0] == 'clusters':
            status = struct.unpack_from('<Q', raw, at)[0]
            at += 8
            if status == REFUSED:
                res.append(REFUSED)
                continue
            assert status == 0
            res.append((np.frombuffer(raw, np.uint32, n, at).copy(), np.frombuffer(raw, np.uint32, n, at + 4 * n).copy()))
            at += 8 * n
        elif q[0] == 'filter':
            m = struct.unpack_from('<Q', raw, at)[0]
            at += 8
            if m == REFUSED:
                res.append(REFUSED)
                continue
            res.append(np.frombuffer(raw, np.uint32, m, at))
            at += 4 * m
        else:
            res.append(np.frombuffer(raw, np.float64, 2 * len(q[1]), at).reshape(-1, 2))
            at += 16 * len(q[1])
    assert at == len(raw)
    return res
