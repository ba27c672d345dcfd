"""Tables shared by tests/test_neighbors_cpu.py and tests/test_neighbors_gpu.py: the smallest inputs at
which each piece of include/st_abi.h's "neighbour distances and outliers" can go wrong, their expected
dist_k by tests/neighbors_ref.py (computed once per process), and the stand-alone program of
st_neighbors.h's serial host form (tests/native/neighbors_cpu_check.cpp).

cases(): {case: {'cols': [(name, array)], 'ks': [k, ...]}}.  BIG's expectation comes from the native
program (20,000 x 20,000 pairs), which the other cases cross-check against numpy."""
import atexit
import math
import os
import pathlib
import shutil
import struct
import subprocess
import tempfile

import numpy as np

import neighbors_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'tests', 'native', 'neighbors_cpu_check.cpp')
DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64]
PLY_CODE = {np.dtype(d): i + 1 for i, d in enumerate(DTYPES)}
KS = [1, 8, 32]
LENGTHS = [0, 1, 2, 8, 9, 32, 33, 63, 64, 65, 257]  # k and k + 1 for each k, the edges of a 64-row leaf
BIG = 'big_20000'
INF, NAN = math.inf, math.nan
REFUSED = 2 ** 64 - 1


def table(a, dtype=np.float32):
    a = np.asarray(a, np.float64).reshape(-1, 3)
    return [('x', a[:, 0].astype(dtype)), ('y', a[:, 1].astype(dtype)), ('z', a[:, 2].astype(dtype))]


def cases():
    if _CASES:
        return _CASES
    rng = np.random.default_rng(71)
    t = {}
    for n in LENGTHS:
        t[f'len_{n}'] = dict(cols=table(rng.normal(0, 1, (n, 3))))
    # two and three (five with 4-row leaves) levels of boxes above the leaves
    for n in (513, 4097):
        t[f'levels_{n}'] = dict(cols=table(rng.normal(0, 1, (n, 3))))
    t['levels_513_f64twin'] = dict(cols=[(k, a.astype(np.float64)) for k, a in t['levels_513']['cols']], twin='levels_513')
    # every row the same point: every d2 is +0; and more than 32 coincident rows inside a cloud: their
    # k-th best is 0 for every k, the walk prunes everything (the test is >=)
    t['coincident_all'] = dict(cols=table(np.tile([0.25, -1.5, 3.0], (200, 1))))
    cloud = rng.normal(0, 1, (500, 3))
    cloud[rng.permutation(500)[:40]] = cloud[0]
    t['coincident_in_cloud'] = dict(cols=table(cloud))
    # zero extent on two axes and on one: the key of that axis is 0, the boxes are flat
    line = np.zeros((300, 3))
    line[:, 0] = rng.normal(0, 1, 300)
    line[:, 1], line[:, 2] = 2.0, -1.0
    t['collinear'] = dict(cols=table(line))
    plane = rng.normal(0, 1, (300, 3))
    plane[:, 2] = 0.5
    t['coplanar'] = dict(cols=table(plane))
    # a 6 x 6 x 6 integer lattice, shuffled: exact ties at every k-th distance
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing='ij'), -1).reshape(-1, 3)
    t['lattice'] = dict(cols=table(rng.permutation(g)), ks=list(range(1, 33)))
    # scale contrast: a dense cluster of spread 1e-3 beside rows at 1e6 (all of the cluster shares one
    # key cell); coordinates near +-3e38, where d2 exceeds the float32 range; differences that are
    # subnormal in float32; float64 coordinates whose d2 overflows to +Infinity
    c = np.concatenate([0.5 + rng.normal(0, 1e-3, (300, 3)), rng.normal(0, 1e6, (60, 3))])
    t['dense_beside_far'] = dict(cols=table(rng.permutation(c)))
    t['near_f32_max'] = dict(cols=table(rng.uniform(-3e38, 3e38, (300, 3))))
    tiny = float(np.float32(1e-45))
    t['subnormal_f32'] = dict(cols=table(rng.integers(-2000, 2000, (300, 3)) * tiny))
    far = rng.normal(0, 1, (120, 3))
    far[rng.permutation(120)[:20]] *= 1e200
    t['overflow_f64'] = dict(cols=table(far, np.float64))
    # NaN and +-Infinity in any of the three axes, scattered through 700 rows
    a = rng.normal(0, 1, (700, 3))
    for v in (NAN, INF, -INF):
        for axis in range(3):
            a[rng.permutation(700)[:25], axis] = v
    t['nonfinite'] = dict(cols=table(a))
    t['nonfinite_f64twin'] = dict(cols=[(k, v.astype(np.float64)) for k, v in t['nonfinite']['cols']], twin='nonfinite')
    # fewer than k rows placed (for k = 8 and 32; k = 1 and the 5 placed rows: finite distances)
    few = rng.normal(0, 1, (20, 3))
    few[np.arange(5, 20), rng.integers(0, 3, 15)] = NAN
    t['few_placed'] = dict(cols=table(few))
    t['none_placed'] = dict(cols=table(np.full((70, 3), NAN)))
    # other column types: int16 / float64 / uint8, among columns the search does not read (a second x)
    t['mixed_types'] = dict(cols=[('w', rng.normal(0, 1, 515).astype(np.float32)),
                                  ('x', rng.integers(-300, 300, 515).astype(np.int16)), ('y', rng.normal(0, 100, 515)),
                                  ('z', rng.integers(0, 256, 515).astype(np.uint8)), ('x', np.zeros(515, np.float32))])
    big = np.concatenate([rng.normal(0, 1, (10_000, 3)), rng.uniform(-4, 4, (10_000, 3))])
    t[BIG] = dict(cols=table(rng.permutation(big)))
    for v in t.values():
        v.setdefault('ks', KS)
        v['n'] = len(v['cols'][0][1])
    _CASES.update(t)
    return _CASES


_CASES, _EXPECTED = {}, {}


def scene():
    """a cluster with floaters: 4,000 rows N(0, 1) and 40 rows U(-30, 30) as float32, shuffled ->
    ([(name, array)], the mask of the cluster rows)"""
    rng = np.random.default_rng(71)
    p = np.concatenate([rng.normal(0, 1, (4000, 3)), rng.uniform(-30, 30, (40, 3))]).astype(np.float32)
    perm = rng.permutation(4040)
    return table(p[perm]), perm < 4000


def expected(case):
    """{k: dist_k as float64 array} of a case, computed once per process"""
    if case not in _EXPECTED:
        c = cases()[case]
        if case == BIG:
            d = tempfile.mkdtemp(prefix='st_neighbors_big_')
            try:
                got = native(c['cols'], [('dist', k) for k in c['ks']], pathlib.Path(d))
            finally:
                shutil.rmtree(d, ignore_errors=True)
            _EXPECTED[case] = dict(zip(c['ks'], got))
        else:
            _EXPECTED[case] = ref.dist_ks(c['cols'], c['ks'])
    return _EXPECTED[case]


# ---- the stand-alone program -----------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_neighbors_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'neighbors_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', '-ffp-contract=off', *flags, '-o', exe,
                               SOURCE])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def native(cols, queries, tmp_path, sanitize=False):
    """the program on [(name, array)] (the first column of a name counts) and queries -- ('dist', k),
    ('outliers', k, mode, value), ('bound', twelve numbers) -> [dist array | rows or REFUSED | bound]"""
    first = {}
    for k, a in cols:
        first.setdefault(k, np.ascontiguousarray(a))
    n = len(first['x'])
    src, out = tmp_path / 'in.bin', tmp_path / 'out.bin'
    with open(src, 'wb') as f:
        f.write(struct.pack('<Q', n))
        for k in 'xyz':
            f.write(struct.pack('<i', PLY_CODE[first[k].dtype]) + first[k].tobytes())
        f.write(struct.pack('<I', len(queries)))
        for q in queries:
            if q[0] == 'dist':
                f.write(struct.pack('<ii', 1, q[1]))
            elif q[0] == 'outliers':
                f.write(struct.pack('<iiid', 2, q[1], q[2], q[3]))
            else:
                f.write(struct.pack('<i12d', 3, *q[1]))
    r = subprocess.run([harness(sanitize), str(src), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    raw = out.read_bytes()
    at = 0
    res = []
    for q in queries:
        if q[0] == 'dist':
            res.append(np.frombuffer(raw, np.float64, n, at))
            at += 8 * n
        elif q[0] == 'outliers':
            count = struct.unpack_from('<Q', raw, at)[0]
            at += 8
            if count == REFUSED:
                res.append(REFUSED)
                continue
            res.append(np.frombuffer(raw, np.uint32, count, at))
            at += 4 * count
        else:
            res.append(struct.unpack_from('<d', raw, at)[0])
            at += 8
    assert at == len(raw)
    return res
