"""The Node host's processDataTable with filterClusters -- the minSize and the keep: 'largest' spelling,
alone and in a chain after a transform, a filterNaN and a filterOutliers -- on a 4,040-row table of
mixed column types (a cluster with floaters): the processed table equals Context.process byte for byte
(tests/js/cluster_actions.js).  The radii were picked on the CPU with tests/clusters_ref.py so that
every case leaves some rows and drops some."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import neighbors_cases as nc
import splat_hip as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, 'splat-transform_amd', 'napi', 'build', 'addon.node')
NODE = shutil.which('node')

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason='node not installed')]

CODE = {np.dtype(np.float32): 'f4', np.dtype(np.float64): 'f8', np.dtype(np.uint16): 'u2', np.dtype(np.int8): 'i1'}


def table():
    rng = np.random.default_rng(43)
    (_, x), (_, y), (_, z) = nc.scene()[0]
    n = len(x)
    cols = [('id', rng.integers(0, 60000, n).astype(np.uint16)), ('x', x.copy()), ('y', y.astype(np.float64)), ('z', z.copy()),
            ('f_dc_0', rng.normal(0, 1, n).astype(np.float32)), ('flag', rng.integers(-100, 100, n).astype(np.int8))]
    cols[1][1][7] = np.nan
    cols[3][1][11] = np.inf
    cols[4][1][rng.permutation(n)[:200]] = np.nan
    return cols


CASES = [
    ('min_size', [{'kind': 'filterClusters', 'radius': 0.3, 'minSize': 5}]),
    ('largest', [{'kind': 'filterClusters', 'radius': 0.3, 'keep': 'largest'}]),
    ('singletons_go', [{'kind': 'filterClusters', 'radius': 0.15, 'minSize': 2}]),
    ('chain', [{'kind': 'translate', 'value': [1, 0, -1]}, {'kind': 'filterNaN'},
               {'kind': 'filterOutliers', 'k': 8, 'sigma': 1.0}, {'kind': 'filterClusters', 'radius': 0.25, 'keep': 'largest'},
               {'kind': 'filterClusters', 'radius': 0.1, 'minSize': 3}]),
]


def test_node_process_equals_context_process(tmp_path):
    if not os.path.exists(ADDON):
        subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'splat-transform_amd', 'napi')])
    cols = table()
    man = {'columns': [], 'cases': []}
    at = 0
    with open(tmp_path / 'in.bin', 'wb') as f:
        for k, a in cols:
            man['columns'].append({'name': k, 'dtype': CODE[a.dtype], 'offset': at, 'nbytes': a.nbytes})
            f.write(a.tobytes())
            at += a.nbytes
    for name, acts in CASES:
        # the reference's CLI hands Vec3 values to translate
        js = [dict(a, value=dict(zip('xyz', a['value']))) if a['kind'] == 'translate' else a for a in acts]
        man['cases'].append({'name': name, 'actions': js})
    (tmp_path / 'manifest.json').write_text(json.dumps(man))
    r = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'cluster_actions.js'), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    ctx = sh.Context(0)
    try:
        for name, acts in CASES:
            want = ctx.process([(k, a.copy()) for k, a in cols], acts)
            rows = len(want[0][1])
            assert got[name]['names'] == [k for k, _ in want] and got[name]['rows'] == rows, name
            assert 0 < rows < 4040, name
            raw = (tmp_path / f'out_{name}.bin').read_bytes()
            assert raw == b''.join(a.tobytes() for _, a in want), name
    finally:
        ctx.close()
