"""The Node host's processDataTable with this project's own action kinds -- filterBox, filterSphere,
decimate (count and fraction) and orderByImportance, alone and after a transform -- on a 5,000-row
table of mixed column types: the processed table equals Context.process byte for byte
(tests/js/importance_actions.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import splat_hip as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, 'splat-transform_amd', 'napi', 'build', 'addon.node')
NODE = shutil.which('node')

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason='node not installed')]

CODE = {np.dtype(np.float32): 'f4', np.dtype(np.float64): 'f8', np.dtype(np.uint16): 'u2', np.dtype(np.int8): 'i1'}


def table():
    rng = np.random.default_rng(41)
    n = 5000
    cols = [(k, rng.normal(0, 2, n).astype(np.float32)) for k in ('x', 'y', 'z', 'f_dc_0')]
    cols += [(f'scale_{i}', (rng.random(n) * 5 - 7).astype(np.float32)) for i in range(2)]
    cols += [('scale_2', rng.random(n) * 5 - 7), ('opacity', rng.normal(0, 2, n).astype(np.float32)),
             ('rot_0', rng.normal(0, 1, n).astype(np.float32)), ('id', rng.integers(0, 60000, n).astype(np.uint16))]
    d = dict(cols)
    d['opacity'][rng.permutation(n)[:200]] = np.nan
    d['x'][7] = np.nan
    d['scale_2'][11] = np.inf
    return cols


CASES = [
    ('box', [{'kind': 'filterBox', 'min': [-1, -2.5, -3], 'max': [2, 2.5, float('inf')]}]),
    ('sphere', [{'kind': 'filterSphere', 'center': [0.5, 0, -0.5], 'radius': 2.75}]),
    ('count', [{'kind': 'decimate', 'count': 1234}]),
    ('fraction', [{'kind': 'decimate', 'fraction': 1 / 3}]),
    ('order', [{'kind': 'orderByImportance'}]),
    ('chain', [{'kind': 'translate', 'value': [1, 0, -1]}, {'kind': 'filterNaN'},
               {'kind': 'filterSphere', 'center': [1, 0, -1], 'radius': 4}, {'kind': 'decimate', 'fraction': 0.5},
               {'kind': 'orderByImportance'}]),
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
        # the reference's CLI hands Vec3 values to translate; the new kinds take arrays or Vec3
        js = [dict(a, value=dict(zip('xyz', a['value']))) if a['kind'] == 'translate' else a for a in acts]
        man['cases'].append({'name': name, 'actions': js})
    # JSON has no Infinity; JSON.parse reads 1e999 as it
    text = json.dumps(man).replace('Infinity', '1e999')
    (tmp_path / 'manifest.json').write_text(text)
    r = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'importance_actions.js'), str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout)
    ctx = sh.Context(0)
    try:
        for name, acts in CASES:
            want = ctx.process([(k, a.copy()) for k, a in cols], acts)
            rows = len(want[0][1])
            assert got[name]['names'] == [k for k, _ in want] and got[name]['rows'] == rows, name
            assert 0 < rows < 5000 or name == 'order'
            raw = (tmp_path / f'out_{name}.bin').read_bytes()
            assert raw == b''.join(a.tobytes() for _, a in want), name
    finally:
        ctx.close()
