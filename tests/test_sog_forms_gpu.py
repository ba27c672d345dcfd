"""The one-call writeSog forms from host memory agree with each other: st_sog_bundle, st_sog_file and
st_sog_bundle_process (no actions) give one archive, st_sog and st_sog_process (no actions) one set
of textures and meta, st_dev_sog_bundle of st_sog's textures that same archive -- on one device and
on the default group (ST_DEFAULT_GROUP_RANKS=2: two host-staged ranks on this one GPU), which is
read once per process, so each setting runs in a child."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHILD = r'''
import ctypes, hashlib, json, os, sys
import numpy as np
one_device = not os.environ.get('ST_DEFAULT_GROUP_RANKS')
if one_device:  # torch's HIP runtime has to come up before the library's (as under pytest and the bench)
    import torch
    torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import splat_hip as sh
n = 30_011
rng = np.random.default_rng(8)
cols = {k: rng.normal(0, 1, n).astype(np.float32) for k in
        ['x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
         'rot_0', 'rot_1', 'rot_2', 'rot_3'] + ['f_rest_%d' % i for i in range(9)]}
draws = np.random.default_rng(9).random(1 << 18)
ctx = sh.Context(0)
n_dev = ctypes.c_int32(0)
sh.check(sh.lib().st_get_devices(ctypes.byref(n_dev)))
sha = lambda b: hashlib.sha256(b).hexdigest()


def tex_digest(tex, meta):
    h = hashlib.sha256()
    for k in ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_labels', 'shN_centroids'):
        h.update(np.ascontiguousarray(tex[k]).tobytes())
    h.update(bytes(meta))
    return h.hexdigest()


res = {'ranks': n_dev.value, 'archives': {}, 'textures': {}}
zipb, used = ctx.sog_bundle(cols, 2, draws, 0, 0)
res['archives']['st_sog_bundle'] = [sha(zipb), used]
used, size = ctx.sog_file(cols, 2, draws, sys.argv[2], 0, 0)
data = open(sys.argv[2], 'rb').read()
assert len(data) == size
res['archives']['st_sog_file'] = [sha(data), used]
zipb, used = ctx.sog_bundle_process(cols, [], 2, draws, 0, 0)
res['archives']['st_sog_bundle_process'] = [sha(zipb), used]
tex, meta, used = ctx.sog(cols, 2, draws)
res['textures']['st_sog'] = [tex_digest(tex, meta), used]
if one_device:
    dtex = {k: torch.from_numpy(np.ascontiguousarray(v)).to('cuda:0') for k, v in tex.items()}
    torch.cuda.synchronize()
    res['archives']['st_dev_sog_bundle'] = [sha(ctx.dev_sog_bundle(meta, n, dtex, 0, 0)), used]
tex, meta, used = ctx.sog_process(cols, [], 2, draws)
res['textures']['st_sog_process'] = [tex_digest(tex, meta), used]
print(json.dumps(res))
'''


def test_host_sog_forms_agree_on_one_device_and_on_the_default_group(tmp_path):
    py = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'splat-transform_amd', 'py')
    out = {}
    for ranks in ('', '2'):
        env = dict(os.environ, ST_DEFAULT_GROUP_RANKS=ranks)
        env.pop('ST_NUM_GPUS', None)
        r = subprocess.run([sys.executable, '-c', _CHILD, py, str(tmp_path / f'forms{ranks}.sog')],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        out[ranks] = json.loads(r.stdout.strip().splitlines()[-1])
        print(ranks or '1', out[ranks])
    assert out['']['ranks'] == 1 and out['2']['ranks'] == 2
    assert set(out['']['archives']) == {'st_sog_bundle', 'st_sog_file', 'st_sog_bundle_process', 'st_dev_sog_bundle'}
    assert set(out['2']['archives']) == {'st_sog_bundle', 'st_sog_file', 'st_sog_bundle_process'}
    archive = out['']['archives']['st_sog_bundle']
    textures = out['']['textures']['st_sog']
    for ranks in ('', '2'):
        for form, got in out[ranks]['archives'].items():
            assert got == archive, (ranks, form)
        assert set(out[ranks]['textures']) == {'st_sog', 'st_sog_process'}
        for form, got in out[ranks]['textures'].items():
            assert got == textures, (ranks, form)
