"""Every host form on the unfilled columns of a resident read (st_ply_read_resident).

The columns' values exist only in HBM, in the reading context's mirror list (st_ctx::HostMirror,
lazy).  The contract: the writeSog host forms (st_sog, st_sog_bundle, st_sog_file) read the device
copy; every other host form copies the column down before it uploads it (staged_h2d on the owning
context); a context other than the reader's, and an explicit group, refuse such a column.

Each case reads the file twice -- eagerly (`ref`) and resident (`cols`) --, overwrites every array
of `cols` with a poison value, and calls the form once on each.  Everything returned or written
must be bit-identical, and afterwards the columns the form was given hold the read's values (or,
for the writeSog forms, still the poison), the others still the poison; a writeSog and a
materialize of every column then show that the mirror list is consistent.  No tolerance anywhere:
bits, bytes, digests and counts against the same call on the eagerly read table.

The default group and the refusals run in two child processes (the group is read once per
process), as in test_sog_forms_gpu.py."""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import splat_hip as sh
from golden_io import Golden
from test_ply_cpu import compressed_file

pytestmark = pytest.mark.gpu

N = 4_099  # every column under 1 MiB: the staged copies' direct path
BIG = 262_147  # 1 MiB + 12 B per float column: the staged path through the pinned slots
ITERS = 2
BASE = ('x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
        'rot_0', 'rot_1', 'rot_2', 'rot_3')
T23 = BASE + tuple(f'f_rest_{i}' for i in range(9))
MOVED = ('x', 'y', 'z', 'rot_0', 'rot_1', 'rot_2', 'rot_3', 'scale_0', 'scale_1', 'scale_2') + \
    tuple(f'f_rest_{i}' for i in range(45))
MIXED = ('x', 'd', 'u', 'c', 's', 'us', 'i', 'ui', 'y')
FPOISON = -12345.5
IPOISON = 0x5B  # every byte of an integer column


@pytest.fixture(scope='module')
def ctx():
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    c = sh.Context(0)
    c.set_stream(s.cuda_stream)
    yield c
    c.close()


def _ply(path, n, seed):
    import bench
    rng = np.random.default_rng(seed)
    names = bench.PLY_ORDER
    rows = np.zeros(n, np.dtype([(k, '<f4') for k in names]))
    for k in names:
        rows[k] = rng.normal(0, 0.1 if k.startswith('f_rest') else 1, n)
    rows['scale_0'] = rng.random(n) * 5 - 7
    head = ('ply\nformat binary_little_endian 1.0\n' + f'element vertex {n}\n' +
            ''.join(f'property float {k}\n' for k in names) + 'end_header\n').encode()
    with open(path, 'wb') as f:
        f.write(head + rows.tobytes())


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('resident_forms')
    out = {'small': str(d / 'small.ply'), 'big': str(d / 'big.ply'), 'mixed': str(d / 'mixed.ply'),
           'comp': str(d / 'comp.ply')}
    _ply(out['small'], N, 21)
    _ply(out['big'], BIG, 22)
    with open(out['mixed'], 'wb') as f:
        f.write(Golden('ply_io')['mixed_file'].tobytes())
    with open(out['comp'], 'wb') as f:
        f.write(compressed_file('sh3'))
    return out


def _draws():
    return np.random.default_rng(9).random(1 << 18)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _poison(cols):
    """every array overwritten after the read: the library must never read these bytes"""
    for v in cols.values():
        if v.dtype.kind == 'f':
            v[:] = FPOISON
        else:
            v.view(np.uint8)[:] = IPOISON


def _is_poison(v):
    if v.dtype.kind == 'f':
        return bool(np.all(v == v.dtype.type(FPOISON)))
    return bool(np.all(v.view(np.uint8) == IPOISON))


def _read_pair(ctx, path, element='vertex'):
    """(ref, cols): the element read eagerly, and read resident with every array poisoned"""
    ref = dict(ctx.read_ply(path)[1])
    res = dict(ctx.read_ply(path, resident=True)[1])
    for cols in res.values():
        _poison(cols)
    return (ref, res) if element is None else (ref[element], res[element])


def _norm(v):
    """a form's result as something `==` compares by bits"""
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, ctypes.Structure):
        return bytes(v)
    if isinstance(v, dict):
        return [(k, _norm(x)) for k, x in v.items()]
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    if isinstance(v, float):
        return struct.pack('<d', v)
    return v


def _final_sog(ctx, table, path, monkeypatch):
    """writeSog of the T23 columns with the eager mirrors' compare off (ST_HOST_MIRROR=0: only lazy
    columns run from HBM) -> (archive, draws used, columns reused)"""
    monkeypatch.setenv('ST_HOST_MIRROR', '0')
    used, size = ctx.sog_file({k: table[k] for k in T23}, ITERS, _draws(), path, 0x1234, 0x5678)
    monkeypatch.delenv('ST_HOST_MIRROR')
    data = open(path, 'rb').read()
    assert len(data) == size
    return data, used, ctx.host_reuse()[0]


def _materialized_equal(ctx, cols, ref):
    for k in cols:
        assert _same(ctx.materialize(cols[k]), ref[k]), k


# ---- the forms: fn(ctx, t, out) on the dict `t` of the columns the case passes; `out` is a file of
# the call's own.  Returns whatever the form returned, and the file's bytes when it wrote one.
def _params():
    return sh.transform_params((1.0, -2.0, 0.5), (0.0, 0.0, 0.0, 1.0), 2.0)


ACTS = [{'kind': 'translate', 'value': (1.0, -2.0, 0.5)}, {'kind': 'filterNaN'}]
CHAIN = [{'kind': 'scale', 'value': 2.0}, {'kind': 'filterNaN'}, {'kind': 'filterBands', 'value': 0}]
TEMPLATE = ('<html><head><link rel="stylesheet" href="./index.css"></head><body>'
            '<script type="module" src="./index.js"></script></body></html>',
            'body { margin: 0; }', 'const content = fetch(contentUrl);\n')


def _filed(call):
    def fn(ctx, t, out):
        ret = call(ctx, t, out)
        return ret, open(out, 'rb').read()
    return fn


def _transform(ctx, t, out):
    ctx.transform(t, _params())
    return t


def _transform_mixed(ctx, t, out):  # st_transform_t: float64 / int32 / int16 columns under the moved names
    ctx.transform({'x': t['d'], 'y': t['i'], 'z': t['s']}, _params())
    return t


def _pack(ctx, t, out):
    order = np.random.default_rng(3).permutation(len(t['x'])).astype(np.uint32)
    return ctx.pack_compressed(t, order, 9)


def _sog_file(ctx, t, out):
    return ctx.sog_file(t, ITERS, _draws(), out, 0x1234, 0x5678)


def _decompress(ctx, t, out):
    return ctx.decompress_ply({k: t[k] for k in sh.CHUNK_COLS}, {k: t[k] for k in sh.VERTEX_COLS},
                              [t[f'f_rest_{i}'] for i in range(len(t) - 22)])


# id -> (file, keys, fn, kind); kind 'down': the columns come down; 'sog': they stay in HBM
FORMS = {
    'transform': ('small', MOVED, _transform, 'down'),
    'transform_t': ('mixed', ('d', 'i', 's'), _transform_mixed, 'down'),
    'filter_finite': ('small', BASE[:6], lambda c, t, o: c.filter_finite(t), 'down'),
    'filter_nan': ('small', BASE[3:9], lambda c, t, o: c.filter_nan(list(t.items())), 'down'),
    'filter_nan_t': ('mixed', MIXED, lambda c, t, o: c.filter_nan(list(t.items())), 'down'),
    'morton_order': ('small', ('x', 'y', 'z'), lambda c, t, o: c.morton_order(t['x'], t['y'], t['z']), 'down'),
    'morton_order_t': ('mixed', ('d', 'i', 'us'), lambda c, t, o: c.morton_order(t['d'], t['i'], t['us']), 'down'),
    'pack_compressed': ('small', T23, _pack, 'down'),
    'kmeans': ('small', ('x', 'y', 'z'), lambda c, t, o: c.kmeans(list(t.values()), 64, ITERS, _draws()), 'down'),
    'cluster1d': ('small', ('f_dc_0', 'f_dc_1', 'f_dc_2'),
                  lambda c, t, o: c.cluster1d(list(t.values()), ITERS, _draws()), 'down'),
    'sog': ('small', T23, lambda c, t, o: c.sog(t, ITERS, _draws()), 'sog'),
    'sog_bundle': ('small', T23, lambda c, t, o: c.sog_bundle(t, ITERS, _draws(), 1, 2), 'sog'),
    'sog_file': ('small', T23, _filed(_sog_file), 'sog'),
    'sog_process': ('small', T23, lambda c, t, o: c.sog_process(t, [], ITERS, _draws()), 'down'),
    'sog_process_acts': ('small', T23, lambda c, t, o: c.sog_process(t, ACTS, ITERS, _draws()), 'down'),
    'sog_bundle_process': ('small', T23, lambda c, t, o: c.sog_bundle_process(t, [], ITERS, _draws(), 1, 2), 'down'),
    'sog_bundle_process_acts': ('small', T23,
                                lambda c, t, o: c.sog_bundle_process(t, ACTS, ITERS, _draws(), 1, 2), 'down'),
    'process': ('small', T23, lambda c, t, o: c.process(t, CHAIN), 'down'),
    'process_t': ('mixed', MIXED, lambda c, t, o: c.process(t, [{'kind': 'filterNaN'}]), 'down'),
    'compressed_ply': ('small', T23, lambda c, t, o: c.compressed_ply(t, ACTS), 'down'),
    'compressed_ply_file': ('small', T23, _filed(lambda c, t, o: c.compressed_ply_file(t, ACTS, o, '1.2.3')), 'down'),
    'ply_rows_file': ('small', T23, _filed(lambda c, t, o: c.ply_rows_file(t, o)), 'down'),
    'ply_rows_file_t': ('mixed', MIXED, _filed(lambda c, t, o: c.ply_rows_file(t, o)), 'down'),
    'ply_file': ('small', T23, _filed(lambda c, t, o: c.ply_file(t, ACTS, o, ('a comment',))), 'down'),
    'ply_file_t': ('mixed', MIXED, _filed(lambda c, t, o: c.ply_file(t, [{'kind': 'filterNaN'}], o)), 'down'),
    'csv_file': ('small', BASE, _filed(lambda c, t, o: c.csv_file(t, ACTS, o)), 'down'),
    'csv_file_t': ('mixed', MIXED, _filed(lambda c, t, o: c.csv_file(t, [], o)), 'down'),
    'html_file': ('small', T23, _filed(lambda c, t, o: c.html_file(t, ACTS, TEMPLATE, o, version='1.2.3')), 'down'),
    'splat_file': ('small', T23, _filed(lambda c, t, o: c.splat_file(t, ACTS, o)), 'down'),
    'spz_file_raw': ('small', T23, _filed(lambda c, t, o: c.spz_file(t, ACTS, o, gzip_level=0)), 'down'),
    'spz_file_device': ('small', T23, _filed(lambda c, t, o: c.spz_file(t, ACTS, o, deflate='device')), 'down'),
    'ksplat_file': ('small', T23, _filed(lambda c, t, o: c.ksplat_file(t, ACTS, o, mode=1)), 'down'),
    'summary': ('small', BASE[:6], lambda c, t, o: c.summary(t), 'down'),
    'summary_t': ('mixed', MIXED, lambda c, t, o: c.summary(t), 'down'),
    # the staged path: every float column is 1 MiB + 12 B
    'transform_big': ('big', MOVED[:10], _transform, 'down'),
    'process_big': ('big', T23, lambda c, t, o: c.process(t, CHAIN), 'down'),
    'ply_file_big': ('big', BASE, _filed(lambda c, t, o: c.ply_file(t, ACTS, o)), 'down'),
    'summary_big': ('big', ('x', 'opacity', 'f_rest_44'), lambda c, t, o: c.summary(t), 'down'),
    'sog_bundle_big': ('big', T23, lambda c, t, o: c.sog_bundle(t, ITERS, _draws(), 1, 2), 'sog'),
}


@pytest.mark.parametrize('form', list(FORMS))
def test_form_on_resident_columns_equals_the_eager_read(ctx, files, tmp_path, monkeypatch, form):
    which, keys, fn, kind = FORMS[form]
    ref, cols = _read_pair(ctx, files[which])
    assert set(keys) <= set(cols) and all(_is_poison(v) for v in cols.values())
    got = _norm(fn(ctx, {k: cols[k] for k in keys}, str(tmp_path / 'got')))
    reuse = ctx.host_reuse()
    want = _norm(fn(ctx, {k: ref[k] for k in keys}, str(tmp_path / 'want')))
    assert got == want
    if kind == 'sog':
        assert reuse == (len(keys), len(keys) * len(ref[keys[0]]) * 4), reuse
    for k in cols:
        if k in keys and kind == 'down':
            assert _same(cols[k], ref[k]), k  # copied down (and, where the form writes it, equally written)
        else:
            assert _is_poison(cols[k]), k  # never read, never filled
    if which != 'mixed':
        down = set(keys) if kind == 'down' else set()
        g = _final_sog(ctx, cols, str(tmp_path / 'a.sog'), monkeypatch)
        assert g[2] == len([k for k in T23 if k not in down]), g[2]
        w = _final_sog(ctx, ref, str(tmp_path / 'b.sog'), monkeypatch)
        assert w[2] == 0 and g[:2] == w[:2]
    _materialized_equal(ctx, cols, ref)


def test_decompress_ply_on_resident_elements(ctx, files):
    """st_decompress_ply fed from a resident read of a compressed .ply: float32 chunk columns, uint32
    vertex columns, uint8 SH columns, every one lazy"""
    ref, res = _read_pair(ctx, files['comp'], element=None)
    flat = lambda els: {k: v for e in ('chunk', 'vertex', 'sh') for k, v in els[e].items()}
    cols, want_cols = flat(res), flat(ref)
    assert len(cols) == 18 + 4 + len(res['sh']) and len(res['sh']) in (9, 24, 45)
    got = _norm(_decompress(ctx, cols, None))
    want = _norm(_decompress(ctx, want_cols, None))
    assert got == want
    for k in cols:
        assert _same(cols[k], want_cols[k]), k
    _materialized_equal(ctx, cols, want_cols)


def test_a_view_of_a_resident_column_brings_the_whole_column_down(ctx, files, tmp_path, monkeypatch):
    ref, cols = _read_pair(ctx, files['small'])
    got = ctx.summary({'x': cols['x'][100:2100]})
    want = ctx.summary({'x': ref['x'][100:2100]})
    assert _norm(got) == _norm(want)
    assert _same(cols['x'], ref['x'])
    assert all(_is_poison(v) for k, v in cols.items() if k != 'x')
    g = _final_sog(ctx, cols, str(tmp_path / 'a.sog'), monkeypatch)
    w = _final_sog(ctx, ref, str(tmp_path / 'b.sog'), monkeypatch)
    assert g[2] == len(T23) - 1 and w[2] == 0 and g[:2] == w[:2]
    _materialized_equal(ctx, cols, ref)


def test_a_partial_overwrite_keeps_the_rest_of_a_resident_column(ctx, files, tmp_path, monkeypatch):
    """st_filter_nan writing h = n // 2 rows into the [:h] views of lazy columns: rows [h:) exist
    only in HBM, so the column is copied down before its mirror is dropped"""
    ref, cols = _read_pair(ctx, files['small'])
    keys, h = ('x', 'opacity', 'f_rest_3'), N // 2
    rng = np.random.default_rng(31)
    src = [(k, rng.normal(0, 1, h).astype(np.float32)) for k in keys]
    dst = [(k, cols[k][:h]) for k in keys]
    ts, td = sh.make_ttable(src), sh.make_ttable(dst)
    m = ctypes.c_uint64()
    sh.check(sh.lib().st_filter_nan(ctx.h, ctypes.byref(ts), ctypes.byref(td), ctypes.byref(m)))
    assert m.value == h
    for k, a in src:
        assert _same(cols[k][:h], a), k
        assert _same(cols[k][h:], ref[k][h:]), k
        ref[k][:h] = a  # the table the caller now holds
    assert all(_is_poison(v) for k, v in cols.items() if k not in keys)
    g = _final_sog(ctx, cols, str(tmp_path / 'a.sog'), monkeypatch)
    w = _final_sog(ctx, ref, str(tmp_path / 'b.sog'), monkeypatch)
    assert g[2] == len(T23) - len(keys) and g[:2] == w[:2]
    _materialized_equal(ctx, cols, ref)


# ---- the default group, an explicit group and a foreign context, one child per group setting ----
_CHILD = r'''
import ctypes, hashlib, json, os, sys
import numpy as np
group = bool(os.environ.get('ST_DEFAULT_GROUP_RANKS'))
if not group:  # torch's HIP runtime has to come up before the library's (as under pytest and the bench)
    import torch
    torch.cuda.init()
sys.path.insert(0, sys.argv[1])
import splat_hip as sh
tmp = sys.argv[2]
n = 30_011
rng = np.random.default_rng(8)
names = ['x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
         'rot_0', 'rot_1', 'rot_2', 'rot_3'] + ['f_rest_%d' % i for i in range(9)]
rows = np.zeros(n, np.dtype([(k, '<f4') for k in names]))
for k in names:
    rows[k] = rng.normal(0, 1, n)
src = os.path.join(tmp, 'in.ply')
with open(src, 'wb') as f:
    f.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % n +
             ''.join('property float %s\n' % k for k in names) + 'end_header\n').encode() + rows.tobytes())
draws = np.random.default_rng(9).random(1 << 18)
ctx = sh.Context(0)
n_dev = ctypes.c_int32(0)
sh.check(sh.lib().st_get_devices(ctypes.byref(n_dev)))
sha = lambda b: hashlib.sha256(b).hexdigest()
POISON = np.float32(-12345.5)


def tex_digest(tex, meta):
    h = hashlib.sha256()
    for k in ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_labels', 'shN_centroids'):
        h.update(np.ascontiguousarray(tex[k]).tobytes())
    h.update(bytes(meta))
    return h.hexdigest()


def eager(c=ctx):
    return dict(c.read_ply(src)[1])['vertex']


def resident(c=ctx):
    cols = dict(c.read_ply(src, resident=True)[1])['vertex']
    for v in cols.values():
        v[:] = POISON  # the library must never read these bytes
    return cols


def poison(cols):
    return all(bool(np.all(v == POISON)) for v in cols.values())


def sog_file(c, cols, name):
    path = os.path.join(tmp, name)
    used, size = c.sog_file(cols, 2, draws, path, 0, 0)
    data = open(path, 'rb').read()
    assert len(data) == size
    return [sha(data), used]


def summary_bits(s):
    return {k: np.array(tuple(v), np.float64).tobytes().hex() for k, v in s.items()}


FORMS = {
    'st_sog_bundle': lambda t: (lambda r: [sha(r[0]), r[1]])(ctx.sog_bundle(t, 2, draws, 0, 0)),
    'st_sog_file': lambda t: sog_file(ctx, t, 'forms.sog'),    'st_sog': lambda t: (lambda r: [tex_digest(r[0], r[1]), r[2]])(ctx.sog(t, 2, draws)),
    'st_sog_process': lambda t: (lambda r: [tex_digest(r[0], r[1]), r[2]])(ctx.sog_process(t, [], 2, draws)),
    'st_sog_bundle_process': lambda t: (lambda r: [sha(r[0]), r[1]])(ctx.sog_bundle_process(t, [], 2, draws, 0, 0)),
}
res = {'ranks': n_dev.value, 'forms': {}, 'reuse': {}}
if not group:
    os.environ['ST_HOST_MIRROR'] = '0'
for name, fn in FORMS.items():
    t = resident() if group else eager()  # a fresh read for each form: the one before brought its columns down
    try:
        res['forms'][name] = fn(t)
    except sh.StError as e:  # reported, so that the parent's comparison fails for this form alone
        res['forms'][name] = ['StError', str(e)]
    res['reuse'][name] = list(ctx.host_reuse())
os.environ.pop('ST_HOST_MIRROR', None)


def refused(call):
    """what a call that must fail with ST_ERR_ARG did"""
    try:
        call()
    except sh.StError as e:
        return {'raised': True, 'code': e.code, 'resident': 'resident' in str(e),
                'materialize': 'st_ply_materialize' in str(e)}
    return {'raised': False}


def owner_still_reuses(cols):
    """nothing was written into the columns, and the owner's writeSog still runs on all of them"""
    ok = poison(cols)
    got = sog_file(ctx, cols, 'owner.sog')
    return {'poison': ok and poison(cols), 'reuse': ctx.host_reuse()[0], 'archive': got}


if not group:
    ref = eager()
    want_summary = summary_bits(ctx.summary({'x': ref['x']}))
    # an explicit group: its ranks' contexts did not read the columns
    g = sh.Group([0, 0], host_staged=True)
    cols = resident()
    ex = {'first': refused(lambda: g.sog_bundle([cols], 2, draws, 0, 0)), 'owner': owner_still_reuses(cols)}
    for v in cols.values():
        ctx.materialize(v)
    zipb, used = g.sog_bundle([cols], 2, draws, 0, 0)
    ex['after'] = [sha(zipb), used]
    g.close()
    res['explicit_group'] = ex
    # a second context given the first one's resident columns
    other = sh.Context(0)
    cols = resident()
    fo = {'summary': refused(lambda: other.summary({'x': cols['x']})),
          'sog_bundle': refused(lambda: other.sog_bundle(cols, 2, draws, 0, 0))}
    mine = resident(other)  # beside resident columns of its own (resident_table's uploads)
    fo['sog_bundle_mixed'] = refused(lambda: other.sog_bundle(dict(mine, x=cols['x']), 2, draws, 0, 0))
    del mine
    fo['owner'] = owner_still_reuses(cols)
    for v in cols.values():
        ctx.materialize(v)
    fo['summary_after'] = summary_bits(other.summary({'x': cols['x']})) == want_summary
    zipb, used = other.sog_bundle(cols, 2, draws, 0, 0)
    fo['after'] = [sha(zipb), used]
    other.close()
    res['foreign'] = fo
print(json.dumps(res))
'''


@pytest.fixture(scope='module')
def children(tmp_path_factory):
    py = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'splat-transform_amd', 'py')
    out = {}
    for ranks in ('', '2'):
        d = tmp_path_factory.mktemp('resident_child' + ranks)
        env = dict(os.environ, ST_DEFAULT_GROUP_RANKS=ranks)
        for k in ('ST_NUM_GPUS', 'ST_HOST_MIRROR'):
            env.pop(k, None)
        r = subprocess.run([sys.executable, '-c', _CHILD, py, str(d)], capture_output=True, text=True, timeout=300,
                           env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        out[ranks] = json.loads(r.stdout.strip().splitlines()[-1])
        print(ranks or '1', out[ranks])
    assert out['']['ranks'] == 1 and out['2']['ranks'] == 2
    return out


HOST_SOG = ('st_sog_bundle', 'st_sog_file', 'st_sog')


@pytest.mark.parametrize('form', HOST_SOG + ('st_sog_process', 'st_sog_bundle_process'))
def test_default_group_on_resident_columns_equals_one_device_on_the_eager_read(children, form):
    """the group's ranks upload host bytes: host_sog copies the resident columns down first"""
    assert children['2']['forms'][form] == children['']['forms'][form]
    assert children['']['reuse'][form] == [0, 0] or form not in HOST_SOG
    if form in HOST_SOG:
        assert children['2']['reuse'][form] == [0, 0]  # nothing ran from HBM, and no earlier call's numbers


REFUSED = {'raised': True, 'code': sh.ST_ERR_ARG, 'resident': True, 'materialize': True}


def _owner_kept(children, rec):
    one = children['']['forms']
    assert rec['owner'] == {'poison': True, 'reuse': 23, 'archive': one['st_sog_file']}, rec
    assert rec['after'] == one['st_sog_bundle'], rec


def test_an_explicit_group_refuses_resident_columns(children):
    ex = children['']['explicit_group']
    assert ex['first'] == REFUSED, ex
    _owner_kept(children, ex)


def test_a_foreign_context_refuses_resident_columns(children):
    fo = children['']['foreign']
    for call in ('summary', 'sog_bundle', 'sog_bundle_mixed'):
        assert fo[call] == REFUSED, (call, fo)
    _owner_kept(children, fo)
    assert fo['summary_after'] is True
