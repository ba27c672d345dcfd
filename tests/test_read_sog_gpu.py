"""The .sog reader on the GPU: k_sog_decode (st_dev_sog_decode) and the whole read (st_sog_read,
st_dev_sog_read, read_sog's unbundled and renamed-file routes, read_table) against the numpy
restatement tests/sog_read_ref.py, every column bit for bit on uint32 views.

Shapes: 4 x 4 textures with count 1, 13 and 16 (padding texels, the last thread of a partial
block, a full texture), and 2,048 splats (48 x 44: eight blocks and a part of a ninth) at bands
1 / 2 / 3 with a 2,048-entry palette.  The planted bytes cover what the decode rules branch on.
"""
import io
import json
import zipfile
import zlib

import numpy as np
import pytest

import sog_read_ref as R
from golden_io import Golden, mulberry32

pytestmark = pytest.mark.gpu

TEX = ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')
SENTINEL = -7.25


@pytest.fixture(scope='module')
def ctx():
    import torch

    import splat_hip as sh
    c = sh.Context(0)
    c.bind_torch_stream(torch.device('cuda', 0))
    yield c
    c.close()


def _synthetic(seed, count, w, h, bands, palette, equal_axis=None):
    """random textures with the edge bytes planted: (SogMeta, restatement meta, textures)"""
    import splat_hip as sh
    rng = np.random.default_rng(seed)
    C = R.COEFFS[bands]
    tex = {k: rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for k in TEX[:5]}
    flat = {k: v.reshape(-1, 4) for k, v in tex.items()}  # views
    # means codes 0 and 65535; opacity bytes 0 and 255 (both clamps); all four tags written as the
    # writer does (252 + t) and alpha bytes below 252 on the other texels
    flat['means_l'][0, 0] = flat['means_u'][0, 0] = 0
    flat['means_l'][0, 1] = flat['means_u'][0, 1] = 255
    flat['sh0'][0, 3] = 0
    flat['quats'][0] = (128, 128, 128, 252)  # c = (~0, ~0, ~0): the largest m
    if count > 1:
        flat['sh0'][1, 3] = 255
        flat['quats'][1] = (0, 0, 255, 253)  # 1 - sum c^2 < 0: the max(0, .) clamp
        flat['means_l'][count - 1, 2] = flat['means_u'][count - 1, 2] = 255
    for i in range(2, min(count, 10)):
        flat['quats'][i, 3] = 252 + i % 4
    if count >= 16:
        flat['quats'][10:16, 3] = (0, 1, 2, 3, 130, 251)
    if count >= 256:  # every codebook entry
        for k in range(3):
            flat['scales'][:256, k] = np.roll(np.arange(256), 17 * k)
            flat['sh0'][:256, k] = np.roll(np.arange(256), 31 * k + 5)
    meta = sh.SogMeta()
    meta.width, meta.height, meta.sh_bands, meta.palette_size = w, h, bands, palette if bands else 0
    mins, maxs = rng.normal(-3, 0.5, 3), rng.normal(3, 0.5, 3)
    if equal_axis is not None:
        maxs[equal_axis] = mins[equal_axis]
    for a in range(3):
        meta.means_min[a], meta.means_max[a] = mins[a], maxs[a]
    # codebooks: sorted float32 values, with a -0, a subnormal and large magnitudes among them
    for name in ('scales_codebook', 'sh0_codebook', 'shn_codebook'):
        cb = np.sort(rng.normal(0, 2, 256)).astype(np.float32)
        cb[100], cb[101], cb[0], cb[255] = -0.0, 1e-42, -3e38, 3e38
        getattr(meta, name)[:] = cb.tolist()
    if bands:
        rows = (palette + 63) // 64
        meta.shn_width, meta.shn_height = 64 * C, rows
        tex['shN_centroids'] = rng.integers(0, 256, (rows, 64 * C, 4), dtype=np.uint8)
        if palette >= 256:
            tex['shN_centroids'].reshape(-1, 4)[:256, :3] = np.arange(256)[:, None]  # every shN codebook entry
        labels = rng.integers(0, palette, w * h)
        plant = [v for v in (63, 64, 255, 256, palette - 1, 0) if v < palette]
        labels[2:2 + len(plant)] = plant
        lab = np.zeros((h * w, 4), np.uint8)
        lab[:, 0], lab[:, 1], lab[:, 2], lab[:, 3] = labels & 255, labels >> 8, rng.integers(0, 256, w * h), 255
        tex['shN_labels'] = lab.reshape(h, w, 4)
    return meta, R.meta_of_struct(meta), tex


def _decode_on_device(ctx, meta, count, tex, capacity):
    import torch

    import splat_hip as sh
    dev = torch.device('cuda', 0)
    dtex = {k: torch.from_numpy(v.reshape(-1).copy()).to(dev) for k, v in tex.items()}
    nsh = 3 * R.COEFFS[meta.sh_bands]
    out = {k: torch.full((capacity,), SENTINEL, dtype=torch.float32, device=dev) for k in sh.reader_columns(nsh)}
    err = None
    try:
        ctx.dev_sog_decode(meta, count, dtex, out)
    except sh.StError as e:
        err = e
    return {k: v.cpu().numpy() for k, v in out.items()}, err


def _assert_columns(got, want, count=None):
    assert list(got) == list(want)
    for k in want:
        g = got[k] if count is None else got[k][:count]
        assert R.bits_equal(g, want[k]), k


@pytest.mark.parametrize('count,bands,palette,equal_axis', [(1, 0, 0, None), (16, 0, 0, 1), (13, 0, 0, None),
                                                            (13, 2, 5, None)],
                         ids=['one', 'full', 'partial', 'partial-sh2-palette5'])
def test_decode_small_textures(ctx, count, bands, palette, equal_axis):
    meta, rmeta, tex = _synthetic(100 + count + bands, count, 4, 4, bands, palette, equal_axis)
    want, bad = R.decode(rmeta, count, tex)
    assert bad == 0
    got, err = _decode_on_device(ctx, meta, count, tex, 16)
    assert err is None
    _assert_columns(got, want, count)
    for k, v in got.items():  # rows past count are not written
        assert (v[count:] == np.float32(SENTINEL)).all(), k
    if equal_axis is not None:  # mins == maxs: every code decodes to the one value
        assert len(set(got['xyz'[equal_axis]][:count].view(np.uint32).tolist())) == 1


@pytest.mark.parametrize('bands', [1, 2, 3])
def test_decode_2048_splats_with_palette(ctx, bands):
    count, w, h, palette = 2048, 48, 44, 2048
    meta, rmeta, tex = _synthetic(7 + bands, count, w, h, bands, palette)
    labels = tex['shN_labels'].reshape(-1, 4)[:count].astype(np.int64)
    labels = labels[:, 0] | (labels[:, 1] << 8)
    assert {63, 64, 255, 256, palette - 1} <= set(labels.tolist())
    assert set(tex['scales'].reshape(-1, 4)[:count, 0].tolist()) == set(range(256))
    assert {0, 1, 2, 3} <= set((tex['quats'].reshape(-1, 4)[:count, 3] & 3).tolist())
    assert (tex['quats'].reshape(-1, 4)[:count, 3] < 252).any()
    want, bad = R.decode(rmeta, count, tex)
    assert bad == 0 and len(want) == 14 + 3 * R.COEFFS[bands]
    got, err = _decode_on_device(ctx, meta, count, tex, w * h)
    assert err is None
    _assert_columns(got, want, count)
    for k, v in got.items():
        assert (v[count:] == np.float32(SENTINEL)).all(), k


def test_nonfinite_extents_propagate(ctx):
    """maxs = +Inf: code 0 gives mins + Inf * 0 = NaN, every other code +Inf; mins = NaN (a JSON null):
    NaN throughout; the finite axis is untouched.  NaN rows are compared as NaN (the payload is the
    platform's), everything else bit for bit"""
    count = 16
    meta, _, tex = _synthetic(91, count, 4, 4, 0, 0)
    meta.means_max[0] = float('inf')
    meta.means_min[1] = float('nan')
    rmeta = R.meta_of_struct(meta)
    want, _ = R.decode(rmeta, count, tex)
    got, err = _decode_on_device(ctx, meta, count, tex, 16)
    assert err is None
    assert np.isnan(want['x'][0]) and np.isposinf(want['x'][1:]).all() and np.isnan(want['y']).all()
    for k in want:
        nan = np.isnan(want[k])
        assert np.array_equal(np.isnan(got[k][:count]), nan), k
        assert R.bits_equal(got[k][:count][~nan], want[k][~nan]), k


def test_labels_outside_the_palette_are_counted(ctx):
    import splat_hip as sh
    count, palette = 16, 10
    meta, rmeta, tex = _synthetic(55, count, 4, 4, 1, palette)
    lab = tex['shN_labels'].reshape(-1, 4)
    lab[3, :2] = (palette, 0)      # the first label past the palette
    lab[7, :2] = (255, 255)        # 65535
    lab[15, :2] = (0, 1)           # 256
    want, bad = R.decode(rmeta, count, tex)
    assert bad == 3
    got, err = _decode_on_device(ctx, meta, count, tex, 16)
    assert err is not None and err.code == sh.ST_ERR_ARG
    assert '3 shN labels outside the palette' in str(err)
    _assert_columns(got, want, count)  # the columns are complete: zeros on those rows
    for i in (3, 7, 15):
        assert all(got[f'f_rest_{k}'][i] == 0 for k in range(9))


# ---- whole files -------------------------------------------------------------------------------
def _golden_case(name):
    import splat_hip as sh
    g = Golden('sog')
    c = next(c for c in g.meta['cases'] if c['name'] == name)
    tex = {k: g[f'{name}_{k}'] for k in TEX if f'{name}_{k}' in g}
    meta, count, names = sh.sog_read_meta(json.dumps(c['meta']))
    meta.height, meta.width = tex['means_l'].shape[:2]
    if 'shN_centroids' in tex:
        meta.shn_height, meta.shn_width = tex['shN_centroids'].shape[:2]
    cols = {k: g[f'{name}_in_{k}'] for k in g.meta[f'{name}_in_columns']}
    return c, meta, count, tex, cols


@pytest.mark.parametrize('name', ['sh0', 'sh1', 'sh2', 'sh3'])
def test_read_sog_of_reference_textures(ctx, name, tmp_path):
    """the reference's own textures, bundled on the device (dev_sog_bundle encodes them), read back
    whole: host and device columns equal the restatement, and the positions land within one
    quantisation step of the writer's inputs"""
    import torch

    import oracle
    c, meta, count, tex, cols = _golden_case(name)
    dev = torch.device('cuda', 0)
    dtex = {k: torch.from_numpy(v.reshape(-1).copy()).to(dev) for k, v in tex.items()}
    path = tmp_path / (name + '.sog')
    path.write_bytes(ctx.dev_sog_bundle(meta, count, dtex, 0x6a2b, 0x58b1))
    want, bad = R.decode(R.meta_of_json(c['meta']), count, tex)
    assert bad == 0
    got = ctx.read_sog(str(path))
    _assert_columns(got, want)
    got_dev = ctx.read_sog_dev(str(path))
    _assert_columns({k: v.cpu().numpy() for k, v in got_dev.items()}, want)
    # the writer truncates 65535 * (lt(x) - min) / (max - min), so a code's value is at most one step
    # (max - min) / 65535 below lt(x); the reader's f32 store of x moves ln(|x| + 1) by at most 2^-24
    order = oracle.morton_order(cols['x'], cols['y'], cols['z'])
    lt = lambda v: np.sign(v) * np.log(np.abs(v) + 1.0)
    for a, axis in enumerate('xyz'):
        mn, mx = c['meta']['means']['mins'][a], c['meta']['means']['maxs'][a]
        d = np.abs(lt(got[axis].astype(np.float64)) - lt(cols[axis][order].astype(np.float64)))
        assert d.max() <= (mx - mn) / 65535 + 2.0 ** -23, (axis, d.max())


def test_write_read_write_chain(ctx, tmp_path):
    """in.ply -> out.sog (the CLI's path) -> read_table -> out.ply: the PLY's columns are the
    restatement of the archive's own textures"""
    import splat_hip as sh
    b = Golden('sog_bundle')
    c = next(c for c in b.meta['cases'] if c['name'] == 'b_sh1')
    cols = b.table('b_sh1_in_')
    src, sog, dst = tmp_path / 'in.ply', tmp_path / 'out.sog', tmp_path / 'out.ply'
    ctx.ply_file(cols, [], str(src))
    archive, used = ctx.ply_sog_bundle(str(src), [], c['iters'], mulberry32(c['seed'], c['draws'] + 64), 0x6a2b, 0x58b1)
    sog.write_bytes(archive)
    zf = zipfile.ZipFile(io.BytesIO(archive))
    meta_json = json.loads(zf.read('meta.json'))
    tex = {k: sh.webp_decode_lossless(zf.read(k + '.webp')) for k in TEX}
    want, bad = R.decode(R.meta_of_json(meta_json), meta_json['count'], tex)
    assert bad == 0 and meta_json['count'] == c['n']
    table = ctx.read_table(str(sog))
    _assert_columns(table, want)
    rows, _ = ctx.ply_file(table, [], str(dst))
    assert rows == c['n']
    _, elements = ctx.read_ply(str(dst))
    assert [nm for nm, _ in elements] == ['vertex']
    _assert_columns(elements[0][1], want)


def test_unbundled_and_renamed_files(ctx, tmp_path):
    """a meta.json directory (the unbundled form), and a bundle whose files carry other names than
    the writer's: both go through the names meta.json gives"""
    import splat_hip as sh
    c, meta, count, tex, _ = _golden_case('sh2')
    want, _ = R.decode(R.meta_of_json(c['meta']), count, tex)
    m = json.loads(json.dumps(c['meta']))
    renamed = {'means_l': 'a.webp', 'means_u': 'b.webp', 'quats': 'q.webp', 'scales': 's.webp', 'sh0': 'c.webp',
               'shN_centroids': 'pal.webp', 'shN_labels': 'lab.webp'}
    m['means']['files'] = [renamed['means_l'], renamed['means_u']]
    m['quats']['files'], m['scales']['files'], m['sh0']['files'] = [renamed['quats']], [renamed['scales']], [renamed['sh0']]
    m['shN']['files'] = [renamed['shN_centroids'], renamed['shN_labels']]
    files = {renamed[k]: ctx.webp_lossless(v) for k, v in tex.items()}
    d = tmp_path / 'scene'
    d.mkdir()
    for nm, data in files.items():
        (d / nm).write_bytes(data)
    (d / 'meta.json').write_text(json.dumps(m))
    _assert_columns(ctx.read_sog(str(d / 'meta.json')), want)
    _assert_columns(ctx.read_table(str(d / 'meta.json')), want)
    entries = [(nm, data, zlib.crc32(data)) for nm, data in files.items()]
    entries.append(('meta.json', json.dumps(m).encode(), zlib.crc32(json.dumps(m).encode())))
    (tmp_path / 'renamed.sog').write_bytes(sh.zip_store(entries, 0, 0))
    got = ctx.read_sog_dev(str(tmp_path / 'renamed.sog'))
    _assert_columns({k: v.cpu().numpy() for k, v in got.items()}, want)
    # a name meta.json gives and the archive lacks
    (tmp_path / 'short.sog').write_bytes(sh.zip_store(entries[1:], 0, 0))
    with pytest.raises(sh.StError) as e:
        ctx.read_sog(str(tmp_path / 'short.sog'))
    assert e.value.code == sh.ST_ERR_ARG and 'a.webp' in str(e.value)
