"""The host pieces of the .sog reader (no GPU): the WebP-lossless decoder (st_vp8l_dec.cpp, all of
RFC 9649), the ZIP index (st_zip_index) and meta.json parsing.

  * the decoder reproduces every image of tests/golden/read_sog.* (streams from Pillow's libwebp:
    predictor / cross-colour / subtract-green, colour-indexing with each bundling width, a colour
    cache, 1 x 1, 1 x N, N x 1 and odd sizes), freshly encoded ones where Pillow imports, every
    stream of this library's own encoder (the vp8l_cpu_check emulation, cache sizes 0 / 4 / 7 /
    10) and the reference's SOG textures encoded that way;
  * st_zip_index agrees with Python's zipfile and the oracle's zip_store on the reference's own
    .sog archives (tests/golden/sog_bundle.*);
  * robustness: every prefix truncation and a few hundred seeded single-byte corruptions of one
    small stream and one small archive give an error or a full result, in a stand-alone program
    (tests/native/sog_read_cpu_check.cpp) built with AddressSanitizer + UBSan.
"""
import atexit
import io
import json
import os
import shutil
import subprocess
import tempfile
import zipfile
import zlib

import numpy as np
import pytest

import sog_container as oc
import splat_hip as sh
from golden_io import Golden
from test_sog_container_cpu import _harness as _encoder_harness
from test_sog_container_cpu import _images as _encoder_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = Golden('read_sog')
B = Golden('sog_bundle')


@pytest.mark.parametrize('name', G.meta['images'])
def test_decoder_reproduces_fixture_image(name):
    data, want = G[name + '_webp'].tobytes(), G[name + '_rgba']
    assert sh.webp_info(data) == (want.shape[1], want.shape[0])
    assert np.array_equal(sh.webp_decode_lossless(data), want)


def test_decoder_writes_rows_at_the_stride():
    import ctypes
    data, want = G['odd_webp'].tobytes(), G['odd_rgba']
    h, w, _ = want.shape
    stride = w * 4 + 12
    out = np.full((h, stride), 0xA5, np.uint8)
    sh.check(sh.lib().st_webp_decode_lossless(data, ctypes.c_uint64(len(data)), sh._vp(out), ctypes.c_int32(stride)))
    assert np.array_equal(out[:, :w * 4].reshape(h, w, 4), want)
    assert (out[:, w * 4:] == 0xA5).all()
    rc = sh.lib().st_webp_decode_lossless(data, ctypes.c_uint64(len(data)), sh._vp(out), ctypes.c_int32(w * 4 - 4))
    assert rc == sh.ST_ERR_ARG


def test_decoder_reproduces_fresh_libwebp_streams():
    """every effort level of libwebp picks other transforms and code shapes"""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(77)
    yy, xx = np.meshgrid(np.arange(150), np.arange(211), indexing='ij')
    smooth = np.stack([(xx + yy) % 256, (xx * 3) % 256, (yy * 2 + xx // 4) % 256, 255 - yy % 7], -1)
    smooth = (smooth + rng.integers(0, 2, smooth.shape[:2] + (1,)) * rng.integers(0, 3, smooth.shape)) % 256
    tiles = np.repeat(np.repeat(rng.integers(0, 256, (40, 40, 4)), 7, 0), 7, 1)[:273, :269]
    pal = rng.integers(0, 256, (200, 4))
    images = {'smooth': smooth, 'tiles': tiles, 'noise': rng.integers(0, 256, (64, 64, 4)),
              'palette200': pal[rng.integers(0, 200, (120, 77))], 'palette3': pal[rng.integers(0, 3, (33, 35))]}
    for name, img in images.items():
        img = np.ascontiguousarray(img, np.uint8)
        for method, quality in ((0, 0), (3, 50), (4, 80), (6, 100)):
            b = io.BytesIO()
            Image.fromarray(img, 'RGBA').save(b, 'WEBP', lossless=True, exact=True, method=method, quality=quality)
            assert np.array_equal(sh.webp_decode_lossless(b.getvalue()), img), (name, method, quality)


def _encode_here(img, tmp_path, cache_bits):
    h, w, _ = img.shape
    src, dst = tmp_path / 'in.rgba', tmp_path / 'out.webp'
    np.ascontiguousarray(img, np.uint8).tofile(src)
    subprocess.run([_encoder_harness(), str(src), str(w), str(h), str(dst), str(cache_bits)], capture_output=True,
                   text=True, check=True)
    return dst.read_bytes()


@pytest.mark.parametrize('bits', [0, 4, 7, 10])
def test_decoder_reproduces_own_encoder_streams(bits, tmp_path):
    for kind, img in _encoder_images().items():
        img = img.astype(np.uint8)
        assert np.array_equal(sh.webp_decode_lossless(_encode_here(img, tmp_path, bits)), img), kind


def test_decoder_reproduces_reference_sog_textures(tmp_path):
    g = Golden('sog')
    for f in ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels'):
        img = g['sh1_' + f]
        assert np.array_equal(sh.webp_decode_lossless(_encode_here(img, tmp_path, -1)), img), f


def _riff(chunks):
    body = b'WEBP' + b''.join(cc + len(d).to_bytes(4, 'little') + d + b'\0' * (len(d) & 1) for cc, d in chunks)
    return b'RIFF' + len(body).to_bytes(4, 'little') + body


def test_container_forms():
    data, want = G['noise_webp'].tobytes(), G['noise_rgba']
    size = int.from_bytes(data[16:20], 'little')
    vp8l = data[20:20 + size]
    vp8x = bytes([0x10, 0, 0, 0]) + (want.shape[1] - 1).to_bytes(3, 'little') + (want.shape[0] - 1).to_bytes(3, 'little')
    extended = _riff([(b'VP8X', vp8x), (b'ICCP', b'abc'), (b'VP8L', vp8l), (b'EXIF', b'xy')])
    assert np.array_equal(sh.webp_decode_lossless(extended), want)
    with pytest.raises(sh.StError) as e:
        sh.webp_decode_lossless(_riff([(b'VP8 ', b'\0' * 20)]))
    assert e.value.code == sh.ST_ERR_UNSUPPORTED
    for bad in (b'', b'RIFF', _riff([]), _riff([(b'VP8X', vp8x)]), data[:12] + b'VP8L\xff\xff\xff\x7f' + data[20:],
                data[:20] + b'\x2e' + data[21:], data[:24] + bytes([data[24] | 0xe0]) + data[25:]):
        with pytest.raises(sh.StError) as e:
            sh.webp_decode_lossless(bad)
        assert e.value.code == sh.ST_ERR_ARG


@pytest.mark.parametrize('name', [c['name'] for c in B.meta['cases']])
def test_zip_index_matches_zipfile_and_oracle(name):
    z = B[name + '_zip'].tobytes()
    zf = zipfile.ZipFile(io.BytesIO(z))
    got = sh.zip_index(z)
    assert [e[0] for e in got] == [i.filename for i in zf.infolist()]
    entries = []
    for (nm, off, size, crc), info in zip(got, zf.infolist()):
        data = z[off:off + size]
        assert size == info.file_size and crc == info.CRC == zlib.crc32(data)
        assert data == zf.read(nm)
        entries.append((nm, data))
    # the oracle's writer lays the same entries out at the same offsets
    c = next(c for c in B.meta['cases'] if c['name'] == name)
    assert oc.zip_store(entries, *oc.dos_clock(*c['clock'])) == z
    # an archive with an end-record comment, extra fields and a directory-less layout of Python's
    b = io.BytesIO()
    with zipfile.ZipFile(b, 'w', zipfile.ZIP_STORED) as f:
        f.comment = b'trailing comment'
        for nm, data in entries:
            f.writestr(nm, data)
    z2 = b.getvalue()
    assert [(nm, z2[off:off + size]) for nm, off, size, _ in sh.zip_index(z2)] == entries


def test_zip_index_refuses_what_it_cannot_read():
    b = io.BytesIO()
    with zipfile.ZipFile(b, 'w', zipfile.ZIP_DEFLATED) as f:
        f.writestr('meta.json', '{"a": 1}' * 50)
    with pytest.raises(sh.StError) as e:
        sh.zip_index(b.getvalue())
    assert e.value.code == sh.ST_ERR_UNSUPPORTED
    z = B['b_sh0_zip'].tobytes()
    for bad in (b'', z[:-1], z[:100], b'\0' * 22, z[:-6] + b'\xff\xff\xff\x7f' + z[-2:]):
        with pytest.raises(sh.StError) as e:
            sh.zip_index(bad)
        assert e.value.code == sh.ST_ERR_ARG


def test_sog_read_meta():
    z = B['b_sh1_zip'].tobytes()
    text = zipfile.ZipFile(io.BytesIO(z)).read('meta.json')
    m = json.loads(text)
    meta, count, names = sh.sog_read_meta(text)
    assert count == m['count'] and names == list(sh.SOG_FILES)
    assert meta.sh_bands == 1 and meta.palette_size == m['shN']['count']
    assert sh.sog_meta_json(meta, count) == text  # every number survives the round trip
    meta0, count0, names0 = sh.sog_read_meta(zipfile.ZipFile(io.BytesIO(B['b_sh0_zip'].tobytes())).read('meta.json'))
    assert meta0.sh_bands == 0 and names0 == list(sh.SOG_FILES[:5])
    m['means']['mins'][1] = None  # the writer's text of a non-finite number
    assert np.isnan(sh.sog_read_meta(json.dumps(m))[0].means_min[1])
    for edit, code in ((lambda d: d.update(version=1), sh.ST_ERR_UNSUPPORTED),
                       (lambda d: d['quats'].pop('files'), sh.ST_ERR_ARG),
                       (lambda d: d['shN'].update(files=['a.webp']), sh.ST_ERR_ARG),
                       (lambda d: d['scales'].update(codebook=[0.0] * 255), sh.ST_ERR_ARG),
                       (lambda d: d.update(count=0), sh.ST_ERR_ARG),
                       (lambda d: d['shN'].update(bands=4), sh.ST_ERR_ARG)):
        d = json.loads(text)
        edit(d)
        with pytest.raises(sh.StError) as e:
            sh.sog_read_meta(json.dumps(d))
        assert e.value.code == code


def test_sog_read_layout():
    import ctypes

    def layout(meta, count, sizes):
        wh = (ctypes.c_int32 * 2 * 7)()
        for k, (w, h) in enumerate(sizes):
            wh[k][0], wh[k][1] = w, h
        n, nsh = ctypes.c_uint64(0), ctypes.c_int32(0)
        rc = sh.lib().st_sog_read_layout(ctypes.byref(meta), ctypes.c_uint64(count), wh, ctypes.byref(n), ctypes.byref(nsh))
        return rc, n.value, nsh.value

    def meta(w, h, bands=0, pal=0, cw=0, ch=0):
        m = sh.SogMeta()
        m.width, m.height, m.sh_bands, m.palette_size, m.shn_width, m.shn_height = w, h, bands, pal, cw, ch
        return m

    per = [(8, 4)] * 5
    assert layout(meta(8, 4), 32, per + [(0, 0)] * 2) == (0, 32, 0)
    assert layout(meta(8, 4, 2, 100, 512, 2), 30, per + [(512, 2), (8, 4)]) == (0, 30, 24)
    assert layout(meta(8, 4, 3, 65536, 960, 1024), 1, per + [(960, 1024), (8, 4)]) == (0, 1, 45)
    for m, count, sizes in ((meta(8, 4), 0, per + [(0, 0)] * 2),              # count
                            (meta(8, 4), 33, per + [(0, 0)] * 2),             # fewer texels than count
                            (meta(8, 4), 8, [(8, 4)] * 3 + [(4, 8)] + [(8, 4)] + [(0, 0)] * 2),  # unequal sizes
                            (meta(8, 8), 8, per + [(0, 0)] * 2),              # meta disagrees
                            (meta(8, 4, 4, 10, 960, 1), 8, per + [(960, 1), (8, 4)]),   # bands
                            (meta(8, 4, 1, 0, 192, 1), 8, per + [(192, 1), (8, 4)]),    # palette 0
                            (meta(8, 4, 1, 65537, 192, 2000), 8, per + [(192, 2000), (8, 4)]),
                            (meta(8, 4, 1, 64, 191, 1), 8, per + [(191, 1), (8, 4)]),   # width != 64 C
                            (meta(8, 4, 1, 65, 192, 1), 8, per + [(192, 1), (8, 4)]),   # 64 h < palette
                            (meta(8, 4, 1, 64, 192, 1), 8, per + [(192, 1), (4, 8)])):  # labels size
        assert layout(m, count, sizes)[0] == sh.ST_ERR_ARG


# ---- robustness, in the stand-alone program under ASan + UBSan ---------------------------------
_CHECK = []


def _check_program():
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    if not _CHECK:
        d = tempfile.mkdtemp(prefix='st_sogread_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'sog_read_cpu_check')
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined',
                               '-fno-sanitize-recover=undefined', '-o', exe,
                               os.path.join(ROOT, 'tests', 'native', 'sog_read_cpu_check.cpp'),
                               os.path.join(ROOT, 'splat-transform_amd', 'csrc', 'st_vp8l_dec.cpp')])
        _CHECK.append(exe)
    return _CHECK[0]


def test_check_program_decodes_and_indexes(tmp_path):
    src, dst = tmp_path / 'in.webp', tmp_path / 'out.rgba'
    src.write_bytes(G['smooth_webp'].tobytes())
    r = subprocess.run([_check_program(), 'decode', str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = G['smooth_rgba']
    assert r.stdout.split() == [str(want.shape[1]), str(want.shape[0])]
    assert np.array_equal(np.fromfile(dst, np.uint8), want.ravel())
    z = tmp_path / 'in.zip'
    z.write_bytes(B['b_sh0_zip'].tobytes())
    r = subprocess.run([_check_program(), 'index', str(z)], capture_output=True, text=True, check=True)
    assert [tuple(l.split()) for l in r.stdout.splitlines()] == \
        [(nm, str(off), str(size), str(crc)) for nm, off, size, crc in sh.zip_index(z.read_bytes())]


@pytest.mark.parametrize('image', ['palette16', 'odd'])
def test_truncated_and_corrupt_streams_are_refused_or_decoded(image, tmp_path):
    src = tmp_path / 'in.webp'
    src.write_bytes(G[image + '_webp'].tobytes())
    r = subprocess.run([_check_program(), 'fuzz-webp', str(src), '11', '400'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    ok, accepted, rejected = r.stdout.split()
    assert ok == 'ok' and int(accepted) + int(rejected) == len(src.read_bytes()) + 400
    assert int(rejected) >= len(src.read_bytes()) - 1  # a cut stream never decodes (the last byte may be padding)


def test_truncated_and_corrupt_archives_are_refused_or_indexed(tmp_path):
    # the writer's own layout: sizes in data descriptors and the central directory only
    parts = [('meta.json', b'{"version":2}'), ('means_l.webp', G['1x1_webp'].tobytes())]
    z = sh.zip_store([(nm, d, zlib.crc32(d)) for nm, d in parts], 0x6a2b, 0x58b1)
    assert [(nm, z[off:off + size]) for nm, off, size, _ in sh.zip_index(z)] == parts
    src = tmp_path / 'in.zip'
    src.write_bytes(z)
    r = subprocess.run([_check_program(), 'fuzz-zip', str(src), '5', '400'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    ok, accepted, rejected = r.stdout.split()
    assert ok == 'ok' and int(accepted) + int(rejected) == len(z) + 400
    assert int(rejected) == len(z) + 400 - int(accepted) and int(rejected) >= len(z)  # no cut archive indexes
