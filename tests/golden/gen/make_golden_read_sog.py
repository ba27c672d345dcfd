"""Writes tests/golden/read_sog.{json,bin}: WebP-lossless files encoded by Pillow's libwebp
(lossless=True, exact=True) with the RGBA they must decode to, for the host VP8L decoder of the
.sog reader (st_vp8l_dec.cpp).  The test machines need no Pillow to use the fixture.

    python3 tests/golden/gen/make_golden_read_sog.py

The images are seeded; the bytes depend on the libwebp build (recorded in meta), so a rerun with
another build gives other streams of the same pixels.
"""
import io
import json
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.dirname(HERE)


def images():
    rng = np.random.default_rng(9649)
    out = {}
    out['noise'] = rng.integers(0, 256, (37, 53, 4))
    gx, gy = np.meshgrid(np.arange(96), np.arange(70))
    out['gradient'] = np.stack([gx * 3 % 256, gy * 2 % 256, (gx + gy) % 256, np.full_like(gx, 255)], -1)
    # smooth structure with sparse noise: the predictor, cross-colour and subtract-green transforms
    # and backward references pay here
    s = np.zeros((96, 128, 4), np.int64)
    yy, xx = np.meshgrid(np.arange(96), np.arange(128), indexing='ij')
    s[..., 0] = (xx * 2 + yy) % 256
    s[..., 1] = (xx + yy * 2) % 256
    s[..., 2] = (s[..., 0] // 2 + s[..., 1] // 3 + 11) % 256
    s[..., 3] = 255 - (yy // 8) * 3
    s[20:60, 30:100, :3] = (200, 90, 30)
    s = (s + rng.integers(0, 2, s.shape[:2] + (1,)) * rng.integers(0, 4, s.shape)) % 256
    out['smooth'] = s
    # palettes: <= 2, <= 4, <= 16 colours bundle 8, 4, 2 pixels per byte; 60 colours index without
    # bundling and repeat without spatial order (a colour cache pays); widths no multiple of 8
    for k, shape in ((2, (45, 67)), (4, (45, 67)), (16, (45, 67)), (60, (90, 131))):
        pal = rng.integers(0, 256, (k, 4))
        out[f'palette{k}'] = pal[rng.integers(0, k, shape)]
    out['1x1'] = rng.integers(0, 256, (1, 1, 4))
    out['1x77'] = rng.integers(0, 256, (77, 1, 4))
    out['50x1'] = rng.integers(0, 256, (1, 50, 4))
    out['odd'] = np.repeat(rng.integers(0, 256, (19, 27, 4)), 2, axis=0)[:37, :]
    return {k: np.ascontiguousarray(v, np.uint8) for k, v in out.items()}


def main():
    blob = bytearray()
    arrays = {}

    def put(name, a):
        a = np.ascontiguousarray(a, np.uint8)
        arrays[name] = dict(dtype='u1', shape=list(a.shape), offset=len(blob), nbytes=a.nbytes)
        blob.extend(a.tobytes())

    names = []
    for name, rgba in images().items():
        b = io.BytesIO()
        Image.fromarray(rgba, 'RGBA').save(b, 'WEBP', lossless=True, exact=True)
        assert np.array_equal(np.array(Image.open(io.BytesIO(b.getvalue())).convert('RGBA')), rgba), name
        put(name + '_webp', np.frombuffer(b.getvalue(), np.uint8))
        put(name + '_rgba', rgba)
        names.append(name)
    meta = dict(images=names, encoder='Pillow %s, libwebp %s' % (Image.__version__, features.version('webp')))
    with open(os.path.join(OUT, 'read_sog.json'), 'w') as f:
        json.dump(dict(meta=meta, arrays=arrays), f, indent=1)
    with open(os.path.join(OUT, 'read_sog.bin'), 'wb') as f:
        f.write(bytes(blob))
    print(len(blob), 'bytes;', meta['encoder'])


if __name__ == '__main__':
    main()
