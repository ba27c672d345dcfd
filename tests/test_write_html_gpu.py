"""The HTML viewer writer on the GPU: k_base64 alone (st_dev_base64) against base64.b64encode, and the
file-streaming forms (st_html_file / st_ply_html_file) against the reference's own writeHtml files
(tests/golden/write_html.*) and the Python restatement pinned to them (tests/write_html_ref.py).
Every byte equal."""
import base64
import os
import random

import numpy as np
import pytest
import torch

import splat_hip as sh
import write_html_ref as ref
from test_ply_gpu import _gs_file
from test_write_html_cpu import CASES, case_columns, case_file, case_template, case_view

pytestmark = pytest.mark.gpu

B64_SPAN = 256 * 12   # the stream bytes one workgroup of k_base64 takes: 12 per lane
S = B64_SPAN
GUARD = 64


@pytest.fixture(scope='module')
def ctx():
    c = sh.Context(0)
    c.bind_torch_stream(0)  # the tests' torch fills and copies are ordered with the library's kernels
    yield c
    c.close()


def dev_segment(data, shift):
    """the bytes in HBM with their first at an address that is `shift` modulo 4: a uint8 tensor view"""
    buf = torch.zeros(len(data) + 8, dtype=torch.uint8, device='cuda')
    at = (shift - buf.data_ptr()) % 4
    seg = buf[at:at + len(data)]
    if len(data):
        seg.copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        assert seg.data_ptr() % 4 == shift
    return seg


def check_b64(ctx, segs, byte0=0, nbytes=None, shifts=None):
    """dev_base64 into a buffer of exactly the bytes wanted plus a guard tail: the size is exact, the
    text is b64encode's, the tail is untouched"""
    stream = b''.join(segs)
    if nbytes is None:
        nbytes = len(stream) - byte0
    want = base64.b64encode(stream[byte0:byte0 + nbytes])
    assert len(want) == sh.base64_size(nbytes)
    dev = [dev_segment(s, (shifts[i] if shifts else 0)) for i, s in enumerate(segs)]
    out = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    size = ctx.dev_base64(dev, out[:len(want)], byte0, nbytes)
    got = out.cpu().numpy()
    assert size == len(want), (size, len(want))
    assert got[:size].tobytes() == want, ([len(s) for s in segs], shifts, byte0, nbytes)
    assert (got[size:] == 0xA5).all(), ([len(s) for s in segs], shifts, byte0, nbytes)


def rand_bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- the kernel alone --------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2, 3])
def test_one_segment_every_short_length(ctx, shift):
    rng = np.random.default_rng(shift)
    for n in range(65):
        check_b64(ctx, [rand_bytes(rng, n)], shifts=[shift])


def test_the_alphabet(ctx):
    alphabet = b'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/'
    raw = base64.b64decode(alphabet)
    assert len(raw) == 48 and base64.b64encode(raw) == alphabet
    check_b64(ctx, [raw])
    check_b64(ctx, [raw[:7], raw[7:8], b'', raw[8:]], shifts=[1, 2, 3, 1])


@pytest.mark.parametrize('n', [S - 1, S, S + 1, 2 * S + 1])
def test_workgroup_span_edges(ctx, n):
    rng = np.random.default_rng(n)
    for shift in range(4):
        check_b64(ctx, [rand_bytes(rng, n)], shifts=[shift])


SEG_LENS = [0, 1, 2, 3, 4, 5, 7, 11, 12, 13, S - 1, S + 1]


def test_four_segments(ctx):
    """lengths around a lane's 12 bytes and the workgroup's span, every source alignment: a lane that
    crosses three boundaries (1, 1, 1, 1), an empty segment inside a lane (5, 0, 2, 4)"""
    rng = np.random.default_rng(4)
    py = random.Random(4)
    combos = [(1, 1, 1, 1), (5, 0, 2, 4), (0, 0, 0, 0), (0, 0, 0, 1), (13, 0, 0, 13), (S - 1, 1, S + 1, 2),
              (S + 1, S + 1, S - 1, S - 1), (3, S - 1, 0, 12), (11, 11, 11, 11), (12, 12, 12, 12)]
    combos += [tuple(py.choice(SEG_LENS) for _ in range(4)) for _ in range(120)]
    for lens in combos:
        check_b64(ctx, [rand_bytes(rng, n) for n in lens], shifts=[py.randrange(4) for _ in range(4)])


@pytest.mark.parametrize('head', range(12))
def test_header_length_in_front_of_a_segment(ctx, head):
    """every header length modulo 12 (the lane's bytes) and so modulo 4 and 3 in front of 4 KiB"""
    rng = np.random.default_rng(head)
    for base in (0, 12 * 21):
        check_b64(ctx, [rand_bytes(rng, base + head), rand_bytes(rng, 4096)], shifts=[head % 4, (head + 1) % 4])
        check_b64(ctx, [rand_bytes(rng, base + head), rand_bytes(rng, 4096), b'', rand_bytes(rng, 5)], shifts=[0, 0, 0, 3])


def test_fewer_segments(ctx):
    rng = np.random.default_rng(7)
    check_b64(ctx, [])
    check_b64(ctx, [rand_bytes(rng, 100), rand_bytes(rng, 101)], shifts=[3, 2])
    check_b64(ctx, [rand_bytes(rng, 10), rand_bytes(rng, S), rand_bytes(rng, 1)], shifts=[1, 1, 1])


def test_ranges(ctx):
    rng = np.random.default_rng(8)
    segs = [rand_bytes(rng, 1000), rand_bytes(rng, 2 * S + 50), rand_bytes(rng, 7), rand_bytes(rng, 300)]
    total = sum(map(len, segs))
    assert total % 3 != 0
    for byte0 in (1002, 1000 + S - 1, 3 * ((1000 + 2 * S) // 3)):   # inside the second segment
        assert byte0 % 3 == 0 and 1000 < byte0 < 1000 + len(segs[1])
        check_b64(ctx, segs, byte0)                                 # to the stream's end: padded
        for nbytes in (0, 3, 12, 15, S, S + 3, 3 * ((total - byte0) // 3)):
            if nbytes > total - byte0:
                continue
            check_b64(ctx, segs, byte0, nbytes, shifts=[1, 3, 2, 0])
    # the pieces of a stream, as the file form cuts it, are the whole text
    piece = S + 3 * 5
    text = b''
    dev = [dev_segment(s, i) for i, s in enumerate(segs)]
    for b in range(0, total, piece):
        nb = min(piece, total - b)
        out = torch.zeros(sh.base64_size(nb), dtype=torch.uint8, device='cuda')
        assert ctx.dev_base64(dev, out, b, nb) == out.numel()
        text += out.cpu().numpy().tobytes()
    assert text == base64.b64encode(b''.join(segs))


def refused(ctx, dev, out, byte0, nbytes):
    before = out.clone()
    with pytest.raises(sh.StError) as e:
        ctx.dev_base64(dev, out, byte0, nbytes)
    assert e.value.code == sh.ST_ERR_ARG
    assert torch.equal(out, before)


def test_refused_calls_write_nothing(ctx):
    rng = np.random.default_rng(9)
    segs = [rand_bytes(rng, 100), rand_bytes(rng, 200)]
    dev = [dev_segment(s, 0) for s in segs]
    buf = torch.full((1024,), 0xA5, dtype=torch.uint8, device='cuda')
    refused(ctx, dev, buf, 102, 10)       # a partial last group before the stream's end
    refused(ctx, dev, buf, 102, 199)      # past the stream's end
    refused(ctx, dev, buf, 100, 30)       # byte0 no multiple of 3
    refused(ctx, dev, buf, 303, 0)        # byte0 past the stream's end
    need = sh.base64_size(300)
    refused(ctx, dev, buf[:need - 1], 0, 300)     # one byte short of the text
    refused(ctx, dev, buf[1:1 + need], 0, 300)    # a misaligned output
    assert buf.data_ptr() % 4 == 0
    # the size is still reported
    import ctypes
    arr = (sh.BytesSeg * 2)(*[sh.BytesSeg(d.data_ptr(), d.numel()) for d in dev])
    size = ctypes.c_uint64()
    rc = sh.lib().st_dev_base64(ctx.h, arr, ctypes.c_int32(2), ctypes.c_uint64(0), ctypes.c_uint64(300),
                                ctypes.c_void_p(buf.data_ptr()), ctypes.c_uint64(need - 1), ctypes.byref(size))
    assert rc == sh.ST_ERR_ARG and size.value == need
    assert int(buf.min()) == 0xA5 == int(buf.max())
    assert ctx.dev_base64(dev, buf[:need], 0, 300) == need


def test_one_mebibyte(ctx):
    rng = np.random.default_rng(10)
    data = bytearray(rand_bytes(rng, 1 << 20))
    data[:256] = bytes(range(256))
    assert set(data) == set(range(256))
    check_b64(ctx, [bytes(data)], shifts=[1])
    check_b64(ctx, [bytes(data[:333_333]), bytes(data[333_333:700_001]), bytes(data[700_001:])], shifts=[2, 3, 1])


# ---- the files ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_html_file_matches_reference(ctx, tmp_path, name):
    cam, tgt = case_view(name)
    want = case_file(name)
    p = tmp_path / 'out.html'
    m, C, size = ctx.html_file(case_columns(name), [], case_template(name), str(p), cam, tgt)
    assert (m, C, size) == (len(case_columns(name)[0][1]), 15 if name == 'sh3' else 0, len(want))
    assert p.read_bytes() == want


def test_missing_pattern_leaves_the_page_alone(ctx, tmp_path):
    cam, tgt = case_view('missing')
    page, suffix, embeds = sh.html_parts(*case_template('missing'), cam, tgt)
    assert embeds == 0 and suffix == b''
    p = tmp_path / 'out.html'
    p.write_bytes(b'\x07' * (len(page) + 99))
    m, C, size = ctx.html_file(case_columns('missing'), [], case_template('missing'), str(p), cam, tgt)
    assert (m, size) == (4, len(page)) and p.read_bytes() == page == case_file('missing')
    # the chain still ran: its errors surface
    with pytest.raises(sh.StError) as e:
        ctx.html_file([kv for kv in case_columns('missing') if kv[0] != 'opacity'], [], case_template('missing'),
                      str(p), cam, tgt)
    assert e.value.code == sh.ST_ERR_ARG


@pytest.fixture(scope='module')
def scene(ctx, tmp_path_factory):
    """test_compressed_ply_file_equals_the_arrays' input cut to 30,001 rows: (path, columns, actions)"""
    d = tmp_path_factory.mktemp('html_scene')
    n = 30_001
    data = bytearray(_gs_file(n, 15, 11))
    src = d / 'in.ply'
    src.write_bytes(bytes(data))
    _, els = ctx.read_ply(str(src))
    cols = dict(els)['vertex']
    cols['x'][::997] = np.nan  # rows filterNaN drops
    src.write_bytes(data[:data.index(b'end_header\n') + 11] + np.stack(list(cols.values()), 1).astype('<f4').tobytes())
    acts = [{'kind': 'rotate', 'value': (0, 45, 0)}, {'kind': 'filterNaN'}]
    return str(src), list(cols.items()), acts


@pytest.mark.parametrize('slot_mb', [None, '1'])
def test_html_file_equals_the_compressed_ply_file(ctx, tmp_path, monkeypatch, scene, slot_mb):
    """the page around the base64 of the .compressed.ply file the same tree writes -- into a file that
    held longer content, from a descriptor position inside a file, with 1 MiB slots too (three pieces
    of text through the ring)"""
    if slot_mb:
        monkeypatch.setenv('ST_CPF_SLOT_MB', slot_mb)
    src, cols, acts = scene
    tpl = case_template('plain')
    cam, tgt = (1.5, -2.25, 3), (0, 0.5, -1)
    cply = tmp_path / 'out.compressed.ply'
    m, C, csize = ctx.ply_compressed_ply_file(src, acts, str(cply))
    payload = cply.read_bytes()
    assert C == 15 and m < 30_001 and len(payload) == csize > 1_800_000
    if slot_mb:
        assert -(-sh.base64_size(csize) // (1 << 20)) == 3
    prefix, suffix, embeds = sh.html_parts(*tpl, cam, tgt)
    want = prefix + base64.b64encode(payload) + suffix
    assert embeds == 1 and want == ref.write_html(*tpl, cam, tgt, payload)
    out = tmp_path / 'out.html'
    out.write_bytes(b'\x07' * (len(want) + 12345))
    assert ctx.html_file(cols, acts, tpl, str(out), cam, tgt) == (m, 15, len(want))
    assert out.read_bytes() == want
    # the file's path in: the same bytes
    out2 = tmp_path / 'out2.html'
    assert ctx.ply_html_file(src, acts, tpl, str(out2), cam, tgt) == (m, 15, len(want))
    assert out2.read_bytes() == want
    # from position 37 of a longer file: the output follows the 37 bytes, the file ends with it, and
    # the position is left behind it
    out.write_bytes(b'#' * (len(want) + 5000))
    fd = os.open(str(out), os.O_RDWR)
    try:
        os.lseek(fd, 37, os.SEEK_SET)
        assert ctx.html_file(cols, acts, tpl, fd, cam, tgt) == (m, 15, len(want))
        assert os.lseek(fd, 0, os.SEEK_CUR) == 37 + len(want)
    finally:
        os.close(fd)
    assert out.read_bytes() == b'#' * 37 + want


def test_version_changes_the_payload_only(ctx, tmp_path, scene):
    src, cols, acts = scene
    tpl = case_template('utf8')
    a, b, cply = tmp_path / 'a.html', tmp_path / 'b.html', tmp_path / 'v.compressed.ply'
    ra = ctx.ply_html_file(src, acts, tpl, str(a))
    rb = ctx.ply_html_file(src, acts, tpl, str(b), version='9.9.9')
    ctx.ply_compressed_ply_file(src, acts, str(cply), version='9.9.9')
    prefix, suffix, _ = sh.html_parts(*tpl)
    fa, fb = a.read_bytes(), b.read_bytes()
    assert ra[:2] == rb[:2] and ra[2] == len(fa) and rb[2] == len(fb) and fa != fb
    assert fa.startswith(prefix) and fb.startswith(prefix) and fa.endswith(suffix) and fb.endswith(suffix)
    assert fb[len(prefix):len(fb) - len(suffix)] == base64.b64encode(cply.read_bytes())
    assert b'splat-transform 9.9.9' in base64.b64decode(fb[len(prefix):len(fb) - len(suffix)])[:200]
    assert b'splat-transform 0.10.1' in base64.b64decode(fa[len(prefix):len(fa) - len(suffix)])[:200]


@pytest.mark.parametrize('flags', [os.O_RDONLY, os.O_WRONLY | os.O_APPEND])
def test_html_file_refuses_descriptor(ctx, tmp_path, scene, flags):
    src, cols, acts = scene
    small = [(k, a[:100]) for k, a in cols]
    p = tmp_path / 'keep.html'
    p.write_bytes(b'keep')
    fd = os.open(str(p), flags)
    try:
        with pytest.raises(sh.StError) as e:
            ctx.html_file(small, [], case_template('plain'), fd)
        assert e.value.code == sh.ST_ERR_ARG
        with pytest.raises(sh.StError) as e:
            ctx.ply_html_file(src, [], case_template('plain'), fd)
        assert e.value.code == sh.ST_ERR_ARG
    finally:
        os.close(fd)
    assert p.read_bytes() == b'keep'
