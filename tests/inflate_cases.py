"""Inputs and helpers shared by tests/test_inflate_cpu.py and tests/test_inflate_gpu.py: the deflate
streams and gzip members on which a chunked parallel INFLATE can go wrong (include/st_abi.h,
"inflating a gzip member on the device"), the streams that must be declined, and the stand-alone
program of st_inflate.h's serial chunked decoder (tests/native/inflate_cpu_check.cpp).  Every stream
is made with Python's zlib (or, for the few that zlib would never write, bit by bit here); the
expected output is always what zlib gives for the same bytes."""
import atexit
import os
import pathlib
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np

import deflate_cases as dc
import splat_hip as sh
from golden_io import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCES = [os.path.join(ROOT, 'tests', 'native', 'inflate_cpu_check.cpp')]
CHUNKS = [256, 1024, 4096, 1 << 30]  # the last: one chunk
STAT_NAMES = ['chunks', 'candidates', 'kept', 'discarded', 'markers', 'stored_blocks', 'fixed_blocks', 'dynamic_blocks']


def deflate(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15, flush=zlib.Z_FINISH):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return c.compress(bytes(data)) + c.flush(flush)


def member(stream, data, flg=0, extra=b''):
    """a gzip member around a raw stream; `extra`: the optional header fields that flg announces"""
    return (b'\x1f\x8b\x08' + bytes([flg]) + b'\0\0\0\0\0\xff' + extra + stream +
            struct.pack('<II', zlib.crc32(data), len(data) & 0xffffffff))


def plane(rng, n):
    return np.clip(rng.normal(128, 6, n), 0, 255).astype(np.uint8).tobytes()


class BitWriter:
    """LSB-first bits; prefix codes go in MSB-first"""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> i) & 1 for i in range(n)]
        return self

    def code(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def inflate_all(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b''
    return out


def cases():
    """{name: (kind, blob, data)}: kind 'raw' = a deflate stream, 'gzip' = a member; built once"""
    if _CASES:
        return _CASES
    c = {}
    p60 = plane(np.random.default_rng(7), 60_000)
    ml1 = deflate(p60, 6, 1)
    c['plane_ml1'] = ('raw', ml1, p60)
    rng = np.random.default_rng(11)
    period = np.frombuffer(plane(rng, 30_000), np.uint8).copy()
    copies = []
    for _ in range(8):
        redraw = rng.random(30_000) < 0.15
        period = np.where(redraw, np.frombuffer(plane(rng, 30_000), np.uint8), period)
        copies.append(period.tobytes())
    chain = b''.join(copies)
    c['chain'] = ('raw', deflate(chain, 9, 1), chain)
    c['huffman_only'] = ('raw', deflate(p60, 6, 3, zlib.Z_HUFFMAN_ONLY), p60)
    c['fixed'] = ('raw', deflate(p60[:50_000], 6, 7, zlib.Z_FIXED), p60[:50_000])
    # real block headers inside stored data
    c['decoy_alone'] = ('raw', deflate(ml1, 0), ml1)
    a, z = p60[:9_000], p60[9_000:20_000]
    c['decoy_between_full'] = ('raw', deflate(a, 6, 1, flush=zlib.Z_FULL_FLUSH) + deflate(ml1, 0, flush=zlib.Z_SYNC_FLUSH) +
                               deflate(z, 6, 1), a + ml1 + z)
    c['decoy_between_sync'] = ('raw', deflate(a, 6, 1, flush=zlib.Z_SYNC_FLUSH) + deflate(ml1, 0, flush=zlib.Z_SYNC_FLUSH) +
                               deflate(z, 6, 1), a + ml1 + z)
    c['level0'] = ('raw', deflate(p60 + p60[:10_000], 0), p60 + p60[:10_000])
    c['empty'] = ('raw', b'\x03\x00', b'')
    for n in (1, 2, 3):
        c[f'bytes_{n}'] = ('raw', deflate(p60[:n]), p60[:n])
    const = bytes([5]) * (1 << 20)
    c['constant_1MiB'] = ('raw', deflate(const), const)
    c['wbits9'] = ('raw', deflate(p60[:20_000], 6, 8, wbits=-9), p60[:20_000])
    # a match of 258 at distance 100 is the first token of a non-final block that follows a sync flush: its
    # source starts in the window before the block and runs on into the block's own bytes
    motif = p60[100:200]
    head = p60[:3_000] + motif * 12
    tail = motif * 3 + p60[20_000:23_000]
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    more = p60[50_000:52_000]
    c['match258_spans'] = ('raw', co.compress(head) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(tail) +
                           co.flush(zlib.Z_SYNC_FLUSH) + co.compress(more) + co.flush(), head + tail + more)
    # the final block starts exactly at byte 8,192: a coded part to a byte boundary, one stored block
    # that fills up to it, the last block
    first = deflate(p60[:6_000], 6, 1, flush=zlib.Z_SYNC_FLUSH)
    fill = 8_192 - len(first) - 5
    assert 0 < fill < 65_536
    filler = p60[30_000:30_000 + fill]
    last = deflate(p60[40_000:40_300])
    c['final_on_boundary'] = ('raw', first + b'\0' + struct.pack('<HH', fill, fill ^ 0xffff) + filler + last,
                              p60[:6_000] + filler + p60[40_000:40_300])
    # members: every optional header field; the host writer's segments; the committed .spz files
    extra = struct.pack('<H', 5) + b'extra' + b'name.spz\0' + b'a comment\0'
    extra += struct.pack('<H', zlib.crc32(member(b'', b'', 30, extra)[:-8]) & 0xffff)  # FHCRC
    c['member_with_fields'] = ('gzip', member(ml1, p60, 4 | 8 | 16 | 2, extra), p60)
    c['member_plain'] = ('gzip', member(ml1, p60), p60)
    raw100 = p60 + p60[:40_000]
    c['spz_deflate_seg20000'] = ('gzip', sh.spz_deflate(raw100, 6, _segment=20_000), raw100)
    g = Golden('readers')
    for case in g.meta['cases']:
        if case['format'] == 'spz' and (case['name'] + '_file') in g:
            blob = g[case['name'] + '_file'].tobytes()
            if blob[:2] == b'\x1f\x8b':
                try:
                    c['fixture_' + case['name']] = ('gzip', blob, zlib.decompress(blob, 31))
                except zlib.error:
                    pass  # a fixture that is corrupt on purpose
    # this project's own writer on tests/deflate_cases.py's inputs
    tmp = tempfile.mkdtemp(prefix='st_inflate_in_')
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)

    for name, data in dc.cases().items():
        c['writer_' + name] = ('raw', dc.native('stream', data, pathlib.Path(tmp))[0], data)
    for name, (kind, blob, data) in c.items():
        got = inflate_all(blob) if kind == 'raw' else zlib.decompress(blob, 31)
        assert got == data, name
    _CASES.update(c)
    return _CASES


_CASES = {}


def declined():
    """{name: (kind, blob, expect)}: every one must come back declined"""
    if _DECLINED:
        return _DECLINED
    c = cases()
    _, ml1, p60 = c['plane_ml1']
    m = c['member_plain'][1]
    d = {}
    for k in range(1, 13):
        d[f'truncated_{k}'] = ('gzip', m[:-k], len(p60))
    d['truncated_mid'] = ('gzip', m[:len(m) // 2], len(p60))
    d['truncated_mid_raw'] = ('raw', ml1[:len(ml1) // 2], len(p60))
    flipped = bytearray(m)
    flipped[len(m) // 3] ^= 0x10
    d['flipped_bit'] = ('gzip', bytes(flipped), len(p60))
    d['wrong_isize'] = ('gzip', m[:-4] + struct.pack('<I', len(p60) + 1), len(p60))
    d['btype3'] = ('raw', BitWriter().put(1, 1).put(3, 2).put(0, 13).bytes(), 1)
    # a fixed block: the literal 'a', then length 3 at distance 2 with one byte of output so far
    far = BitWriter().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7).bytes()
    d['distance_too_far'] = ('raw', far, 4)
    # a dynamic header whose code-length code gives all 19 symbols one bit
    over = BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        over.put(1, 3)
    d['oversubscribed'] = ('raw', over.put(0, 64).bytes(), 4)
    d['two_members'] = ('gzip', m + m, len(p60))
    d['two_members_both'] = ('gzip', m + m, 2 * len(p60))
    d['reserved_flg'] = ('gzip', m[:3] + b'\x20' + m[4:], len(p60))
    for kind, blob in (('raw', ml1), ('gzip', m)):
        d[f'expect_short_{kind}'] = (kind, blob, len(p60) - 1)
        d[f'expect_long_{kind}'] = (kind, blob, len(p60) + 1)
    for name in ('btype3', 'distance_too_far', 'oversubscribed', 'truncated_mid_raw'):
        try:
            inflate_all(d[name][1])
        except (zlib.error, AssertionError):
            continue
        raise AssertionError(name + ': zlib takes it')
    _DECLINED.update(d)
    return _DECLINED


_DECLINED = {}

# ---- the stand-alone program ---------------------------------------------------------------------------
_EXE = {}


def harness(sanitize=False):
    """the program's path, built once per session into a directory of its own (removed at exit)"""
    if sanitize not in _EXE:
        d = tempfile.mkdtemp(prefix='st_inflate_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'inflate_cpu_check')
        flags = ['-O2']
        if sanitize:  # host code only: the program has no kernels
            flags = ['-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host',
                     '-fno-sanitize-recover=undefined', '-fno-gpu-sanitize']
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-std=c++17', *flags, '-o', exe, *SOURCES])
        _EXE[sanitize] = exe
    return _EXE[sanitize]


def run_program(args, sanitize=False):
    r = subprocess.run([harness(sanitize), *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def native(kind, blob, want, expect, chunks, tmp_path, sanitize=False):
    """{chunk: None (declined) | {stat: value}} by the program's inflate_chunked on the host"""
    src, ref = tmp_path / 'in.bin', tmp_path / 'want.bin'
    src.write_bytes(blob)
    ref.write_bytes(want)
    lines = run_program(['inflate' if kind == 'raw' else 'gunzip', src, ref, expect, *chunks], sanitize)
    out = {}
    for line in lines:
        w = line.split()
        if w[0] != 'R':
            continue
        assert w[2] in ('OK', 'DECLINED'), line
        out[int(w[1])] = dict(zip(STAT_NAMES, (int(x) for x in w[3:]))) if w[2] == 'OK' else None
    assert sorted(out) == sorted(set(chunks))
    return out


_NATIVE = {}


def native_cached(name, chunks, tmp_path):
    """the program's statistics for a named case, computed once per session"""
    key = (name, tuple(chunks))
    if key not in _NATIVE:
        kind, blob, data = cases()[name]
        _NATIVE[key] = native(kind, blob, data, len(data), chunks, tmp_path)
    return _NATIVE[key]
