"""The DEFLATE encoder of include/st_abi.h ("the gzip member around a .spz image") without a GPU:
st_deflate.h's serial encoder in a stand-alone program (tests/native/deflate_cpu_check.cpp, also
built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly) against zlib -- the
stream inflates to the input with nothing unused, the member passes gzip (CRC-32 and ISIZE), the
size keeps to the bound --, the token rule against its restatement, the block choice on bytes that
do not compress, the 15-bit limit, and the code builder called directly.  The device must give
these bytes (tests/test_deflate_gpu.py)."""
import gzip
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import splat_hip as sh

CASES = sorted(dc.cases())


def inflate(stream):
    d = zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b'' and d.unconsumed_tail == b''
    return out


def test_bounds():
    assert sh.deflate_bound(0) == 2 and sh.gzip_bound(0) == 20
    assert sh.deflate_bound(1) == 6 and sh.deflate_bound(65_535) == 65_540
    # a full segment is two stored blocks
    assert sh.deflate_bound(dc.SEG) == dc.SEG + 5 * -(-dc.SEG // 65_535)
    assert sh.deflate_bound(2 * dc.SEG + 1) == 2 * sh.deflate_bound(dc.SEG) + 6
    assert sh.gzip_bound(12_345) == sh.deflate_bound(12_345) + 18


@pytest.mark.parametrize('name', CASES)
def test_stream_inflates_to_the_input(name, tmp_path):
    data = dc.cases()[name]
    stream, lines = dc.native('stream', data, tmp_path, sanitize=True)
    n, size, bound = (int(x) for x in lines[0].split()[1:4])
    assert (n, size) == (len(data), len(stream)) and bound == sh.deflate_bound(n) and size <= bound
    assert inflate(stream) == data
    assert len(lines) - 1 == -(-n // dc.SEG)
    member, _ = dc.native('gzip', data, tmp_path, sanitize=True)
    assert member[:10] == bytes.fromhex('1f8b08000000000000ff') and member[10:-8] == stream
    assert gzip.decompress(member) == data
    assert member[-8:] == (zlib.crc32(data)).to_bytes(4, 'little') + (n & 0xffffffff).to_bytes(4, 'little')
    # the optimised build gives the same bytes
    assert dc.native('stream', data, tmp_path)[0] == stream
    if n == 0:
        assert stream == b'\x03\x00'


@pytest.mark.parametrize('name', [k for k in CASES if k.startswith('run_') or k in
                                  ('every_run_length', 'one_byte', 'bytes_259', 'bytes_%d' % (dc.SEG + 1))])
def test_tokens_follow_the_rule(name, tmp_path):
    data = dc.cases()[name]
    src = tmp_path / 'in.bin'
    src.write_bytes(data)
    r = subprocess.run([dc.harness(True), 'tokens', str(src)], capture_output=True, text=True, check=True)
    got, seg = [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == 'E':
            got.append(seg)
            seg = []
        else:
            seg.append((w[0], int(w[1])))
    assert got == dc.tokens(data)


def test_a_run_is_cut_at_the_segment_boundary():
    """on the restatement only: that this input exercises the cut (the encoder's tokens are compared
    with the restatement's on this input in test_tokens_follow_the_rule)"""
    toks = dc.tokens(dc.cases()['run_across_segments'])
    assert toks[0][-2:] == [('L', 200), ('M', 99)]  # 100 bytes of the run before the boundary
    assert toks[1][:2] == [('L', 200), ('M', 199)]  # the segment's first byte is a literal


def test_every_length_code_and_extra_bit_class_is_used():
    """on the restatement only: that this input holds every match length (the encoder's tokens are
    compared with the restatement's on this input in test_tokens_follow_the_rule)"""
    lengths = {t[1] for seg in dc.tokens(dc.cases()['every_run_length']) for t in seg if t[0] == 'M'}
    assert lengths == set(range(3, 259))


@pytest.mark.parametrize('name', [k for k in CASES if k.startswith(('highest_symbol_', 'longest_run_'))] +
                         ['bell_with_run_250'])
def test_dynamic_block_with_every_highest_length_symbol(name, tmp_path):
    """the literal/length code is built from its HLIT lengths alone: a dynamic block whose highest
    used length symbol is 284 (HLIT 28) once took the first distance length into its canonical
    codes and did not inflate"""
    data = dc.cases()[name]
    matches = [t[1] for t in dc.tokens(data)[0] if t[0] == 'M']
    highest = max(dc.length_symbol(m) for m in matches)
    if name.startswith('highest_symbol_'):
        assert len(matches) == 1 and highest == int(name.rsplit('_', 1)[1])
    elif name.startswith('longest_run_'):
        L = int(name.rsplit('_', 1)[1])
        assert highest == (284 if L in dc.HIGHEST_284 else 283)
    else:
        assert highest == 284
    stream, lines = dc.native('stream', data, tmp_path, sanitize=True)
    assert lines[1].split()[2] == '2'  # the first segment is a dynamic block
    assert stream[0] & 6 == 4
    assert ((stream[0] >> 3) | (stream[1] << 5)) & 31 == highest + 1 - 257  # HLIT
    assert inflate(stream) == data


@pytest.mark.parametrize('name', dc.STORED_CASES)
def test_bytes_that_do_not_compress_are_stored(name, tmp_path):
    data = dc.cases()[name]
    stream, lines = dc.native('stream', data, tmp_path)
    assert stream[0] & 6 == 0  # BTYPE = 00 in the first byte
    assert all(l.split()[2] == '0' for l in lines[1:])
    assert len(stream) == sh.deflate_bound(len(data))
    if name == 'spz_v2_d3_n300':
        assert (len(data), len(stream)) == (16 + 300 * 64, 16 + 300 * 64 + 5)


def test_fibonacci_counts_meet_the_15_bit_limit(tmp_path):
    data = dc.cases()['fibonacci']
    assert len(data) == sum(dc.FIBONACCI) == 17_710
    stream, lines = dc.native('stream', data, tmp_path)
    _, _, btype, _, free_depth, longest = lines[1].split()
    assert btype == '2' and int(free_depth) > 15 >= int(longest)
    assert inflate(stream) == data


def test_a_constant_buffer_is_runs_of_258(tmp_path):
    """at most 254 matches per 64 KiB and at most 13 bits each under the fixed code, about 3.3 kbit
    against the 8 kbit that n / 64 allows a segment"""
    data = dc.cases()['constant_1MiB']
    stream, _ = dc.native('stream', data, tmp_path)
    print('constant 1 MiB:', len(stream), 'bytes')
    assert len(stream) <= len(data) // 64


def test_coded_size_beside_zlib(tmp_path):
    """recorded, not gated here (the gate is the device test's): the serial encoder's stream
    beside zlib's on the size gate's two images, cut to 16,000 rows"""
    for zero_rows in (False, True):
        raw = dc.size_image(zero_rows, 16_000)
        stream, _ = dc.native('stream', raw, tmp_path)
        print('zero_rows', zero_rows, 'raw', len(raw), 'stream', len(stream), 'zlib 6', len(zlib.compress(raw, 6)),
              'zlib 1', len(zlib.compress(raw, 1)))
        assert inflate(stream) == raw


# ---- the code builder called directly -------------------------------------------------------------------
def build_code(limit, counts):
    r = subprocess.run([dc.harness(True), 'code', str(limit)] + [str(c) for c in counts], capture_output=True,
                       text=True, check=True)
    lens, cost = r.stdout.splitlines()
    lens = [int(x) for x in lens.split()[1:]]
    ours, vp8l, depth = (int(x) for x in cost.split()[1:])
    assert ours == sum(c * l for c, l in zip(counts, lens))
    return lens, ours, vp8l, depth


def kraft(lens):
    return sum(2 ** (32 - l) for l in lens if l)  # in units of 2^-32


CODE_CASES = {
    'two_used': (15, [0, 5, 0, 0, 9]),
    'all_equal_286': (15, [3] * 286),
    'all_equal_19': (7, [1] * 19),
    'fibonacci_lit': (15, [1] + dc.FIBONACCI),
    'powers_cl': (7, [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 0, 0, 0, 0, 3, 0, 5]),  # depth 13 unlimited
    'fibonacci_cl': (7, dc.FIBONACCI[:19]),
    'sparse': (15, [0] * 100 + [7, 0, 0, 1, 65_000, 2] + [0] * 150 + [1]),
}


@pytest.mark.parametrize('name', sorted(CODE_CASES))
def test_code_builder(name):
    limit, counts = CODE_CASES[name]
    lens, ours, vp8l, depth = build_code(limit, counts)
    print(name, 'coded bits', ours, "vp8l::huffman_lengths'", vp8l, 'unlimited depth', depth)
    assert kraft(lens) == 2 ** 32
    assert max(lens) <= limit
    assert all((l == 0) == (c == 0) for c, l in zip(counts, lens))
    if name in ('fibonacci_lit', 'powers_cl', 'fibonacci_cl'):
        assert depth > limit


@pytest.mark.parametrize('used', [0, 3])
def test_code_builder_one_used_symbol(used):
    """one used symbol: it and the lowest other symbol get length 1 (zlib's way round a one-symbol
    code) -- the one unused symbol whose length is not 0; the code is complete"""
    counts = [0] * 6
    counts[used] = 11
    lens, _, _, _ = build_code(15, counts)
    partner = 1 if used == 0 else 0
    assert lens[used] == 1 and lens[partner] == 1 and kraft(lens) == 2 ** 32
    assert all(l == 0 for i, l in enumerate(lens) if i not in (used, partner))
