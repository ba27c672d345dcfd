"""The chunked INFLATE of include/st_abi.h ("inflating a gzip member on the device") without a GPU:
st_inflate.h's serial implementation of the chunked method in a stand-alone program
(tests/native/inflate_cpu_check.cpp, also built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly) against zlib on every stream of tests/inflate_cases.py
at chunk sizes 256, 1,024, 4,096 and one chunk; the streams that must be declined; the statistics
that show the chain was really walked; the candidate predicate on every true block start; the gzip
header parse and the serial head.  The device must give these bytes and these statistics
(tests/test_inflate_gpu.py)."""
import ctypes
import zlib

import pytest

import inflate_cases as ic
import splat_hip as sh

CASES = sorted(ic.cases())
DECLINED = sorted(ic.declined())


@pytest.mark.parametrize('name', CASES)
def test_every_chunk_size_gives_zlibs_bytes(name, tmp_path):
    kind, blob, data = ic.cases()[name]
    got = ic.native(kind, blob, data, len(data), ic.CHUNKS, tmp_path, sanitize=True)
    for chunk in ic.CHUNKS:
        st = got[chunk]
        assert st is not None, (name, chunk, 'declined')
        nbytes = len(blob) if kind == 'raw' else None
        if nbytes:
            assert st['chunks'] == max(1, -(-nbytes // chunk))
        assert st['kept'] + st['discarded'] == 1 + st['candidates'] and 1 <= st['kept'] <= st['chunks']
    assert got[1 << 30]['kept'] == 1 and got[1 << 30]['markers'] == 0
    # the optimised build gives the same numbers
    fast = ic.native(kind, blob, data, len(data), [1024, 0, sh.INFLATE_CHUNK], tmp_path)
    assert fast[1024] == got[1024] and fast[0] == fast[sh.INFLATE_CHUNK]  # chunk size 0 is the default


@pytest.mark.parametrize('name', DECLINED)
def test_declined(name, tmp_path):
    kind, blob, expect = ic.declined()[name]
    got = ic.native(kind, blob, b'', expect, ic.CHUNKS, tmp_path, sanitize=True)
    assert got == {c: None for c in ic.CHUNKS}


def test_the_chain_is_walked(tmp_path):
    """the numbers that show parallel decoders, markers and discarded decoders are really there
    (measured with zlib 1.2.11: plane_ml1 280 dynamic blocks, 44 of 45 1 KiB chunks with a start;
    chain 541 dynamic blocks, 105 of 106): a zlib that moves a stream out of these bounds fails here"""
    st = {name: ic.native_cached(name, ic.CHUNKS, tmp_path) for name in
          ('plane_ml1', 'chain', 'huffman_only', 'fixed', 'decoy_alone', 'decoy_between_full', 'decoy_between_sync',
           'match258_spans', 'final_on_boundary', 'level0', 'constant_1MiB')}
    for name in st:
        print(name, st[name][1024])
    for name in ('plane_ml1', 'chain'):
        assert st[name][1024]['kept'] >= 20 and st[name][1024]['markers'] > 1000
        assert st[name][1024]['dynamic_blocks'] >= 100 and st[name][1024]['stored_blocks'] == 0
    assert st['chain'][256]['kept'] >= 100
    assert st['huffman_only'][1024]['markers'] == 0 and st['huffman_only'][1024]['kept'] >= 20
    assert st['huffman_only'][1024]['dynamic_blocks'] >= 50
    for chunk in ic.CHUNKS:
        assert st['fixed'][chunk]['kept'] == 1 and st['fixed'][chunk]['fixed_blocks'] >= 2
        assert st['fixed'][chunk]['dynamic_blocks'] == 0
    for name in ('decoy_alone', 'decoy_between_full', 'decoy_between_sync'):
        assert st[name][1024]['discarded'] >= 1 and st[name][1024]['stored_blocks'] >= 1
    assert st['decoy_alone'][1024]['kept'] == 1
    assert st['match258_spans'][256]['kept'] >= 2 and st['match258_spans'][256]['markers'] >= 258
    assert st['level0'][1024] == dict(chunks=st['level0'][1024]['chunks'], candidates=st['level0'][1024]['candidates'],
                                      kept=1, discarded=st['level0'][1024]['candidates'], markers=0, stored_blocks=2,
                                      fixed_blocks=0, dynamic_blocks=0)
    assert st['constant_1MiB'][256]['kept'] >= 1


def test_the_predicate_accepts_every_true_dynamic_block_start(tmp_path):
    src = tmp_path / 'in.bin'
    starts = 0
    for name in ('plane_ml1', 'chain', 'huffman_only', 'match258_spans'):
        src.write_bytes(ic.cases()[name][1])
        lines = [l.split() for l in ic.run_program(['starts', src], sanitize=True)]
        assert lines[-1] == ['E', str(len(ic.cases()[name][2]))]
        for w in lines[:-1]:
            assert w[0] == 'B'
            final, btype, accepted = int(w[2]), int(w[3]), int(w[4])
            assert accepted == (1 if btype == 2 and not final else 0), (name, w)
            starts += accepted
    assert starts >= 500


def test_final_block_on_a_chunk_boundary(tmp_path):
    src = tmp_path / 'in.bin'
    src.write_bytes(ic.cases()['final_on_boundary'][1])
    lines = [l.split() for l in ic.run_program(['starts', src])]
    final = [w for w in lines if w[0] == 'B' and w[2] == '1']
    assert len(final) == 1 and int(final[0][1]) == 8 * 8192


def test_head(tmp_path):
    src = tmp_path / 'in.bin'
    for name in ('plane_ml1', 'level0', 'fixed', 'constant_1MiB', 'bytes_3', 'empty'):
        _, blob, data = ic.cases()[name]
        src.write_bytes(blob)
        for want in (0, 1, 16, 300):
            line = ic.run_program(['head', src, want], sanitize=True)[0].split()
            got = min(want, len(data))
            assert line[:2] == ['H', str(got)] and bytes.fromhex(line[2] if len(line) > 2 else '') == data[:got]
    src.write_bytes(ic.declined()['btype3'][1])
    assert ic.run_program(['head', src, 16])[0] == 'H BROKEN'
    # through the library: st_inflate_head and st_gzip_member_layout are host calls
    _, blob, data = ic.cases()['member_with_fields']
    off, length, crc, isize = sh.gzip_member_layout(blob)
    assert blob[off:off + length] == ic.cases()['plane_ml1'][1] and (crc, isize) == (zlib.crc32(data), len(data))
    assert sh.inflate_head(blob[off:off + length], 16) == data[:16]
    assert sh.inflate_head(ic.cases()['bytes_3'][1], 16) == ic.cases()['bytes_3'][2]
    assert sh.gzip_member_layout(b'NGSP' + bytes(40)) is None
    assert sh.gzip_member_layout(ic.declined()['reserved_flg'][1]) is None
    assert sh.inflate_head(ic.declined()['btype3'][1], 16) is None
