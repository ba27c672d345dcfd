"""The PLY writer on the host side (no GPU): the numpy restatement of writePly
(tests/write_ply_ref.py) against the reference's own output files (tests/golden/write_ply.*,
and the two-element mixed-type file of tests/golden/ply_io.*), and the product's header text
(st_ply_header_text / st_ply_element_text) against the same headers, argument errors included.
"""
import ctypes

import numpy as np
import pytest

import ply
import splat_hip as sh
import write_ply_ref as ref
from golden_io import Golden

W = Golden('write_ply')
G = Golden('ply_io')
CASES = list(W.meta)


def case_elements(name):
    """[(element name, [(column, numpy array)], rows)] of a write_ply fixture case"""
    return [(e['name'], [(c['name'], W[f"{name}_{e['name']}_{c['name']}"]) for c in e['columns']], e['rows'])
            for e in W.meta[name]['elements']]


def case_header(name):
    return W[f'{name}_file'][:W.meta[name]['header_bytes']].tobytes()


def test_fixture_covers_the_cases():
    m = W.meta
    assert m['empty']['elements'][0]['rows'] == 0
    assert m['cli']['comments'] == [] and [e['name'] for e in m['cli']['elements']] == ['vertex']
    assert m['sh1']['elements'][0]['rows'] == 300 and len(m['sh1']['elements'][0]['columns']) == 17 + 9
    assert [c['dtype'] for c in m['uds']['elements'][0]['columns']] == ['u1', 'f8', 'i2']
    assert m['uds']['elements'][0]['rows'] == 1025
    assert sorted(c['dtype'] for c in m['types8']['elements'][0]['columns']) == sorted(ref.PLY_NAMES)
    assert m['nocols']['elements'][0]['columns'] == []


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference(name):
    want = W[f'{name}_file'].tobytes()
    assert ref.write_ply(W.meta[name]['comments'], case_elements(name)) == want
    rows = sum(e['rows'] * sum(np.dtype(c['dtype']).itemsize for c in e['columns']) for e in W.meta[name]['elements'])
    assert len(want) == W.meta[name]['header_bytes'] + rows


def test_restatement_round_trips_the_mixed_file():
    comments, els = ply.read_ply(G['mixed_file'].tobytes())
    assert ref.write_ply(comments, [(n, list(c.items())) for n, c in els]) == G['mixed_file'].tobytes()


@pytest.mark.parametrize('name', CASES)
def test_header_text_matches_reference(name):
    m = W.meta[name]
    els = case_elements(name)
    if len(els) == 1:
        el, cols, n = els[0]
        assert sh.ply_header_text(cols, n, el, m['comments']) == case_header(name)
    # the same header composed from the element blocks, as a host of several elements does
    head = b'ply\nformat binary_little_endian 1.0\n' + b''.join(b'comment %s\n' % c.encode() for c in m['comments'])
    for el, cols, n in els:
        head += sh.ply_header_text(cols, n, el, element_only=True)
    assert head + b'end_header\n' == case_header(name)


def test_header_text_of_the_mixed_file():
    h = sh.ply_parse_header(G['mixed_file'].tobytes())
    head = b'ply\nformat binary_little_endian 1.0\n' + b''.join(b'comment %s\n' % c.encode() for c in h.comment_list())
    for name, count, props in h.layout():
        head += sh.ply_header_text(props, count, name, element_only=True)
    assert head + b'end_header\n' == G['mixed_file'][:h.header_bytes].tobytes()


def test_header_text_defaults():
    # element NULL is the CLI's "vertex"; dtypes stand in for arrays; no columns, no comments
    assert sh.ply_header_text([('x', np.float32), ('n', np.uint16)], 7) == \
        b'ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty ushort n\nend_header\n'
    assert sh.ply_header_text([], 3, 'bare') == b'ply\nformat binary_little_endian 1.0\nelement bare 3\nend_header\n'
    assert sh.ply_header_text([], 2 ** 40, element_only=True) == b'element vertex 1099511627776\n'
    assert sh.ply_header_text([('a', t) for t in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32,
                                                  np.float32, np.float64)], 0, element_only=True) == (
        b'element vertex 0\nproperty char a\nproperty uchar a\nproperty short a\nproperty ushort a\nproperty int a\n'
        b'property uint a\nproperty float a\nproperty double a\n')


def _raw_ttable(names, types, n=1):
    cn = (ctypes.c_char_p * len(names))(*[k.encode() for k in names])
    ct = (ctypes.c_int32 * len(types))(*types)
    t = sh.TTable(n, len(names), ctypes.cast(cn, ctypes.POINTER(ctypes.c_char_p)),
                  ctypes.cast(ct, ctypes.POINTER(ctypes.c_int32)), None)
    t._keep = (cn, ct)
    return t


def test_header_text_argument_errors():
    L = sh.lib()
    out, size = ctypes.c_void_p(), ctypes.c_uint64()
    good = _raw_ttable(['x'], [7])
    assert L.st_ply_header_text(ctypes.byref(good), None, None, 0, ctypes.byref(out), ctypes.byref(size)) == sh.ST_OK
    L.st_free(out)
    # NULL output, NULL size, NULL table
    assert L.st_ply_header_text(ctypes.byref(good), None, None, 0, None, ctypes.byref(size)) == sh.ST_ERR_ARG
    assert L.st_ply_header_text(ctypes.byref(good), None, None, 0, ctypes.byref(out), None) == sh.ST_ERR_ARG
    assert L.st_ply_header_text(None, None, None, 0, ctypes.byref(out), ctypes.byref(size)) == sh.ST_ERR_ARG
    assert L.st_ply_element_text(ctypes.byref(good), None, None, ctypes.byref(size)) == sh.ST_ERR_ARG
    # type codes outside ST_PLY_CHAR..ST_PLY_DOUBLE
    for bad in (0, 9, -1):
        t = _raw_ttable(['x', 'y'], [7, bad])
        assert L.st_ply_header_text(ctypes.byref(t), None, None, 0, ctypes.byref(out), ctypes.byref(size)) == \
            sh.ST_ERR_ARG
        assert b'bad column type' in L.st_last_error()
        assert L.st_ply_element_text(ctypes.byref(t), None, ctypes.byref(out), ctypes.byref(size)) == sh.ST_ERR_ARG
    # comments announced but not given
    assert L.st_ply_header_text(ctypes.byref(good), None, None, 2, ctypes.byref(out), ctypes.byref(size)) == \
        sh.ST_ERR_ARG
    assert L.st_ply_header_text(ctypes.byref(good), None, None, -1, ctypes.byref(out), ctypes.byref(size)) == \
        sh.ST_ERR_ARG
