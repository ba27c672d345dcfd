"""The readers' CPU restatement (oracle/readers.py) against the reference's own readers: every
accepted case of tests/golden/readers.* and readers_edges.* goes through it, every column bit-equal
(where they disagree the fixture is right).  And what the readers_edges set is for: computed here
from the fixture files' own headers, so that a regeneration cannot lose it silently.
"""
import gzip
import os

import numpy as np
import pytest

import readers as oracle_readers
import splat_hip as sh
from golden_io import GOLDEN, Golden
from readers_files import ksplat_sections, spz_planes

SETS = {name: Golden(name) for name in ('readers', 'readers_edges')}
CASES = [(s, c['name']) for s, g in SETS.items() for c in g.meta['cases']]
EDGES = SETS['readers_edges']


def case(set_name, name):
    g = SETS[set_name]
    return g, next(c for c in g.meta['cases'] if c['name'] == name)


def restate(fmt, data):
    if fmt == 'splat':
        return oracle_readers.read_splat(data)
    if fmt == 'ksplat':
        return oracle_readers.read_ksplat(data)
    return oracle_readers.read_spz(gzip.decompress(data))


@pytest.mark.parametrize('set_name,name', CASES, ids=[f'{s}-{n}' for s, n in CASES])
def test_restatement_matches_reference(set_name, name):
    g, c = case(set_name, name)
    got, n, nsh = restate(c['format'], g[name + '_file'].tobytes())
    want = g[name + '_cols']
    assert (n, nsh) == (c['n'], c['nsh'])
    assert c['columns'] == sh.reader_columns(nsh)
    assert got.dtype == np.float32 and got.shape == want.shape == (14 + nsh, n)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, [(c['columns'][a], int(b), hex(got.view(np.uint32)[a, b]), hex(want.view(np.uint32)[a, b]))
                            for a, b in diff[:5]]


def test_the_two_sets_share_no_case_name():
    names = [n for _, n in CASES]
    assert len(names) == len(set(names))


# ---- what readers_edges must contain ---------------------------------------------------------------
def _spz_cases():
    for c in EDGES.meta['cases']:
        if c['format'] == 'spz':
            raw = gzip.decompress(EDGES[c['name'] + '_file'].tobytes())
            off, n, nsh, version = spz_planes(raw)
            yield c['name'], raw, off, n, nsh, version


def _ksplat_cases():
    for c in EDGES.meta['cases']:
        if c['format'] == 'ksplat':
            data = EDGES[c['name'] + '_file'].tobytes()
            yield (c['name'], data) + ksplat_sections(data)


@pytest.mark.parametrize('version', [2, 3])
def test_edges_spz_plane_skews(version):
    seen = {p: set() for p in ('alpha', 'colour', 'scale', 'sh')}
    for _, _, off, n, nsh, v in _spz_cases():
        if v == version and n:
            for p in seen:
                if p != 'sh' or nsh:  # (an SH plane of no bytes is not staged from anywhere)
                    seen[p].add(off[p] % 4)
    assert {1, 2, 3} <= seen['alpha'], seen
    assert 2 in seen['colour'], seen
    assert {1, 2, 3} <= seen['scale'], seen
    assert {1, 2, 3} <= seen['sh'], seen


def test_edges_spz_file_lengths_and_tiles():
    lengths = {len(raw) % 4 for _, raw, *_ in _spz_cases()}
    assert {1, 2, 3} <= lengths, lengths
    rows = {n for _, _, _, n, _, _ in _spz_cases()}
    assert {257, 258, 259} <= rows and {1, 2, 3, 5} <= rows, rows
    # degrees 0 and 2 at every residue of n, degrees 1 and 3 at an odd n
    by_degree = {d: {n % 4 for _, _, _, n, nsh, _ in _spz_cases() if nsh == k and n > 255}
                 for d, k in enumerate((0, 9, 24, 45))}
    assert {1, 2, 3} <= by_degree[0] and {1, 2, 3} <= by_degree[2], by_degree
    assert by_degree[1] & {1, 3} and by_degree[3] & {1, 3}, by_degree
    # both versions at every residue
    for version in (2, 3):
        assert {1, 2, 3} <= {n % 4 for _, _, _, n, _, v in _spz_cases() if v == version and n > 255}


def test_edges_spz_directed_rotation_words():
    name = 'spz_v3_rot_directed'
    raw = gzip.decompress(EDGES[name + '_file'].tobytes())
    off, n, _, version = spz_planes(raw)
    assert version == 3
    words = [int.from_bytes(raw[off['rot'] + s:off['rot'] + s + 4], 'big') for s in range(n)]
    assert {w >> 30 for w in words} == {0, 1, 2, 3}
    all_511 = [w for w in words if all((w >> (10 * k)) & 511 == 511 for k in range(3))]
    assert {w >> 30 for w in all_511} >= {0, 1}  # a component is left to the square root: 1 - 1.5 < 0
    cols = EDGES[name + '_cols']
    assert np.isnan(cols[10:14]).any()


def test_edges_ksplat_record_offsets():
    residues = {m: set() for m in (0, 1, 2)}
    lengths = set()
    for _, data, mode, sections in _ksplat_cases():
        for s in sections:
            if s['count']:
                residues[mode].add(s['data_off'] % 4)
        lengths.add(len(data) % 4)
    assert {1, 2, 3} <= set().union(*residues.values()), residues
    for mode in (0, 1, 2):
        assert residues[mode] - {0}, (mode, residues)
    assert residues[0] & {1, 3}, residues  # mode 0: an odd offset (every 4-byte read crosses a word)
    assert lengths - {0}, lengths


def test_edges_ksplat_tiles_and_partial_buckets():
    big = [(name, mode, s) for name, _, mode, sections in _ksplat_cases() for s in sections
           if s['count'] > 256 and s['partial'] > 16]
    assert {mode for _, mode, _ in big} >= {1, 2}, big
    # a second section whose first row is not a multiple of the 128-record tile and whose degree is higher
    two = [sections for _, _, _, sections in _ksplat_cases() if len(sections) == 2]
    assert any(s[0]['count'] % 128 and s[0]['degree'] < s[1]['degree'] for s in two)
    # bucket storage sizes that are no multiple of 4, and the default of 12
    storage = {s['storage'] for _, _, _, sections in _ksplat_cases() for s in sections}
    assert storage >= {12, 13, 14}, storage


def test_edges_ksplat_short_partial_sizes_reach_a_later_tile():
    """the sizes of ksplat_m2_walk257_short sum below the partial splats: rows of the second and
    third tile have NaN positions"""
    cols = EDGES['ksplat_m2_walk257_short_cols']
    nan_rows = np.flatnonzero(np.isnan(cols[0]))
    assert len(nan_rows) and nan_rows.min() >= 128 and nan_rows.max() == 256, nan_rows


def test_edges_set_is_under_one_mib():
    assert len(EDGES.blob) + os.path.getsize(os.path.join(GOLDEN, 'readers_edges.json')) < 1 << 20
