"""The .splat / .ksplat / .spz readers' host side (no GPU): st_*_layout against the reference's
own readers (tests/golden/readers.*: readSplat / readKsplat / readSpz run on seeded files, their
row and column counts, and for the files they reject the message of the error they throw), and
Context.read_table's dispatch on the file name.
"""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import splat_hip as sh
from golden_io import Golden

G = Golden('readers')
CASES = {c['name']: c for c in G.meta['cases']}
ERRORS = {e['name']: e for e in G.meta['errors']}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference names these as something it does not support; every other rejection is a bad file
UNSUPPORTED = ('Unsupported version', 'Invalid compression mode')


def file_bytes(name, size=None):
    return G[name + '_file'].tobytes() if size is None or size else b''


def layout(fmt, data):
    """st_<fmt>_layout of a file's bytes as Context.read_<fmt> calls it"""
    if fmt == 'splat':
        return sh.splat_layout(len(data))
    if fmt == 'ksplat':
        return sh.ksplat_layout(data)
    return sh.spz_layout(sh.spz_inflate(data))


@pytest.mark.parametrize('name', list(CASES))
def test_layout_matches_reference(name):
    c = CASES[name]
    assert layout(c['format'], file_bytes(name)) == (c['n'], c['nsh'])
    assert c['columns'] == sh.reader_columns(c['nsh'])


@pytest.mark.parametrize('name', list(ERRORS))
def test_layout_rejects_what_the_reference_rejects(name):
    e = ERRORS[name]
    with pytest.raises(sh.StError) as ei:
        layout(e['format'], file_bytes(name, e['size']))
    want = sh.ST_ERR_UNSUPPORTED if e['message'].startswith(UNSUPPORTED) else sh.ST_ERR_ARG
    assert ei.value.code == want
    assert e['message'] in str(ei.value)
    if not (name == 'spz_err_raw'):  # (that one is the Python wrapper's: the library never sees a raw file)
        assert e['message'] in sh.lib().st_last_error().decode()


def test_error_cases_cover_the_issue_list():
    assert set(ERRORS) == {
        'splat_err_size', 'splat_err_empty',
        'ksplat_err_short', 'ksplat_err_version', 'ksplat_err_mode', 'ksplat_err_zero', 'ksplat_err_mismatch',
        'ksplat_err_truncated', 'ksplat_err_misaligned',
        'spz_err_magic', 'spz_err_version', 'spz_err_raw', 'spz_err_truncated', 'spz_err_v3_n1'}


def test_ksplat_layout_needs_only_the_headers_of_a_longer_file():
    # the layout call over the whole file and the planner over its headers agree on a file whose
    # every section view fits: cutting one byte anywhere after the headers is caught
    data = file_bytes('ksplat_two_sections')
    assert sh.ksplat_layout(data) == (100, 24)
    with pytest.raises(sh.StError):
        sh.ksplat_layout(data[:-1])


def test_read_table_unknown_suffix(tmp_path):
    p = tmp_path / 'scene.obj'
    p.write_bytes(b'x')
    ctx = sh.Context.__new__(sh.Context)  # the dispatch needs no device
    ctx.h = None
    with pytest.raises(sh.StError) as ei:
        ctx.read_table(str(p))
    assert 'Unsupported input file type' in str(ei.value)


# ---- the decoders' arithmetic on the host: st_readers.hip's __host__ __device__ decode functions
# in a stand-alone program (tests/native/readers_cpu_check.cpp), every column bit-equal
_HARNESS = []  # built once per session into a directory of its own (removed at exit)
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def _harness():
    if not _HARNESS:
        d = tempfile.mkdtemp(prefix='st_readers_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'readers_cpu_check')
        subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-ffp-contract=off', '-o', exe,
                               os.path.join(ROOT, 'tests', 'native', 'readers_cpu_check.cpp')])
        _HARNESS.append(exe)
    return _HARNESS[0]


@pytest.mark.parametrize('name', list(CASES))
def test_host_decode_matches_reference(name, tmp_path):
    c = CASES[name]
    data = file_bytes(name)
    src, dst = tmp_path / 'in.bin', tmp_path / 'out.f32'
    src.write_bytes(sh.spz_inflate(data) if c['format'] == 'spz' else data)
    r = subprocess.run([_harness(), c['format'], str(src), str(dst)], capture_output=True, text=True, check=True)
    assert r.stdout.strip() == f'OK {c["n"]} {c["nsh"]}'
    want = G[name + '_cols']
    got = np.fromfile(dst, np.float32).reshape(want.shape)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(diff) == 0, [(c['columns'][a], int(b), hex(got.view(np.uint32)[a, b]), hex(want.view(np.uint32)[a, b]))
                            for a, b in diff[:5]]
