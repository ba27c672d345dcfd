"""The HTML viewer writer on the host side (no GPU): the Python restatement of writeHtml
(tests/write_html_ref.py) against the reference's own files (tests/golden/write_html.*: V8's
String.prototype.replace and JSON.stringify, Node's base64 of the reference's compressed-PLY file),
and the product's page text (st_html_parts) against the restatement: the fixture templates, a few
hundred random templates assembled from the patterns, '$' sequences and newlines, and the settings
text of the CSV fixture's float64 boundary values.
"""
import base64
import os
import random

import numpy as np
import pytest

import oracle
import splat_hip as sh
import write_csv_ref
import write_html_ref as ref
from golden_io import Golden

H = Golden('write_html')
CASES = list(H.meta)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_columns(name):
    """[(column name, float32 array)] of a write_html fixture case"""
    return [(k, H[f'{name}_col{i}']) for i, k in enumerate(H.meta[name]['columns'])]


def case_file(name):
    return H[f'{name}_file'].tobytes()


def case_template(name):
    """(html, css, js) as str"""
    return tuple(H[f'{name}_{k}'].tobytes().decode('utf-8') for k in ('html', 'css', 'js'))


def case_view(name):
    return H[f'{name}_camera'], H[f'{name}_target']


_PLY = {}


def case_ply(name):
    """the case's .compressed.ply file by the oracle (computed once): bytes"""
    if name not in _PLY:
        m = H.meta[name]
        _, chunk, vertex, shb = oracle.compressed_ply(case_columns(name), [])
        _PLY[name] = ref.compressed_ply_file(m['rows'], m['sh_coeffs'], chunk, vertex, shb)
    return _PLY[name]


def test_fixture_covers_the_cases():
    assert set(CASES) == {'plain', 'mod3_1', 'mod3_2', 'mod3_3', 'sh3', 'dollars', 'nested', 'missing', 'camera',
                          'utf8'}
    m = H.meta
    assert m['plain']['rows'] == 300 and m['plain']['sh_coeffs'] == 0
    html, css, js = case_template('plain')
    for pat in (ref.STYLE, ref.SCRIPT, ref.SETTINGS, ref.CONTENT):
        assert html.count(pat) == 1
    for t in (css, js):
        assert '\n\n' in t and t.endswith('\n')
    # the three residues of the payload's length, from one header length
    assert [m[f'mod3_{i}']['rows'] for i in (1, 2, 3)] == [1, 2, 3]
    plys = [case_ply(f'mod3_{i}') for i in (1, 2, 3)]
    assert len({p.index(b'end_header\n') for p in plys}) == 1
    assert [len(b) - len(a) for a, b in zip(plys, plys[1:])] == [16, 16]
    assert {len(p) % 3 for p in plys} == {0, 1, 2}
    tails = set()
    for i in (1, 2, 3):
        f = case_file(f'mod3_{i}')
        text = f[f.index(b'base64,') + 7:f.index(b'")', f.index(b'base64,'))]
        tails.add(len(text) - len(text.rstrip(b'=')))
    assert tails == {0, 1, 2}
    assert m['sh3']['rows'] == 257 and m['sh3']['sh_coeffs'] == 15 and len(m['sh3']['columns']) == 14 + 45
    _, css, js = case_template('dollars')
    for seq in ('$$', '$&', '$`', "$'", '$1', '$<a>'):
        assert seq in css + js
    assert css.endswith('$') and js.endswith('$')
    html, css, js = case_template('nested')
    assert ref.SCRIPT in css and ref.CONTENT in css
    for pat in (ref.STYLE, ref.SCRIPT, ref.SETTINGS, ref.CONTENT):
        assert html.count(pat) == 2
    html, _, _ = case_template('missing')
    assert ref.CONTENT not in html and ref.STYLE not in html
    cam, tgt = case_view('camera')
    assert cam.tolist()[1:] == [1e21, 1e-7] and np.signbit(cam[0]) and cam[0] == 0
    assert tgt[0] == 0.1 and np.isnan(tgt[1]) and np.isinf(tgt[2])
    html, css, js = case_template('utf8')
    assert all(any(ord(ch) > 127 for ch in t) for t in (html, css, js)) and any(ord(ch) > 0xffff for ch in html)
    assert any(ord(ch) > 127 for ch in html[:html.index(ref.STYLE)])
    assert any(ord(ch) > 127 for ch in html[html.index(ref.SETTINGS):html.index(ref.CONTENT)])
    for ext in ('bin', 'json'):
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f'write_html.{ext}')) < 1 << 20


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference(name):
    cam, tgt = case_view(name)
    assert ref.write_html(*case_template(name), cam, tgt, case_ply(name)) == case_file(name)


def test_restatement_examples():
    """String.prototype.replace with a string pattern, as V8 runs it"""
    s = 'A[X]B[X]C'
    assert ref.js_replace(s, '[X]', "<$$|$&|$`|$'|$1|$0|$01|$<n>|$>") == 'A<$|[X]|A|B[X]C|$1|$0|$01|$<n>|$>B[X]C'
    assert ref.js_replace(s, '[X]', 'end$') == 'Aend$B[X]C'
    assert ref.js_replace(s, '[Y]', '$&') == s
    assert ref.pad('a\n\nb\n', 2) == '  a\n  \n  b\n  '
    assert ref.settings_json([-0.0, 1e21, 1e-7], [0.1, float('nan'), float('inf')]) == \
        ('{"camera":{"fov":50,"position":[0,1e+21,1e-7],"target":[0.1,null,null],"startAnim":"none"},'
         '"background":{"color":[0.4,0.4,0.4]},"animTracks":[]}')


# ---- the product's host-only calls -----------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_html_parts_matches_reference(name):
    cam, tgt = case_view(name)
    prefix, suffix, embeds = sh.html_parts(*case_template(name), cam, tgt)
    assert (prefix, suffix, embeds) == ref.parts(*case_template(name), cam, tgt)
    file = case_file(name)
    if name == 'missing':
        assert embeds == 0 and suffix == b'' and prefix == file
    else:
        assert embeds == 1 and prefix.endswith(b'fetch("data:application/ply;base64,') and suffix.startswith(b'")')
        assert file == prefix + base64.b64encode(case_ply(name)) + suffix
    # the template as UTF-8 bytes is the same call
    assert sh.html_parts(*[t.encode('utf-8') for t in case_template(name)], cam, tgt) == (prefix, suffix, embeds)


def test_html_parts_defaults():
    html, css, js = case_template('plain')
    assert sh.html_parts(html, css, js) == ref.parts(html, css, js, (2, 2, -2), (0, 0, 0))


def random_template(rng):
    atoms = [ref.STYLE, ref.SCRIPT, ref.SETTINGS, ref.CONTENT, '$$', '$&', '$`', "$'", '$1', '$0', '$<a>', '$', '\n',
             '\n\n', ' ', 'x', 'fetch(', 'settings: ', '<link', 'é', '視', '🎥', '{}', '"']
    weights = [3, 3, 3, 3] + [1] * (len(atoms) - 4)
    return tuple(''.join(rng.choices(atoms, weights, k=rng.randrange(0, 14))) for _ in range(3))


def test_html_parts_on_random_templates():
    rng = random.Random(20)
    seen = {0: 0, 1: 0}
    for _ in range(400):
        html, css, js = random_template(rng)
        cam = [rng.choice([0.0, -0.0, 1.5, 1e21, 1e-7, float('nan'), -float('inf'), rng.gauss(0, 10)]) for _ in range(3)]
        tgt = [rng.gauss(0, 1e-3) for _ in range(3)]
        want = ref.parts(html, css, js, cam, tgt)
        assert sh.html_parts(html, css, js, cam, tgt) == want, (html, css, js)
        seen[want[2]] += 1
    assert min(seen.values()) > 40


def test_settings_numbers_at_the_float64_edges():
    """every value of the CSV fixture's edges64 column through the settings text, three per call:
    Number::toString's digits (write_csv_ref), null for what is not finite"""
    v = Golden('write_csv')['edges64_col0']
    v = np.concatenate([v, np.zeros(-len(v) % 6)])
    for row in v.reshape(-1, 6).tolist():
        prefix, suffix, embeds = sh.html_parts(ref.SETTINGS, '', '', row[:3], row[3:])
        nums = [write_csv_ref.js_number(x) if np.isfinite(x) else 'null' for x in row]
        want = ('settings: {"camera":{"fov":50,"position":[' + ','.join(nums[:3]) + '],"target":[' +
                ','.join(nums[3:]) + '],"startAnim":"none"},"background":{"color":[0.4,0.4,0.4]},"animTracks":[]}')
        assert (prefix.decode(), suffix, embeds) == (want, b'', 0), row


def test_base64_size():
    for n in list(range(0, 50)) + [3071, 3072, 3073, 2**32 - 1, 2**32, 2**40 + 1]:
        assert sh.base64_size(n) == 4 * ((n + 2) // 3)
        if n < 5000:
            assert sh.base64_size(n) == len(base64.b64encode(bytes(n)))


def test_null_template_is_an_error():
    import ctypes
    out = [ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int32()]
    v = (ctypes.c_double * 3)(0, 0, 0)
    for tpl in ((None, b'', b''), (b'', None, b''), (b'', b'', None)):
        rc = sh.lib().st_html_parts(*tpl, v, v, *[ctypes.byref(o) for o in out])
        assert rc == sh.ST_ERR_ARG and out[0].value is None
