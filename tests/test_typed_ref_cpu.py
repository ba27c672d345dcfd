"""The float64 restatement of the typed-column paths (tests/typed_ref.py) pinned from both sides:
to the reference's own transform() / generateOrdering on tables of every column type
(tests/golden/typed_edges, make_golden_typed_edges.js), and to the C oracle on float32 tables.
Then the two things the fixture is for: its sub-float32 jitter really orders differently from the
float32 casts, and its wrap rows really tell a wrapping store from a clamping one.  No GPU."""
import numpy as np
import pytest

import oracle
import splat_hip as sh
import typed_ref
from golden_io import Golden
from test_gpu_edges import (DEGENERATE_CASES, TRANSFORM_EXTREMES, _table, morton_degenerate_case)
from test_oracle_golden import same_bits

G = Golden('typed_edges')
TABLES = {t['name']: t for t in G.meta['tables']}
KINDS = G.meta['kinds']
SETS = [(t['name'], s) for t in G.meta['tables'] for s in t['sets']]
INT_TABLES = [n for n, t in TABLES.items() if n.startswith('all_') and 'float' not in n]
ORDERINGS = [o['name'] for o in G.meta['ordering']]
DT = {'int8': np.int8, 'uint8': np.uint8, 'int16': np.int16, 'uint16': np.uint16, 'int32': np.int32,
      'uint32': np.uint32, 'float32': np.float32, 'float64': np.float64}


def fixture_table(name, prefix='in'):
    return {c: G[f'{name}_{prefix}_{c}'] for c in TABLES[name]['columns']}


def set_params(name, st):
    """the (t, r, s) of every transform() call of a set, as oracle.transform_params"""
    return [oracle.transform_params(t=row[:3], quat=row[3:7], s=row[7]) for row in G[f'{name}_{st}_trs']]


def classify(v, dtype, counts):
    """make_golden_typed_edges.js `classify`, vectorised: which store edge a JS number meets"""
    info = np.iinfo(dtype)
    v = np.asarray(v, np.float64)
    counts['nan'] += int(np.isnan(v).sum())
    counts['pinf'] += int((v == np.inf).sum())
    counts['ninf'] += int((v == -np.inf).sum())
    f = v[np.isfinite(v)]
    a, t = np.abs(f), np.trunc(f)
    big = a >= 2.0 ** 63
    counts['fmod'] += int((big & (a < 2.0 ** 84) & (np.fmod(t, 2.0 ** 32) != 0)).sum())
    f, t = f[~big], t[~big]
    counts['frac_to_zero'] += int(((f < 0) & (f > -1)).sum())
    counts['frac_trunc'] += int(((f < -1) & (f != t)).sum())
    counts['wrap_high'] += int((t > info.max).sum())
    counts['wrap_low'] += int((t < info.min).sum())


def test_fixture_fits_and_covers_every_type():
    import os
    from golden_io import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, 'typed_edges.bin')) <= os.path.getsize(
        os.path.join(GOLDEN, 'typed_columns.bin'))
    assert os.path.getsize(os.path.join(GOLDEN, 'typed_edges.bin')) <= 1 << 20
    for ty in DT:
        t = TABLES[f'all_{ty}']
        assert set(t['types']) == {ty} and len(t['columns']) == 10 + 9
        assert set(t['sets']) == {'rotate', 'translate', 'scale', 'chain', 'trs'}
        for c in t['columns']:
            assert G[f'all_{ty}_in_{c}'].dtype == np.dtype(DT[ty])
    for C in (0, 8, 15):
        t = TABLES[f'f64_c{C}']
        assert set(t['types']) == {'float64'} and len(t['columns']) == 10 + 3 * C
    for name in ('mixed_a', 'mixed_b'):
        t = TABLES[name]
        for grp in (typed_ref.POS, typed_ref.ROT, typed_ref.SCL, [c for c in t['columns'] if c.startswith('f_rest_')]):
            assert len({t['types'][t['columns'].index(c)] for c in grp}) >= 2, (name, grp)
    for name, drop in (('no_pos', 'y'), ('no_rot', 'rot_2'), ('no_scale', 'scale_0')):
        assert drop not in TABLES[name]['columns']


@pytest.mark.parametrize('name', INT_TABLES)
def test_every_integer_type_meets_every_store_edge(name):
    """the counts the generator recorded (from the reference's own numbers) are all > 0, and the
    restatement's numbers give the same counts"""
    rec = TABLES[name]['counts']
    for k in KINDS:
        assert rec[k] > 0, (name, k)
    counts = {k: 0 for k in KINDS}
    for st in TABLES[name]['sets']:
        cols = fixture_table(name)
        for p in set_params(name, st):
            res, _ = typed_ref.results(cols, p)
            for c, v in res.items():
                classify(v, cols[c].dtype, counts)
            typed_ref.transform(cols, p)
    assert counts == rec


@pytest.mark.parametrize('name,st', SETS)
def test_transform_restatement_equals_reference(name, st):
    """typed_ref.transform on every table and set of the fixture, byte for byte (a NaN that came
    from a NaN operand as NaN only)"""
    cols = fixture_table(name)
    taint = None
    for p in set_params(name, st):
        taint = typed_ref.transform(cols, p)
    typed_ref.same_table(cols, fixture_table(name, st), taint, f'{name} {st}')


@pytest.mark.parametrize('name', ORDERINGS)
def test_ordering_restatement_equals_reference(name):
    x, y, z = (G[f'{name}_{a}'] for a in 'xyz')
    same_bits(typed_ref.morton_order(x, y, z), G[f'{name}_order'])
    same_bits(typed_ref.morton_order(x, y, z, G[f'{name}_sub']), G[f'{name}_sub_order'])


# ---- float32 tables: the restatement equals the C oracle ---------------------------------------
def _params(action):
    kind, value = action
    return (oracle.transform_params(s=float(value)) if kind == 'scale' else
            oracle.transform_params(t=value) if kind == 'translate' else oracle.transform_params(euler=value))


@pytest.mark.parametrize('C', [0, 3, 8, 15])
@pytest.mark.parametrize('action', TRANSFORM_EXTREMES + [('trs', None)])
def test_transform_restatement_equals_oracle_on_float32(action, C):
    cols = _table(700, C, 11 + C, spice=True)
    ref = {k: v.copy() for k, v in cols.items()}
    p = (oracle.transform_params(t=(0.5, -2.0, 1e3), euler=(33, -71, 12), s=0.37) if action[0] == 'trs'
         else _params(action))
    oracle.transform(ref, p, C)
    taint = typed_ref.transform(cols, p)
    typed_ref.same_table(cols, ref, taint)


def test_ordering_restatement_equals_oracle_on_ordering_fixture():
    g = Golden('ordering')
    for name in g.meta['cases']:
        x, y, z = g[f'{name}_x'], g[f'{name}_y'], g[f'{name}_z']
        same_bits(typed_ref.morton_order(x, y, z), oracle.morton_order(x, y, z))
        same_bits(typed_ref.morton_order(x, y, z), g[f'{name}_order'])


@pytest.mark.parametrize('case', DEGENERATE_CASES)
@pytest.mark.parametrize('n', [5000, 70001])
def test_ordering_restatement_equals_oracle_on_degenerate_cases(case, n):
    x, y, z = morton_degenerate_case(case, n)
    same_bits(typed_ref.morton_order(x, y, z), oracle.morton_order(x, y, z))
    idx = np.random.default_rng(n).integers(0, n, n // 2).astype(np.uint32)
    same_bits(typed_ref.morton_order(x, y, z, idx), oracle.morton_order(x, y, z, idx))


@pytest.mark.parametrize('spice', [False, True])
def test_sog_member_textures_equal_oracle_on_float32(spice):
    n = 3000
    cols = _table(n, 0, 77)
    if spice:
        rng = np.random.default_rng(1)
        for i in range(4):
            cols[f'rot_{i}'][rng.random(n) < 0.05] = 0.0
        for i in range(4):
            cols[f'rot_{i}'][3::17] = 0.0  # all-zero quaternions: 0 / 0
        cols['rot_2'][::7] = -5.0
        cols['opacity'][::11] = np.nan
        cols['opacity'][1::11] = 200.0
        cols['opacity'][2::11] = -800.0
        cols['y'][5] = np.nan
        cols['x'][::13] = -0.0
    rc, otex, ometa, _ = oracle.sog(cols, 0, 2, oracle.mulberry32(3, 1 << 14))
    assert rc == 0
    order = oracle.morton_order(cols['x'], cols['y'], cols['z'])
    tex, mins, maxs = typed_ref.sog_member_textures(cols, order)
    for k in ('means_l', 'means_u', 'quats'):
        same_bits(tex[k], otex[k].reshape(-1)[:4 * n])
    same_bits(tex['sh0_alpha'], otex['sh0'].reshape(-1)[3:4 * n:4])
    same_bits(mins, np.array(ometa.means_min[:]))
    same_bits(maxs, np.array(ometa.means_max[:]))


# ---- discrimination ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ORDERINGS)
def test_sub_float32_jitter_orders_differently_from_the_float32_casts(name):
    """the fixture's clumps are one point to float32, so an ordering that rounded to float32
    anywhere would leave them in index order"""
    x, y, z = (G[f'{name}_{a}'] for a in 'xyz')
    cast = oracle.morton_order(*(np.ascontiguousarray(a.astype(np.float32)) for a in (x, y, z)))
    want = G[f'{name}_order']
    assert sorted(cast.tolist()) == sorted(want.tolist())
    assert (cast != want).sum() > len(want) // 2


@pytest.mark.parametrize('kind', ['wrap_high', 'wrap_low', 'fmod'])
@pytest.mark.parametrize('name', INT_TABLES)
def test_a_clamping_store_would_differ(name, kind):
    """every stored value that wrapped (or went through ToInt32's modulo at 2^63 and above) holds
    other bytes than a saturating store would have written"""
    seen = differ = 0
    info = np.iinfo(DT[TABLES[name]['types'][0]])
    for st in TABLES[name]['sets']:
        cols = fixture_table(name)
        want = fixture_table(name, st)
        params = set_params(name, st)
        for i, p in enumerate(params):
            res, _ = typed_ref.results(cols, p)
            typed_ref.transform(cols, p)
            if i + 1 < len(params):
                continue  # the fixture holds the table after the set's last call
            for c, v in res.items():
                with np.errstate(invalid='ignore'):
                    t = np.trunc(v)
                    fin = np.isfinite(v)
                    big = fin & (np.abs(v) >= 2.0 ** 63)
                    rows = {'wrap_high': fin & ~big & (t > info.max), 'wrap_low': fin & ~big & (t < info.min),
                            'fmod': big & (np.abs(v) < 2.0 ** 84) & (np.fmod(t, 2.0 ** 32) != 0)}[kind]
                seen += int(rows.sum())
                differ += int((typed_ref.clamp_store(v, cols[c].dtype)[rows] != want[c][rows]).sum())
    assert seen > 0
    # a wrapped value equals the saturated one only when it lands on the type's end by chance
    assert differ >= seen * 0.9, (seen, differ)


# ---- oracle.process on typed tables --------------------------------------------------------------
TC = Golden('typed_columns')


@pytest.mark.parametrize('case', TC.meta['cases'])
def test_oracle_process_reproduces_typed_columns(case):
    """oracle.process transforms columns of every type (it used to leave all but the float32 ones
    untouched): the processed table, and the input table after the transforms that precede the
    first filter (the reference mutates it in place), as the reference left them"""
    acts = TC.meta[f'{case}_actions']
    src = [(k, TC[f'{case}_in_{k}']) for k in TC.meta[f'{case}_in_columns']]
    out = oracle.process(src, acts)
    assert [k for k, _ in out] == TC.meta[f'{case}_out_columns']
    for k, a in out:
        same_bits(a, TC[f'{case}_out_{k}'])
    # filterBands renames columns without copying them, so a transform after it still mutates
    # the input's arrays: the region runs up to the first row filter
    first = next((i for i, a in enumerate(acts) if a['kind'] in ('filterNaN', 'filterByValue')), len(acts))
    region = acts[:first]
    after = [a.copy() for _, a in src]
    for (_, a), (_, _, j) in zip(oracle.process(src, region), sh.process_schema(src, region, with_source=True)):
        after[j] = a
    assert [k for k, _ in src] == TC.meta[f'{case}_after_columns']
    for (k, _), a in zip(src, after):
        same_bits(a, TC[f'{case}_after_{k}'])
