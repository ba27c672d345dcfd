"""The typed twins of the float32 kernels at the float32 edges: k_transform_t, morton_order_impl
<double>, the typed chunk packer and sog_tdev on columns that are not float32, bit for bit.

Two references ("Typed columns: the two references"): (a) for carriers whose values
are all float32 values the C oracle on the float32 casts is exact, since the reference reads the
same JS numbers from either array; (b) tests/typed_ref.py, the float64 restatement pinned to the
reference by tests/golden/typed_edges, for inputs no float32 holds and for the typed stores."""
import functools

import numpy as np
import pytest

import oracle
import splat_hip as sh
import typed_ref
from golden_io import Golden
from test_gpu_edges import (DEGENERATE_CASES, ONESWEEP_N, PACK_EDGES, RAGGED_N, TRANSFORM_EXTREMES, _table,
                            morton_degenerate_case, morton_onesweep_case, morton_ragged_case)
from test_oracle_golden import same_bits

pytestmark = pytest.mark.gpu

G = Golden('typed_edges')
TABLES = {t['name']: t for t in G.meta['tables']}
SETS = [(t['name'], s) for t in G.meta['tables'] for s in t['sets']]


@pytest.fixture(scope='module')
def ctx():
    import torch  # noqa: F401  (torch's HIP runtime first: see splat_hip.Context)
    c = sh.Context(0)
    yield c
    c.close()


def f32(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float32))


# ---- ordering ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _degenerate(case, n):
    """the float32 case, its oracle order and a permutation with its oracle order: reference (a)"""
    x, y, z = morton_degenerate_case(case, n)
    perm = np.random.default_rng(n + len(case)).permutation(n).astype(np.uint32)
    return (x, y, z), oracle.morton_order(x, y, z), perm, oracle.morton_order(x, y, z, perm)


@pytest.mark.parametrize('n', RAGGED_N)
def test_morton_float64_ragged(ctx, n):
    x, y, z = morton_ragged_case(n)
    same_bits(ctx.morton_order(*(a.astype(np.float64) for a in (x, y, z))), oracle.morton_order(x, y, z))


@pytest.mark.parametrize('case,n', [(c, n) for n in (5000, 70001) for c in DEGENERATE_CASES] + [('clumps', 1_000_003)])
def test_morton_float64_degenerate(ctx, case, n):
    """every degenerate float32 case through morton_order_impl<double>: 64-bit extent keys, NaN and
    Inf extents, zero extents, the recursion over equal-key runs, the identity and a permutation"""
    (x, y, z), want, perm, want_perm = _degenerate(case, n)
    d = [a.astype(np.float64) for a in (x, y, z)]
    same_bits(ctx.morton_order(*d), want)
    same_bits(ctx.morton_order(*d, perm), want_perm)


@pytest.mark.parametrize('n', ONESWEEP_N)
def test_morton_float64_onesweep_sizes(ctx, n):
    x, y, z, perm = morton_onesweep_case(n)
    d = [a.astype(np.float64) for a in (x, y, z)]
    same_bits(ctx.morton_order(*d, perm), oracle.morton_order(x, y, z, perm))
    same_bits(ctx.morton_order(*d), oracle.morton_order(x, y, z))


@pytest.mark.parametrize('dtype', [np.int8, np.int16, np.int32])
@pytest.mark.parametrize('case', ['lattice', 'all_equal', 'one_axis_flat'])
@pytest.mark.parametrize('n', [5000, 70001])
def test_morton_integer_carriers(ctx, case, dtype, n):
    """integer columns are where runs of exact duplicates come from: the coordinates rounded to
    integers (|v| < 40 fits an int8), carried as int8 / int16 / int32"""
    r = [np.round(a) for a in morton_degenerate_case(case, n)]
    assert max(np.abs(a).max() for a in r) < 127
    want = oracle.morton_order(*(f32(a) for a in r))
    same_bits(ctx.morton_order(*(a.astype(dtype) for a in r)), want)


def test_morton_three_types_on_three_axes(ctx):
    x, y, z = morton_degenerate_case('lattice', 70001)
    x, z = np.round(x), np.round(z)
    want = oracle.morton_order(f32(x), y, f32(z))
    same_bits(ctx.morton_order(x.astype(np.int8), y.astype(np.float64), z.astype(np.int32)), want)
    same_bits(ctx.morton_order(x.astype(np.int16), y, z.astype(np.float64)), want)  # float32 in the middle


def jitter_clumps(n, nan):
    """~600-member clumps near 1 whose members differ by less than a float32 can hold: to float32
    every clump is one point, in float64 every level of the recursion has extents of its own"""
    rng = np.random.default_rng(n + nan)
    x, y, z = (rng.normal(0, 5, n) for _ in range(3))
    m = rng.random(n) < 0.8
    cid = rng.integers(0, max(1, int(n * 0.8) // 600), n)
    for a in (x, y, z):
        cen = 1 + rng.integers(0, 64, cid.max() + 1) / 64
        a[m] = cen[cid[m]] + rng.random(m.sum()) * 1e-12
    if nan:
        x[rng.random(n) < 0.02] = np.nan
        z[m & (rng.random(n) < 0.01)] = np.nan
    return x, y, z


@pytest.mark.parametrize('nan', [0, 1])
def test_morton_sub_float32_jitter(ctx, nan):
    """reference (b): the order depends on bits below float32 resolution at every level below the
    first, so any rounding to float32 inside the double ordering shows"""
    n = 70001
    x, y, z = jitter_clumps(n, nan)
    want = typed_ref.morton_order(x, y, z)
    assert (oracle.morton_order(f32(x), f32(y), f32(z)) != want).sum() > n // 2
    same_bits(ctx.morton_order(x, y, z), want)
    perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
    same_bits(ctx.morton_order(x, y, z, perm), typed_ref.morton_order(x, y, z, perm))


@pytest.mark.parametrize('name', [o['name'] for o in G.meta['ordering']])
def test_morton_fixture_orderings(ctx, name):
    """the reference's own orders of the float64 and the int16 / float64 / int32 set"""
    x, y, z = (G[f'{name}_{a}'] for a in 'xyz')
    same_bits(ctx.morton_order(x, y, z), G[f'{name}_order'])


@pytest.mark.parametrize('n', [3000, 70001])
def test_morton_float64_index_lists_with_repeats(ctx, n):
    """an index list that repeats rows and leaves others out.  The Python binding has no typed
    index-list entry point of its own: morton_order(..., indices) hands the list to
    st_morton_order_t, which takes one length for the columns and the list"""
    rng = np.random.default_rng(n)
    x, y, z = (rng.normal(0, 3, n).astype(np.float32) for _ in range(3))
    x[rng.random(n) < 0.01] = np.nan
    idx = rng.integers(0, n, n).astype(np.uint32)
    assert len(np.unique(idx)) < n
    same_bits(ctx.morton_order(*(a.astype(np.float64) for a in (x, y, z)), idx), oracle.morton_order(x, y, z, idx))
    j = jitter_clumps(n, 1)
    same_bits(ctx.morton_order(*j, idx), typed_ref.morton_order(*j, idx))


# ---- transform -----------------------------------------------------------------------------------
def _gpu_params(row):
    return sh.transform_params(t=tuple(row[:3]), r=tuple(row[3:7]), s=float(row[7]))


def _ref_params(row):
    return oracle.transform_params(t=row[:3], quat=row[3:7], s=row[7])


@pytest.mark.parametrize('name,st', SETS)
def test_transform_fixture_tables(ctx, name, st):
    """every table and set of tests/golden/typed_edges against the reference's own output: all
    eight types at every store edge, float64 at every SH band, mixed groups, missing groups"""
    cols = {c: G[f'{name}_in_{c}'] for c in TABLES[name]['columns']}
    ref = {k: v.copy() for k, v in cols.items()}
    taint = None
    for row in G[f'{name}_{st}_trs']:
        ctx.transform(cols, _gpu_params(row))
        taint = typed_ref.transform(ref, _ref_params(row))
    want = {c: G[f'{name}_{st}_{c}'] for c in TABLES[name]['columns']}
    typed_ref.same_table(cols, want, taint, f'{name} {st}')


def _action_params(action):
    kind, value = action
    return (oracle.transform_params(s=float(value)) if kind == 'scale' else
            oracle.transform_params(t=value) if kind == 'translate' else oracle.transform_params(euler=value))


@pytest.mark.parametrize('C', [0, 3, 8, 15])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 2000])
@pytest.mark.parametrize('action', TRANSFORM_EXTREMES)
def test_transform_float64_extremes(ctx, action, n, C):
    """the spiced table (NaN / Inf / -0, scales past the clamp, zero quaternions) as float64 under
    the five extreme actions, around the 256-thread block, at every SH band: reference (b)"""
    cols = {k: v.astype(np.float64) for k, v in _table(n, C, 11, spice=True).items()}
    ref = {k: v.copy() for k, v in cols.items()}
    taint = typed_ref.transform(ref, _action_params(action))
    ctx.transform(cols, sh.action_params(*action))
    typed_ref.same_table(cols, ref, taint)


BIG_N = 2_097_153 + 257  # past the 8,192 blocks of 256 threads the launch is capped at


def _big_table(dtype):
    rng = np.random.default_rng(99)
    cols = {k: rng.normal(0, 3, BIG_N).astype(dtype) for k in ('x', 'y', 'z', 'rot_0', 'rot_1', 'rot_2', 'rot_3')}
    for k, v in ((0, np.nan), (BIG_N - 1, np.inf), (2_097_152, -np.inf), (2_097_153, -0.0)):
        cols['x'][k] = v
        cols['rot_2'][k] = v
    return cols


def test_transform_float64_grid_stride(ctx):
    """more rows than threads launched: k_transform_t's grid-stride loop, its SCL = false and
    C = 0 form (no scale columns, no SH)"""
    cols = _big_table(np.float64)
    ref = {k: v.copy() for k, v in cols.items()}
    quat = sh.quat_from_euler(10, 20, 30)
    taint = typed_ref.transform(ref, oracle.transform_params(t=(0.5, -2, 1e3), quat=quat, s=0.37))
    ctx.transform(cols, sh.transform_params(t=(0.5, -2, 1e3), r=tuple(quat), s=0.37))
    typed_ref.same_table(cols, ref, taint)


def test_transform_float32_grid_stride(ctx):
    """the same shape through the float32 kernel against the C oracle"""
    cols = _big_table(np.float32)
    ref = {k: v.copy() for k, v in cols.items()}
    quat = sh.quat_from_euler(10, 20, 30)
    oracle.transform(ref, oracle.transform_params(t=(0.5, -2, 1e3), quat=quat, s=0.37), 0)
    ctx.transform(cols, sh.transform_params(t=(0.5, -2, 1e3), r=tuple(quat), s=0.37))
    for k in cols:
        same_bits(cols[k], ref[k])


# ---- chunk packing and writeSog on float32-representable carriers: reference (a) -------------------
def _integer_mix(cols, C):
    """int8 scales and uint8 / int8 f_rest columns holding in-range integers; the rest float64"""
    rng = np.random.default_rng(len(cols['x']) + C)
    n = len(cols['x'])
    out = {k: v.astype(np.float64) for k, v in cols.items()}
    for i in range(3):
        out[f'scale_{i}'] = rng.integers(-30, 31, n).astype(np.int8)  # past the +-20 clamp both ways
    for i in range(3 * C):
        out[f'f_rest_{i}'] = (rng.integers(0, 256, n).astype(np.uint8) if i % 2 else
                              rng.integers(-128, 128, n).astype(np.int8))
    return out


@pytest.mark.parametrize('mix', ['float64', 'integers'])
@pytest.mark.parametrize('n,C', PACK_EDGES)
def test_compressed_ply_typed_edges(ctx, n, C, mix):
    """the typed chunk packer on the spiced table: NaN-propagating chunk min/max, the scale clamp,
    zero quaternions, the padded last chunk, SH byte saturation from float64 and integer columns"""
    base = _table(n, C, 100 + n, spice=True)
    cols = {k: v.astype(np.float64) for k, v in base.items()} if mix == 'float64' else _integer_mix(base, C)
    _, chunk, vertex, shb = oracle.compressed_ply([(k, f32(v)) for k, v in cols.items()], [])
    m, gchunk, gvertex, gsh = ctx.compressed_ply(cols, [])
    assert m == n
    for g, w in ((gchunk, chunk), (gvertex, vertex), (gsh, shb)):
        same_bits(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8))


SOG_SHAPES = [(5000, 0), (5000, 3), (5000, 8), (5000, 15),
              (1, 3), (2, 0), (17, 8), (85, 0), (86, 0), (300, 15), (1023, 3), (1025, 15)]


@functools.lru_cache(maxsize=None)
def _sog_reference(n, C):
    """test_sog_all_bands' and test_sog_small_tables' tables, their draws and the oracle's writeSog"""
    cols = _table(n, C, 40 + C) if n == 5000 else _table(n, C, 500 + n)
    draws = oracle.mulberry32(C + 1, 1 << 15) if n == 5000 else oracle.mulberry32(n, 1 << 14)
    return cols, draws, oracle.sog(cols, C, 3, draws)


def _check_sog(tex, meta, used, otex, ometa, oused):
    assert used == oused
    assert set(tex) == set(otex)
    for k in tex:
        same_bits(tex[k], otex[k])
    for f in ('width', 'height', 'sh_bands', 'palette_size', 'shn_width', 'shn_height'):
        assert getattr(meta, f) == getattr(ometa, f), f
    for f in ('means_min', 'means_max', 'scales_codebook', 'sh0_codebook', 'shn_codebook'):
        same_bits(np.array(getattr(meta, f)[:]), np.array(getattr(ometa, f)[:]))


@pytest.mark.parametrize('which', ['all_float64', 'positions_float64'])
@pytest.mark.parametrize('n,C', SOG_SHAPES)
def test_sog_typed_edges(ctx, n, C, which):
    """writeSog of a typed table for every SH band and for the small tables: float64 everywhere
    (pos64 / rot64 / op64 / sh64 all set), and float64 positions only (the others stay null)"""
    base, draws, (rc, otex, ometa, oused) = _sog_reference(n, C)
    cols = {k: (v.astype(np.float64) if which == 'all_float64' or k in ('x', 'y', 'z') else v) for k, v in base.items()}
    if 3 * n < 256:
        assert rc != 0
        with pytest.raises(sh.StError):
            ctx.sog_process(cols, [], 3, draws)
        return
    assert rc == 0
    tex, meta, used = ctx.sog_process(cols, [], 3, draws)
    _check_sog(tex, meta, used, otex, ometa, oused)


def test_sog_float64_members(ctx):
    """positions, rotations and opacity that no float32 holds: sub-float32 jitter in clumped
    positions (the Morton order and the means quantisation see it), quaternions of all zeros and
    with a negative largest component, opacities at both saturation ends: reference (b)"""
    n = 5000
    rng = np.random.default_rng(8)
    cols = dict(_table(n, 0, 123))
    cols['x'], cols['y'], cols['z'] = jitter_clumps(n, 0)
    for i in range(4):
        cols[f'rot_{i}'] = rng.normal(0, 1, n)
    zero, neg = rng.random(n) < 0.03, rng.random(n) < 0.2
    for i in range(4):
        cols[f'rot_{i}'][zero] = 0.0
    cols['rot_2'][neg] = -5.0 - rng.random(neg.sum())
    cols['opacity'] = rng.normal(0, 3, n)
    cols['opacity'][::97] = 800.0
    cols['opacity'][1::97] = -800.0
    order = typed_ref.morton_order(cols['x'], cols['y'], cols['z'])
    assert (oracle.morton_order(f32(cols['x']), f32(cols['y']), f32(cols['z'])) != order).sum() > n // 2
    want, mins, maxs = typed_ref.sog_member_textures(cols, order)
    tex, meta, _ = ctx.sog_process(cols, [], 3, oracle.mulberry32(2, 1 << 15))
    for k in ('means_l', 'means_u', 'quats'):
        same_bits(tex[k].reshape(-1)[:4 * n], want[k])
        assert not tex[k].reshape(-1)[4 * n:].any()
    same_bits(tex['sh0'].reshape(-1)[3:4 * n:4], want['sh0_alpha'])
    same_bits(np.array(meta.means_min[:]), mins)
    same_bits(np.array(meta.means_max[:]), maxs)
