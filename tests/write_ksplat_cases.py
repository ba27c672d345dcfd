"""Shared by the .ksplat writer's CPU and GPU tests: the fixture files' sections with their own bucket
tables (from the file's bytes, via readers_files), the classes of fields a decode cannot give back
(computed from the file's bytes alone), and the tables whose plan is known by construction."""
import struct

import numpy as np

import splat_hip as sh
import write_ksplat_ref as ref
from golden_io import Golden
from readers_files import KS_COLOUR, SH_COUNT, ksplat_sections

SETS = {name: Golden(name) for name in ('readers', 'readers_edges')}
KSPLAT_CASES = [(s, c['name']) for s, g in SETS.items() for c in g.meta['cases'] if c['format'] == 'ksplat']
NINE = [f'ksplat_m{m}_d{d}' for m in range(3) for d in range(3)]
DEFAULT_QUANT = (1, 32767, 32767)


def fixture(set_name, name):
    g = SETS[set_name]
    c = next(c for c in g.meta['cases'] if c['name'] == name)
    return g[name + '_file'].tobytes(), g[name + '_cols'], c


def sections(data, cols):
    """per non-empty section of a fixture file: its table (the reference's decoded columns of its rows,
    f_rest columns of its own degree), its records, and its own grid.  A record whose bucket index lies
    past the centre table points at an extra all-NaN centre (the reader reads `undefined` there)."""
    mode, secs = ksplat_sections(data)
    lo_h, hi_h = struct.unpack_from('<ff', data, 36)
    row = 0
    out = []
    for si, s in enumerate(secs):
        h = 4096 + 1024 * si
        count = s['count']
        if not count:
            continue
        capacity, nbuckets = struct.unpack_from('<II', data, h + 8)
        block = struct.unpack_from('<f', data, h + 16)[0]
        quant = struct.unpack_from('<I', data, h + 24)[0] or DEFAULT_QUANT[mode]
        full = struct.unpack_from('<I', data, h + 32)[0]
        sizes = np.frombuffer(data, '<u4', s['partial'], s['start'])
        centres = np.frombuffer(data, '<f4', 3 * nbuckets, s['start'] + 4 * s['partial']).reshape(nbuckets, 3)
        bucket = np.zeros(count, np.int64)
        current, base = full, full * capacity
        for r in range(count):  # read-ksplat.ts:251-269
            if r < full * capacity:
                bucket[r] = r // capacity
            else:
                j = current - full
                if j < len(sizes) and r >= base + int(sizes[j]):
                    current += 1
                    base += int(sizes[j])
                bucket[r] = current
        past = bucket >= nbuckets
        centres = np.vstack([centres, np.full((1, 3), np.nan, np.float32)])
        bucket = np.where(past, nbuckets, bucket)
        nsh = SH_COUNT[s['degree']]
        names = sh.reader_columns(nsh)
        table = [(k, np.ascontiguousarray(cols[i, row:row + count])) for i, k in enumerate(names)]
        rec = np.frombuffer(data, np.uint8, count * s['stride'], s['data_off']).reshape(count, s['stride'])
        # the reader's `|| default` on the header range (read-ksplat.ts:135-136)
        sh_min = -1.5 if (lo_h == 0 or lo_h != lo_h) else lo_h
        sh_max = 1.5 if (hi_h == 0 or hi_h != hi_h) else hi_h
        out.append(dict(mode=mode, degree=s['degree'], table=table, records=rec, bucket=bucket.astype(np.uint32),
                        centres=centres, block=block, quant=quant, sh_min=sh_min, sh_max=sh_max, past=past, row0=row))
        row += count
    return out


def half_value(h):
    return np.asarray(h, np.uint16).view(np.float16).astype(np.float64)


def is_snan32(w):
    w = np.asarray(w, np.uint32)
    return ((w & 0x7f800000) == 0x7f800000) & ((w & 0x007fffff) != 0) & ((w & 0x00400000) == 0)


def words(rec, off, count, width):
    return np.ascontiguousarray(rec[:, off:off + count * width]).view(f'<u{width}').reshape(len(rec), count)


def excused(sec):
    """{class name: bool [records, record bytes]} of the bytes a class excuses, from the file's bytes
    and header alone"""
    mode, rec = sec['mode'], sec['records']
    m, stride = rec.shape
    nsh = SH_COUNT[sec['degree']]
    cls = {k: np.zeros((m, stride), bool) for k in ('rotation', 'scale_lost', 'scale_log', 'half_nan', 'snan', 'ps',
                                                    'past_table', 'sh_range')}

    def mark(name, off, width, mask):  # mask [m, count]
        for j in range(mask.shape[1]):
            cls[name][:, off + j * width:off + (j + 1) * width] |= mask[:, j:j + 1]
    if mode == 0:
        cls['rotation'][:, 24:40] = True
        with np.errstate(invalid='ignore'):
            s = words(rec, 12, 3, 4).view(np.float32).astype(np.float64)
        mark('scale_lost', 12, 4, ~(s > 0) | np.isinf(s))
        mark('scale_log', 12, 4, (s > 0) & np.isfinite(s))
        mark('snan', 0, 4, is_snan32(words(rec, 0, 3, 4)))
        if nsh:
            mark('snan', 44, 4, is_snan32(words(rec, 44, nsh, 4)))
    else:
        cls['rotation'][:, 12:20] = True
        s = half_value(words(rec, 6, 3, 2))
        mark('scale_lost', 6, 2, ~(s > 0) | np.isinf(s))
        with np.errstate(all='ignore'):
            ps = np.float64(np.float32(sec['block'])) / 2.0 / float(sec['quant'])
        if not (np.isfinite(ps) and ps != 0):
            cls['ps'][:, 0:6] = True
        cls['past_table'][:, 0:6] |= sec['past'][:, None]
        if mode == 1 and nsh:
            mark('half_nan', 24, 2, np.isnan(half_value(words(rec, 24, nsh, 2))))
        if mode == 2 and nsh and not (np.isfinite(sec['sh_min']) and np.isfinite(sec['sh_max'])):
            cls['sh_range'][:, 24:] = True
    return cls


def restated(sec):
    return ref.records(sec['table'], sec['mode'], None, sec['bucket'], sec['centres'], -1, sec['block'], sec['quant'],
                       sec['sh_min'], sec['sh_max'])


# ---- tables whose plan is known by construction ----------------------------------------------------
def ordinary(rng, n, C, dtype=np.float32, spread=8.0):
    """a plain table of n rows in the readers' column order with 3C f_rest columns"""
    out = []
    for k in sh.reader_columns(3 * C):
        a = rng.normal(0, 1.5, n)
        a = a * spread if k in 'xyz' else a - 4 if k.startswith('scale') else a / 4 if k.startswith('f_rest') else a
        out.append((k, a.astype(dtype)))
    return out


def with_positions(n, x, y=None, z=None, C=0, seed=3):
    cols = dict(ordinary(np.random.default_rng(seed), n, C))
    cols['x'] = np.asarray(x, np.float32)
    cols['y'] = np.zeros(n, np.float32) if y is None else np.asarray(y, np.float32)
    cols['z'] = np.zeros(n, np.float32) if z is None else np.asarray(z, np.float32)
    return [(k, cols[k]) for k in sh.reader_columns(3 * C)]


def plan_tables():
    """{name: (columns, block, expected or None)}; expected = (F, P, partial sizes, clamped)"""
    t = {}
    for m in (1, 255, 256, 257, 513):
        t[f'one_cell_{m}'] = (with_positions(m, np.linspace(0, 1, m)), 5.0,
                              (m // 256, 1 if m % 256 else 0, [m % 256] if m % 256 else [], 0))
    # two cells of 300 and 212 rows, interleaved in the input: full buckets of both before the partials
    x = np.where(np.arange(512) % 512 < 300, 1.0, 7.0)
    t['two_cells'] = (with_positions(512, np.random.default_rng(5).permutation(x)), 5.0, (1, 2, [44, 212], 0))
    # rows in reverse key order: the sort must move all of them and keep equal keys in row order
    t['reverse'] = (with_positions(600, np.repeat(np.arange(6)[::-1] * 5.0 + 1, 100)), 5.0, (0, 6, [100] * 6, 0))
    t['axis_without_finite'] = (with_positions(40, np.linspace(0, 30, 40), y=np.full(40, np.nan),
                                               z=np.resize([np.inf, -np.inf], 40)), 5.0, None)
    sp = np.array([np.nan, np.inf, -np.inf, 1e30, 0, 1, 2, 3] * 5, np.float32)
    t['specials'] = (with_positions(40, sp, y=sp[::-1].copy(), z=np.linspace(-3, 3, 40)), 5.0, None)
    t['one_point'] = (with_positions(700, np.full(700, 2.5), y=np.full(700, -1.0), z=np.full(700, 9.0)), 5.0,
                      (2, 1, [188], 0))
    return t


def image_table(n, C, seed=11, dtype=np.float32):
    """several cells at block size 5: positions are >= 0 with the last row at the origin, so cell 0 is
    [0, 5)^3.  From 257 rows on, cell 0 holds 257 rows (300 from 513 on) -- more than one bucket -- and
    the other rows lie outside it (at n = 257 there are no others)"""
    rng = np.random.default_rng(seed + n + 100 * C)
    cols = dict(ordinary(rng, n, C, dtype, spread=6.0))
    inside = 0 if n < 257 else 300 if n >= 513 else 257
    for k in 'xyz':
        a = np.abs(cols[k].astype(np.float64))
        if inside:
            a[:inside - 1] = rng.uniform(0.1, 4.9, inside - 1)
            a[inside - 1:] += 5.0
        a[n - 1] = 0.0
        cols[k] = a.astype(dtype)
    return [(k, cols[k]) for k in sh.reader_columns(3 * C)]
