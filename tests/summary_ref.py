"""The column summary of include/st_abi.h ("column summary") restated in plain Python, for
tests/test_summary_cpu.py and tests/test_summary_gpu.py.  Nothing here shares a line with the code
under test: elements become Python floats (every one of the eight types widens exactly), d_i and t_i
are Python float operations, the exact sums are fractions.Fraction over integer numerators in units
of 2^-1074 (float(Fraction) rounds correctly; its OverflowError is a signed infinity), and the
median comes from a sort under the total order in which -0 precedes +0."""
import collections
import math
from fractions import Fraction

import numpy as np

import write_csv_ref as wc

FIELDS = ('rows', 'nan_count', 'inf_count', 'min', 'max', 'sum', 'mean', 'ssd', 'std_dev', 'median')
Summary = collections.namedtuple('Summary', FIELDS)
_UNIT = 1 << 1074


def exact_sum(values):
    """the real-number sum of finite Python floats, rounded once"""
    total = 0
    for v in values:
        num, den = v.as_integer_ratio()  # den is a power of two, at most 2^1074
        total += num << (1074 - (den.bit_length() - 1))
    try:
        return float(Fraction(total, _UNIT))
    except OverflowError:
        return math.inf if total > 0 else -math.inf


def total_order(values):
    """finite floats sorted with -0 before +0"""
    v = np.asarray(values, np.float64)
    return v[np.lexsort((~np.signbit(v), v))].tolist()


def summarize(column):
    """Summary of one numpy column of any of the eight types"""
    with np.errstate(invalid='ignore'):  # (a signalling NaN's widening)
        vals = np.asarray(column).astype(np.float64)
    n = len(vals)
    nan = int(np.isnan(vals).sum())
    inf = int(np.isinf(vals).sum())
    fin = total_order(vals[np.isfinite(vals)])
    m = len(fin)
    assert m == n - nan - inf
    if m == 0:
        return Summary(n, nan, inf, math.nan, math.nan, 0.0, math.nan, 0.0, math.nan, math.nan)
    s = exact_sum(fin)
    mean = s / float(m)
    ts = []
    for v in fin:
        d = v - mean
        ts.append(d * d)
    ssd = math.inf if any(math.isinf(t) for t in ts) else exact_sum(ts)
    std = math.sqrt(ssd / float(m))
    median = fin[(m - 1) // 2] if m % 2 else (fin[m // 2 - 1] + fin[m // 2]) / 2
    return Summary(n, nan, inf, fin[0], fin[-1], s, mean, ssd, std, median)


def fast_path(column):
    """whether the column's sum fits the int128 fast path: every finite non-zero element's set bits lie
    between 2^lo and 2^hi, and hi - lo + 1 plus the bit length of m is at most 126"""
    with np.errstate(invalid='ignore'):
        vals = np.asarray(column).astype(np.float64)
    fin = vals[np.isfinite(vals)]
    lo, hi = None, None
    for v in fin[fin != 0].tolist():
        num, den = abs(v).as_integer_ratio()
        low = (num & -num).bit_length() - den.bit_length()
        high = num.bit_length() - den.bit_length()
        lo = low if lo is None else min(lo, low)
        hi = high if hi is None else max(hi, high)
    return lo is None or hi - lo + 1 + len(fin).bit_length() <= 126


def bits(x):
    return int(np.float64(x).view(np.uint64))


def same(got, want):
    """field by field: counts equal; doubles as bit patterns (the sign of zero counts), NaN as NaN"""
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        if f in ('rows', 'nan_count', 'inf_count'):
            if int(a) != int(b):
                return f'{f}: {a} != {b}'
        elif math.isnan(b):
            if not math.isnan(a):
                return f'{f}: {a!r} is not NaN'
        elif bits(a) != bits(b):
            return f'{f}: {a!r} ({bits(a):#x}) != {b!r} ({bits(b):#x})'
    return None


def text(names, summaries):
    """st_summary_text's bytes: the number text is write_csv_ref's (JavaScript's Number::toString)"""
    out = 'column,rows,nanCount,infCount,min,max,mean,stdDev,median\n'
    for name, s in zip(names, summaries):
        cells = [name, str(s.rows), str(s.nan_count), str(s.inf_count)]
        cells += [wc.js_number(float(v)) for v in (s.min, s.max, s.mean, s.std_dev, s.median)]
        out += ','.join(cells) + '\n'
    return out.encode()
