"""writeCsv (writers/write-csv.ts:5-23) restated: the header line, then per row the cells
'' + column[i] joined by ',' and a '\\n'.

A cell is ECMA-262 Number::toString (radix 10) of the element read as a JS number: an integer
column's plain decimal, a float32 widened exactly to a double first, NaN / Infinity / -Infinity,
0 for both zeros.  The digits of a finite double come from Python's repr(float), which is -- like
V8's -- the shortest string that rounds back, the closest among those; the layout rules (fixed up
to 21 digits, leading zeros down to 1e-6, exponent form outside) are applied here.  Pinned to the
reference's own files by tests/golden/write_csv.* (test_write_csv_cpu.py).
"""
import math

import numpy as np

MAX_CELL = {'i1': 4, 'u1': 3, 'i2': 6, 'u2': 5, 'i4': 11, 'u4': 10, 'f4': 25, 'f8': 25}


def js_number(v):
    """Number::toString of a Python int or float (a float32 is widened by float(np.float32))"""
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    v = float(v)
    if math.isnan(v):
        return 'NaN'
    if math.isinf(v):
        return 'Infinity' if v > 0 else '-Infinity'
    if v == 0:
        return '0'
    sign = '-' if v < 0 else ''
    r = repr(abs(v))
    mant, _, exp = r.partition('e')
    ip, _, fp = mant.partition('.')
    digits = ip + fp
    n = len(ip) + (int(exp) if exp else 0)   # value = 0.digits x 10^n before the strip
    lead = len(digits) - len(digits.lstrip('0'))
    digits = digits.lstrip('0')
    n -= lead
    digits = digits.rstrip('0')
    k = len(digits)
    if k <= n <= 21:
        return sign + digits + '0' * (n - k)
    if 0 < n <= 21:
        return sign + digits[:n] + '.' + digits[n:]
    if -6 < n <= 0:
        return sign + '0.' + '0' * -n + digits
    e = n - 1
    return sign + digits[0] + ('.' + digits[1:] if k > 1 else '') + 'e' + ('+' if e >= 0 else '-') + str(abs(e))


def column_text(a):
    """the cells of one numpy column: list of str"""
    a = np.asarray(a)
    if a.dtype.kind in 'iu':
        return [str(v) for v in a.tolist()]
    with np.errstate(invalid='ignore'):   # (a signalling NaN's widening)
        wide = a.astype(np.float64)
    return [js_number(v) for v in wide.tolist()]


def header(names):
    return (','.join(names) + '\n').encode('utf-8')


def rows(cols, row0=0, nrows=None):
    """the rows' bytes of [(name, numpy array)]"""
    if not cols:
        return b''
    end = len(cols[0][1]) if nrows is None else row0 + nrows
    texts = [column_text(a[row0:end]) for _, a in cols]
    return ''.join(','.join(cells) + '\n' for cells in zip(*texts)).encode('ascii')


def write_csv(cols):
    return header([k for k, _ in cols]) + rows(cols)
