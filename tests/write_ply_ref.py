"""numpy restatement of the reference's writePly (writers/write-ply.ts:5-68), the expectation of the
PLY writer tests.  tests/test_write_ply_cpu.py checks it against the reference's own output
(tests/golden/write_ply.*)."""
import numpy as np

PLY_NAMES = {'i1': 'char', 'u1': 'uchar', 'i2': 'short', 'u2': 'ushort', 'i4': 'int', 'u4': 'uint', 'f4': 'float',
             'f8': 'double'}


def code(a):
    dt = a.dtype if isinstance(a, np.ndarray) else np.dtype(a)
    return dt.kind + str(dt.itemsize)


def element_text(name, n, schema):
    """schema: [(column name, dtype or array)]"""
    return f'element {name} {n}\n' + ''.join(f'property {PLY_NAMES[code(a)]} {k}\n' for k, a in schema)


def header(comments, elements):
    """elements: [(element name, rows, schema)]"""
    return ('ply\nformat binary_little_endian 1.0\n' + ''.join(f'comment {c}\n' for c in comments) +
            ''.join(element_text(*e) for e in elements) + 'end_header\n').encode()


def rows(cols, n=None):
    """cols: [(name, numpy column)] -> the rows' bytes: each row its columns' elements back to back"""
    if not cols:
        return b''
    n = len(cols[0][1]) if n is None else n
    rec = np.zeros(n, np.dtype({'names': [f'c{i}' for i in range(len(cols))],
                                'formats': ['<' + code(a) for _, a in cols],
                                'offsets': np.cumsum([0] + [a.dtype.itemsize for _, a in cols])[:-1].tolist(),
                                'itemsize': sum(a.dtype.itemsize for _, a in cols)}))
    for i, (_, a) in enumerate(cols):
        rec[f'c{i}'] = a
    return rec.tobytes()


def write_ply(comments, elements):
    """elements: [(element name, [(column name, numpy column)])] or (name, cols, rows) for an element
    without columns -> the file's bytes"""
    els = [(e[0], e[1], e[2] if len(e) > 2 else len(e[1][0][1])) for e in elements]
    return header(comments, [(nm, n, cols) for nm, cols, n in els]) + b''.join(rows(cols, n) for nm, cols, n in els)
