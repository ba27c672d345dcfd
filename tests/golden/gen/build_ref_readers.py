#!/usr/bin/env python3
"""Stage the reference's .splat / .ksplat / .spz readers next to the other modules.

TEST INFRASTRUCTURE ONLY.  build_ref.py with three more files (readers/read-splat,
readers/read-ksplat, readers/read-spz); the result goes to $ST_REF_JS (default
/tmp/st_ref_js) and is never committed -- only the vectors make_golden_readers.js
records from running it are (tests/golden/readers.*).

One pre-pass before the type eraser: strip_ts.py erases the annotation of the first
declarator of a `let` only, so `let x: number, y: number, z: number;` would come out
as `let x, y: number, z: number;`.  Lines of exactly that form (every declarator a
bare name with a one-word type, no initialiser) lose their annotations here.
"""
import re

import build_ref

build_ref.FILES += ['readers/read-splat', 'readers/read-ksplat', 'readers/read-spz']

_MULTI_LET = re.compile(r'^(\s*let\s+)(\w+\s*:\s*\w+(?:\s*,\s*\w+\s*:\s*\w+)+)(\s*;\s*)$', re.M)


def plain_multi_let(src):
    return _MULTI_LET.sub(lambda m: m.group(1) + re.sub(r'\s*:\s*\w+', '', m.group(2)) + m.group(3), src)


_strip = build_ref.strip
build_ref.strip = lambda src: _strip(plain_multi_let(src))

if __name__ == '__main__':
    build_ref.main()
