#!/usr/bin/env python3
"""Stage the reference's CSV writer next to the other modules.

TEST INFRASTRUCTURE ONLY.  build_ref.py with one more file (writers/write-csv); the result
goes to $ST_REF_JS (default /tmp/st_ref_js) and is never committed -- only the vectors
make_golden_write_csv.js records from running it are (tests/golden/write_csv.*).
"""
import build_ref

build_ref.FILES += ['writers/write-csv']

if __name__ == '__main__':
    build_ref.main()
