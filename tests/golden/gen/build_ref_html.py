#!/usr/bin/env python3
"""Stage the reference's HTML viewer writer next to the other modules.

TEST INFRASTRUCTURE ONLY.  build_ref.py with one more file (writers/write-html); the result
goes to $ST_REF_JS (default /tmp/st_ref_js) and is never committed -- only the vectors
make_golden_write_html.js records from running it are (tests/golden/write_html.*).  The module's
import of '@playcanvas/supersplat-viewer' stays a bare require: make_golden_write_html.js puts a
stand-in of that name into the staging directory's node_modules.
"""
import build_ref

build_ref.FILES += ['writers/write-html']

if __name__ == '__main__':
    build_ref.main()
