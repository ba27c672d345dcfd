'use strict';
// The reference's writeCsv under Node on this host's CPU, for scale (indicative: one machine,
// one run; the page cache takes the file).  Needs the reference's modules staged by
// tests/golden/gen/build_ref_csv.py ($ST_REF_JS, default /tmp/st_ref_js).
//
//   node tools/bench_node_csv.js [rows] [columns]
const fs = require('fs');
const os = require('os');
const path = require('path');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const { Column, DataTable } = require(path.join(REF, 'data-table.js'));
const { writeCsv } = require(path.join(REF, 'writers/write-csv.js'));

const rows = parseInt(process.argv[2] || '100000', 10);
const ncol = parseInt(process.argv[3] || '14', 10);

let a = 12345;
const u = () => {
    a = (a + 0x6D2B79F5) >>> 0;
    let t = a;
    t = Math.imul(t ^ (t >>> 15), t | 1);
    t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
    return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
};

const main = async () => {
    const cols = [];
    for (let c = 0; c < ncol; ++c) {
        const d = new Float32Array(rows);
        for (let i = 0; i < rows; ++i) d[i] = (u() + u() + u() + u() - 2) * 3;
        cols.push(new Column(`c${c}`, d));
    }
    const table = new DataTable(cols);
    const tmp = path.join(os.tmpdir(), `st_bench_${process.pid}.csv`);
    const times = [];
    let size = 0;
    for (let r = 0; r < 3; ++r) {
        const fh = await fs.promises.open(tmp, 'w');
        const t0 = process.hrtime.bigint();
        await writeCsv(fh, table);
        await fh.close();
        times.push(Number(process.hrtime.bigint() - t0) / 1e6);
        size = fs.statSync(tmp).size;
        fs.unlinkSync(tmp);
    }
    times.sort((x, y) => x - y);
    console.log(JSON.stringify({ node: process.version, rows, columns: ncol, file_bytes: size, median_ms: times[1],
        min_ms: times[0], max_ms: times[2], MBps: size / times[1] / 1e3 }));
};

main().catch((e) => { console.error(e); process.exit(1); });
