'use strict';
// Node host: processDataTable with filterClusters (st_abi.h, "clusters"), alone
// and in a chain, on a table the Python test wrote.
//   node cluster_actions.js <dir>
// <dir>/manifest.json: { columns: [{ name, dtype, offset, nbytes }], cases: [{ name, actions }] } over
// <dir>/in.bin.  Per case the processed columns go back to back into <dir>/out_<name>.bin; stdout is
// one JSON object { <name>: { names, rows } }.
const fs = require('fs');
const path = require('path');

const host = require(path.join(__dirname, '..', '..', 'splat-transform_amd', 'js'));

const CTOR = { f4: Float32Array, f8: Float64Array, u4: Uint32Array, i4: Int32Array, u1: Uint8Array, i1: Int8Array,
    u2: Uint16Array, i2: Int16Array };
const dir = process.argv[2];
const man = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json'), 'utf8'));
const blob = fs.readFileSync(path.join(dir, 'in.bin'));
const column = (c) => {
    const ctor = CTOR[c.dtype];
    const copy = Buffer.from(blob.subarray(c.offset, c.offset + c.nbytes));
    return new host.Column(c.name, new ctor(copy.buffer, copy.byteOffset, c.nbytes / ctor.BYTES_PER_ELEMENT));
};

const out = {};
for (const c of man.cases) {
    const res = host.processDataTable(new host.DataTable(man.columns.map(column)), c.actions);
    const parts = res.columns.map(col => Buffer.from(col.data.buffer, col.data.byteOffset, col.data.byteLength));
    fs.writeFileSync(path.join(dir, `out_${c.name}.bin`), Buffer.concat(parts));
    out[c.name] = { names: res.columns.map(col => col.name), rows: res.columns.length ? res.columns[0].data.length : 0 };
}
console.log(JSON.stringify(out));
