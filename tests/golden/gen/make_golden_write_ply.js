'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/write_ply.{json,bin}.
//
// Runs the reference's writePly (type-erased into $ST_REF_JS by build_ref_writers.py, never
// committed) on seeded tables built here, into a scratch file, and records every input column
// and the bytes of the file it wrote.
//
//   python3 tests/golden/gen/build_ref_writers.py && node tests/golden/gen/make_golden_write_ply.js
//
// Reference call site exercised: writers/write-ply.ts:5-68 (through data-table.ts's Column / DataTable).

const fs = require('fs');
const os = require('os');
const path = require('path');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const OUT = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');

const { Column, DataTable } = require(path.join(REF, 'data-table.js'));
const { writePly } = require(path.join(REF, 'writers/write-ply.js'));

const mulberry32 = (seed) => {
    let a = seed >>> 0;
    return () => {
        a = (a + 0x6D2B79F5) >>> 0;
        let t = a;
        t = Math.imul(t ^ (t >>> 15), t | 1);
        t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
        return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
    };
};

const DTYPES = {
    Int8Array: 'i1', Uint8Array: 'u1', Int16Array: 'i2', Uint16Array: 'u2',
    Int32Array: 'i4', Uint32Array: 'u4', Float32Array: 'f4', Float64Array: 'f8'
};

class Fixture {
    constructor(name) { this.name = name; this.arrays = {}; this.chunks = []; this.offset = 0; this.meta = {}; }
    add(key, arr) {
        const dtype = DTYPES[arr.constructor.name];
        if (!dtype) throw new Error(`bad array type for ${key}`);
        const buf = Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength);
        const pad = (8 - (this.offset % 8)) % 8;
        if (pad) { this.chunks.push(Buffer.alloc(pad)); this.offset += pad; }
        this.arrays[key] = { dtype, shape: [arr.length], offset: this.offset, nbytes: buf.length };
        this.chunks.push(Buffer.from(buf));
        this.offset += buf.length;
    }
    save() {
        fs.writeFileSync(path.join(OUT, `${this.name}.bin`), Buffer.concat(this.chunks));
        fs.writeFileSync(path.join(OUT, `${this.name}.json`), JSON.stringify({
            generator: 'tests/golden/gen/make_golden_write_ply.js (reference modules type-erased by build_ref_writers.py)',
            reference: '@playcanvas/splat-transform 0.10.1 @ /root/reference',
            meta: this.meta,
            arrays: this.arrays
        }, null, 1));
        process.stderr.write(`  ${this.name}: ${Object.keys(this.arrays).length} arrays, ${(this.offset / 1024).toFixed(1)} KiB\n`);
    }
}

// a column of n seeded values of the array type: floats bell-shaped, integers over their whole range
const fill = (Type, n, u) => {
    const a = new Type(n);
    const bytes = new Uint8Array(a.buffer);
    if (Type === Float32Array || Type === Float64Array) {
        for (let i = 0; i < n; ++i) a[i] = (u() + u() + u() + u() - 2) * 3;
    } else {
        for (let i = 0; i < bytes.length; ++i) bytes[i] = Math.floor(u() * 256);
    }
    return a;
};

const gsNames = (coeffs) => ['x', 'y', 'z', 'nx', 'ny', 'nz', 'f_dc_0', 'f_dc_1', 'f_dc_2']
    .concat(Array.from({ length: 3 * coeffs }, (_, i) => `f_rest_${i}`))
    .concat(['opacity', 'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3']);

const floats = names => names.map(nm => [nm, Float32Array]);

// name -> { comments, elements: [[element name, rows, [[column, type]]]] }
const CASES = {
    // no rows at all
    empty: { comments: ['nothing here'], elements: [['vertex', 0, floats(['x', 'y', 'z'])]] },
    // the CLI's shape (index.ts:126-133): no comments, one element named vertex
    cli: { comments: [], elements: [['vertex', 64, floats(gsNames(0))]] },
    // an SH-1 float table
    sh1: { comments: ['first comment', 'second'], elements: [['vertex', 300, floats(gsNames(3))]] },
    // 11-byte rows with the double at offset 1; one row more than writePly's 1024-row chunk
    uds: { comments: ['odd rows'], elements: [['odd', 1025, [['a', Uint8Array], ['b', Float64Array], ['c', Int16Array]]]] },
    // every type name
    types8: {
        comments: [],
        elements: [['vertex', 3, [['c', Int8Array], ['uc', Uint8Array], ['s', Int16Array], ['us', Uint16Array],
            ['i', Int32Array], ['ui', Uint32Array], ['f', Float32Array], ['d', Float64Array]]]]
    },
    // an element without columns (rows of 0 bytes) before one with
    nocols: { comments: ['c'], elements: [['bare', 5, []], ['vertex', 2, [['x', Float32Array], ['k', Uint8Array]]]] }
};

const main = async () => {
    const fx = new Fixture('write_ply');
    const tmp = path.join(os.tmpdir(), `st_write_ply_${process.pid}.ply`);
    let seed = 7100;
    for (const [name, spec] of Object.entries(CASES)) {
        const u = mulberry32(seed++);
        const elements = spec.elements.map(([elName, rows, cols]) => {
            const columns = cols.map(([nm, Type]) => new Column(nm, fill(Type, rows, u)));
            // (DataTable refuses an empty column list: the reference's PlyData only needs these two members)
            const dataTable = columns.length ? new DataTable(columns) : { numRows: rows, columns: [] };
            return { name: elName, dataTable };
        });
        const fh = await fs.promises.open(tmp, 'w');
        try {
            await writePly(fh, { comments: spec.comments, elements });
        } finally {
            await fh.close();
        }
        const file = fs.readFileSync(tmp);
        fs.unlinkSync(tmp);
        fx.add(`${name}_file`, new Uint8Array(file.buffer, file.byteOffset, file.length));
        const end = file.indexOf('end_header\n') + 11;
        fx.meta[name] = {
            comments: spec.comments,
            header_bytes: end,
            elements: elements.map(e => ({
                name: e.name,
                rows: e.dataTable.numRows,
                columns: e.dataTable.columns.map(c => ({ name: c.name, dtype: DTYPES[c.data.constructor.name] }))
            }))
        };
        for (const e of elements) for (const c of e.dataTable.columns) fx.add(`${name}_${e.name}_${c.name}`, c.data);
    }
    fx.save();
};

main().catch((e) => { console.error(e); process.exit(1); });
