'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/write_csv.{json,bin}.
//
// Runs the reference's writeCsv (type-erased into $ST_REF_JS by build_ref_csv.py, never
// committed) on tables built here, into a scratch file, and records every input column and the
// bytes of the file it wrote.  The cells are therefore V8's own Number -> String conversions.
//
//   python3 tests/golden/gen/build_ref_csv.py && node tests/golden/gen/make_golden_write_csv.js
//
// Reference call site exercised: writers/write-csv.ts:5-23 (through data-table.ts's Column / DataTable).

const fs = require('fs');
const os = require('os');
const path = require('path');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const OUT = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');

const { Column, DataTable } = require(path.join(REF, 'data-table.js'));
const { writeCsv } = require(path.join(REF, 'writers/write-csv.js'));

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
            generator: 'tests/golden/gen/make_golden_write_csv.js (reference modules type-erased by build_ref_csv.py)',
            reference: '@playcanvas/splat-transform 0.10.1',
            meta: this.meta,
            arrays: this.arrays
        }, null, 1));
        process.stderr.write(`  ${this.name}: ${Object.keys(this.arrays).length} arrays, ${(this.offset / 1024).toFixed(1)} KiB\n`);
    }
}

const bell = (u) => (u() + u() + u() + u() - 2) * 3;
const rand32 = (u) => Math.floor(u() * 4294967296) >>> 0;

const bellColumn = (Type, n, u) => {
    const a = new Type(n);
    for (let i = 0; i < n; ++i) a[i] = bell(u);
    return a;
};

// an integer column over its whole range, its extremes and 0 first
const intColumn = (Type, n, u, lo, hi) => {
    const a = new Type(n);
    const bytes = new Uint8Array(a.buffer);
    for (let i = 0; i < bytes.length; ++i) bytes[i] = Math.floor(u() * 256);
    [lo, hi, 0, 1, -1, 10, 100, 1000, 100000, 1000000000].forEach((v, i) => { a[i] = v; });
    return a;
};

// every biased exponent with the mantissas 0, 1, all ones and two random ones, in both signs
const edges32 = (u) => {
    const bits = [];
    for (let e = 0; e < 256; ++e) {
        for (const m of [0, 1, 0x7fffff, rand32(u) & 0x7fffff, rand32(u) & 0x7fffff]) {
            for (const s of [0, 1]) bits.push(((s << 31) | (e << 23) | m) >>> 0);
        }
    }
    return new Float32Array(new Uint32Array(bits).buffer);
};

// every biased exponent with the mantissas 0, 1, all ones and three random ones (random sign), then
// the values around the layout's thresholds
const edges64 = (u) => {
    const words = [];  // (low, high) pairs
    for (let e = 0; e < 2048; ++e) {
        const ms = [[0, 0], [1, 0], [0xffffffff, 0xfffff]];
        for (let k = 0; k < 3; ++k) ms.push([rand32(u), rand32(u) & 0xfffff]);
        for (const [lo, hi] of ms) words.push(lo, (((u() < 0.5 ? 1 : 0) << 31) | (e << 20) | hi) >>> 0);
    }
    const head = new Float64Array(new Uint32Array(words).buffer);
    const next = (x, d) => {
        const f = new Float64Array([x]);
        const w = new BigUint64Array(f.buffer);
        w[0] += BigInt(d);
        return f[0];
    };
    const special = [];
    for (const x of [1e21, 1e-6, 1e-7, 1e20, 1e22, 1e-5, 1, 10, 0.1, 123456789012345680000]) {
        special.push(next(x, -1), x, next(x, 1), -x);
    }
    special.push(2 ** 53 - 1, 2 ** 53, 2 ** 53 + 2, -(2 ** 53) - 2, 5e-324, -5e-324, 1.7976931348623157e308,
        -1.7976931348623157e308, 2.2250738585072014e-308, 2.225073858507201e-308,
        -0.0000012345678901234567, 0.0000012345678901234567, 9007199254740993, 4294967296, 0.5, 0.25, 1 / 3,
        123456789, 1.5, 1e15, 1e16, 1e17, 12345678901234567890, 0, -0, Infinity, -Infinity, NaN);
    const a = new Float64Array(head.length + special.length);
    a.set(head, 0);
    a.set(special, head.length);
    return a;
};

const SH0 = ['x', 'y', 'z', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity', 'scale_0', 'scale_1', 'scale_2',
    'rot_0', 'rot_1', 'rot_2', 'rot_3'];

// name -> (u) => [[column name, typed array]]
const CASES = {
    // no rows: the header alone
    empty: () => ['x', 'y', 'z'].map(nm => [nm, new Float32Array(0)]),
    // the CLI's shape: 64 rows of the 14 SH-0 float columns
    cli: u => SH0.map(nm => [nm, bellColumn(Float32Array, 64, u)]),
    // one column of each type, the integer extremes among random values, floats bell-shaped
    types8: (u) => {
        const n = 300;
        const f = bellColumn(Float32Array, n, u), d = bellColumn(Float64Array, n, u);
        [3.4028234663852886e38, -3.4028234663852886e38, 1.401298464324817e-45, 0.1, 1e21, 16777216, -0, NaN, Infinity]
            .forEach((v, i) => { f[i] = v; });
        [1.7976931348623157e308, 5e-324, -1e21, 1e-7, 0.1, 4294967295, -2147483648, NaN, -Infinity]
            .forEach((v, i) => { d[i] = v; });
        return [['c', intColumn(Int8Array, n, u, -128, 127)], ['uc', intColumn(Uint8Array, n, u, 0, 255)],
            ['s', intColumn(Int16Array, n, u, -32768, 32767)], ['us', intColumn(Uint16Array, n, u, 0, 65535)],
            ['i', intColumn(Int32Array, n, u, -2147483648, 2147483647)],
            ['ui', intColumn(Uint32Array, n, u, 0, 4294967295)], ['f', f], ['d', d]];
    },
    edges32: u => [['v', edges32(u)]],
    edges64: u => [['v', edges64(u)]],
    // names are written raw
    names: u => [['a,b', bellColumn(Float32Array, 5, u)], ['say "hi"', intColumn(Uint8Array, 5, u, 0, 255)],
        ['two words', bellColumn(Float64Array, 5, u)], ['größe µ', intColumn(Int16Array, 5, u, -32768, 32767)]]
};

const main = async () => {
    const fx = new Fixture('write_csv');
    const tmp = path.join(os.tmpdir(), `st_write_csv_${process.pid}.csv`);
    let seed = 8100;
    for (const [name, make] of Object.entries(CASES)) {
        const cols = make(mulberry32(seed++));
        const dataTable = new DataTable(cols.map(([nm, data]) => new Column(nm, data)));
        const fh = await fs.promises.open(tmp, 'w');
        try {
            await writeCsv(fh, dataTable);
        } finally {
            await fh.close();
        }
        const file = fs.readFileSync(tmp);
        fs.unlinkSync(tmp);
        fx.add(`${name}_file`, new Uint8Array(file.buffer, file.byteOffset, file.length));
        fx.meta[name] = {
            rows: dataTable.numRows,
            columns: cols.map(([nm, data]) => ({ name: nm, dtype: DTYPES[data.constructor.name] }))
        };
        cols.forEach(([, data], i) => fx.add(`${name}_col${i}`, data));
    }
    fx.save();
};

main().catch((e) => { console.error(e); process.exit(1); });
