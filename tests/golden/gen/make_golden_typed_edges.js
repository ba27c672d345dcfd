'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/typed_edges.{json,bin}.
//
// Runs the reference's own transform() and generateOrdering (type-erased into $ST_REF_JS by
// build_ref.py, never committed) on small tables whose columns are NOT all Float32Arrays, built
// here so that every TypedArray store edge is met: negative fractions, wraps at both ends of
// every integer type, NaN / +Inf / -Inf results, and numbers of 2^63 and above that are not a
// multiple of 2^32.  Records every input column, every column after each set of transform()
// calls, the (t, r, s) of every call, and per table how many stored values met each edge.
//
//   python3 tests/golden/gen/build_ref.py && node tests/golden/gen/make_golden_typed_edges.js
//
// Reference call sites exercised: transform.ts:12-65 (getRow / setRow of data-table.ts:63-76),
// ordering.ts:4-110.
//
// How an edge is recognised: before each transform() call the table is copied into a shadow whose
// columns are all Float64Arrays holding the same numbers; the same call on the shadow keeps the
// JS number that setRow was handed, and that number is classified against the column's type.

const fs = require('fs');
const path = require('path');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const OUT = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');

const { Column, DataTable } = require(path.join(REF, 'data-table.js'));
const { transform } = require(path.join(REF, 'transform.js'));
const { generateOrdering } = require(path.join(REF, 'ordering.js'));
const pc = require(path.join(REF, '__stubs/playcanvas.js'));

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

const TYPES = {
    int8: { ctor: Int8Array, dtype: 'i1', min: -128, max: 127, bits: 7 },
    uint8: { ctor: Uint8Array, dtype: 'u1', min: 0, max: 255, bits: 8 },
    int16: { ctor: Int16Array, dtype: 'i2', min: -32768, max: 32767, bits: 15 },
    uint16: { ctor: Uint16Array, dtype: 'u2', min: 0, max: 65535, bits: 16 },
    int32: { ctor: Int32Array, dtype: 'i4', min: -2147483648, max: 2147483647, bits: 31 },
    uint32: { ctor: Uint32Array, dtype: 'u4', min: 0, max: 4294967295, bits: 32 },
    float32: { ctor: Float32Array, dtype: 'f4' },
    float64: { ctor: Float64Array, dtype: 'f8' }
};
const typeOf = arr => Object.keys(TYPES).find(k => TYPES[k].ctor === arr.constructor);

class Fixture {
    constructor(name) { this.name = name; this.arrays = {}; this.chunks = []; this.offset = 0; this.meta = {}; }
    add(key, arr, shape) {
        const dtype = TYPES[typeOf(arr)].dtype;
        const buf = Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength);
        const pad = (8 - (this.offset % 8)) % 8;
        if (pad) { this.chunks.push(Buffer.alloc(pad)); this.offset += pad; }
        this.arrays[key] = { dtype, shape: shape || [arr.length], offset: this.offset, nbytes: buf.length };
        this.chunks.push(Buffer.from(buf));
        this.offset += buf.length;
    }
    save() {
        fs.writeFileSync(path.join(OUT, `${this.name}.bin`), Buffer.concat(this.chunks));
        fs.writeFileSync(path.join(OUT, `${this.name}.json`), JSON.stringify({
            generator: 'tests/golden/gen/make_golden_typed_edges.js (reference modules type-erased by build_ref.py)',
            reference: '@playcanvas/splat-transform 0.10.1',
            meta: this.meta,
            arrays: this.arrays
        }, null, 1));
        process.stderr.write(`  ${this.name}: ${Object.keys(this.arrays).length} arrays, ${(this.offset / 1024).toFixed(1)} KiB\n`);
    }
}

// ---------------------------------------------------------------------------
// transform() calls: (t, r, s) as processDataTable builds them (process.ts:71-83), or all three
const V = (x, y, z) => new pc.Vec3(x, y, z);
const rotate = (x, y, z) => ({ t: pc.Vec3.ZERO, r: new pc.Quat().setFromEulerAngles(x, y, z), s: 1 });
const translate = (x, y, z) => ({ t: V(x, y, z), r: pc.Quat.IDENTITY, s: 1 });
const scale = s => ({ t: pc.Vec3.ZERO, r: pc.Quat.IDENTITY, s });

const ROWS = 128;
const POS = ['x', 'y', 'z'];
const ROT = ['rot_0', 'rot_1', 'rot_2', 'rot_3'];
const SCL = ['scale_0', 'scale_1', 'scale_2'];
const rest = C => new Array(3 * C).fill('').map((_, i) => `f_rest_${i}`);
const groupOf = nm => (POS.includes(nm) ? 'pos' : ROT.includes(nm) ? 'rot' : SCL.includes(nm) ? 'scale' : 'sh');

// the value of column `nm`, row i, for a column of type `type`
const fill = (u, nm, type, i) => {
    const T = TYPES[type];
    const g = groupOf(nm);
    const signed = T.min < 0;
    if (T.min === undefined) {
        // floats: numbers a float32 cannot hold in the float64 columns, specials in the first rows
        const wide = (u() + u() + u() + u() - 2);
        const v = g === 'pos' ? wide * 7 : g === 'rot' ? wide : g === 'scale' ? -7 + 5 * u() : wide * 0.2;
        const k = (i * 7 + nm.length + nm.charCodeAt(nm.length - 1)) % 29;
        if (i < 40) {
            if (k === 0) return NaN;
            if (k === 1) return Infinity;
            if (k === 2) return -Infinity;
            if (k === 3) return -0;
            if (k === 4) return 0;
            if (g === 'scale' && k === 5) return 800;    // exp overflows
            if (g === 'scale' && k === 6) return -800;   // exp underflows to 0: log(0)
            if (g === 'sh' && k === 5) return 1e39;      // Infinity once in shCoeffs (float64 columns)
            if (g === 'sh' && k === 6) return 1e-46;     // 0 once in shCoeffs
        }
        return v;
    }
    if (g === 'pos') {
        // the ends of the type in the first rows, then the whole range
        const j = POS.indexOf(nm);
        if (i < 8) return [[T.max, 0, T.min], [T.max - 1, 1, signed ? T.min + 1 : 0], [0, 0, 0], [1, 0, 1],
            [signed ? -1 : 2, 1, 0], [T.max, T.max, T.max], [T.min, T.min, T.min], [2, 3, 1]][i][j];
        return Math.floor(T.min + u() * (T.max - T.min + 1));
    }
    if (g === 'rot') {
        if (i % 16 === 3) return 0;  // all-zero quaternions
        return signed ? Math.floor(u() * 7) - 3 : Math.floor(u() * 4);
    }
    if (g === 'scale') {
        if (i % 8 === 5) return Math.min(T.max, 1000);  // exp(1000) overflows where the type holds it
        return signed ? Math.floor(u() * 9) - 6 : Math.floor(u() * 4);
    }
    return signed ? Math.floor(u() * 5) - 2 : Math.floor(u() * 3);
};

const makeTable = (seed, names, typeFor) => {
    const u = mulberry32(seed);
    return new DataTable(names.map((nm) => {
        const type = typeFor(nm);
        const data = new TYPES[type].ctor(ROWS);
        for (let i = 0; i < ROWS; ++i) data[i] = fill(u, nm, type, i);
        return new Column(nm, data);
    }));
};

const cloneTable = t => new DataTable(t.columns.map(c => c.clone()));
const shadowOf = t => new DataTable(t.columns.map(c => new Column(c.name, Float64Array.from(c.data))));

const KINDS = ['frac_to_zero', 'frac_trunc', 'wrap_high', 'wrap_low', 'nan', 'pinf', 'ninf', 'fmod'];
const TWO63 = 9223372036854775808, TWO84 = 19342813113834066795298816, TWO32 = 4294967296;

// classify the number v that setRow stored into an integer column of type T
const classify = (v, T, counts) => {
    if (v !== v) { counts.nan++; return; }
    if (v === Infinity) { counts.pinf++; return; }
    if (v === -Infinity) { counts.ninf++; return; }
    const a = Math.abs(v), t = Math.trunc(v);
    if (a >= TWO63) {
        if (a < TWO84 && t % TWO32 !== 0) counts.fmod++;
        return;
    }
    if (v < 0 && v > -1) counts.frac_to_zero++;
    if (v < -1 && v !== t) counts.frac_trunc++;
    if (t > T.max) counts.wrap_high++;
    if (t < T.min) counts.wrap_low++;
};

const runSet = (table, calls, counts) => {
    for (const c of calls) {
        const shadow = shadowOf(table);
        transform(shadow, c.t, c.r, c.s);
        transform(table, c.t, c.r, c.s);
        table.columns.forEach((col, k) => {
            const T = TYPES[col.dataType];
            if (T.min === undefined) return;
            const sd = shadow.columns[k].data;
            for (let i = 0; i < sd.length; ++i) classify(sd[i], T, counts);
        });
    }
};

const trsArray = calls => Float64Array.from([].concat(...calls.map(c =>
    [c.t.x, c.t.y, c.t.z, c.r.x, c.r.y, c.r.z, c.r.w, c.s])));

// ---------------------------------------------------------------------------
const fx = new Fixture('typed_edges');
const tables = [];

const addCase = (name, seed, names, typeFor, sets) => {
    const input = makeTable(seed, names, typeFor);
    const info = { name, rows: ROWS, columns: names, types: input.columns.map(c => c.dataType), sets: Object.keys(sets), counts: {} };
    KINDS.forEach((k) => { info.counts[k] = 0; });
    input.columns.forEach((c) => { fx.add(`${name}_in_${c.name}`, c.data); });
    for (const set of Object.keys(sets)) {
        const t = cloneTable(input);
        runSet(t, sets[set], info.counts);
        fx.add(`${name}_${set}_trs`, trsArray(sets[set]), [sets[set].length, 8]);
        t.columns.forEach((c) => { fx.add(`${name}_${set}_${c.name}`, c.data); });
    }
    tables.push(info);
};

const ROTATE = rotate(10, 20, 30);
const FINITE_CHAIN = [ROTATE, translate(1.5, -0.9, -1.5), scale(1.75)];
const INF_CHAIN = [ROTATE, translate(Infinity, -Infinity, 0.25), scale(0)];
const names = C => POS.concat(ROT, SCL, rest(C));

// one table per type, every transformed column of that type, SH band 1
Object.keys(TYPES).forEach((type, k) => {
    const T = TYPES[type];
    // all three at once, scaled so that the type's largest positions land in [2^63, 2^84): the
    // tiny rotation mixes a second product in below 2^32 (one product of an 8-bit value and a
    // float32 matrix entry would be a multiple of 2^32 once it reaches 2^63)
    const big = T.bits ? Math.pow(2, 66 - T.bits) * (1 + Math.pow(2, -20)) : 1048577;
    addCase(`all_${type}`, 7100 + k, names(3), () => type, {
        rotate: [ROTATE],
        translate: [translate(1.5, -0.9, -1.5)],
        scale: [scale(-2.5)],    // log of a negative: NaN from operands that hold none
        chain: INF_CHAIN,
        trs: [{ t: V(0.5, 0, 0), r: new pc.Quat().setFromEulerAngles(0, 0, 1e-6), s: big }]
    });
});

// float64 at the other bands
[0, 8, 15].forEach((C, k) => {
    addCase(`f64_c${C}`, 7200 + k, names(C), () => 'float64', { chain: FINITE_CHAIN });
});

// every column group of at least two types
const cyc = (list, nm) => list[(nm.charCodeAt(nm.length - 1) + nm.length) % list.length];
addCase('mixed_a', 7301, names(3), nm => ({
    pos: cyc(['float64', 'int16', 'uint32'], nm), rot: cyc(['float64', 'float32', 'int8'], nm),
    scale: cyc(['int8', 'float64', 'uint16'], nm), sh: cyc(['float64', 'uint8', 'int8', 'float32'], nm)
}[groupOf(nm)]), { chain: FINITE_CHAIN, chain_inf: INF_CHAIN });
addCase('mixed_b', 7302, names(8), nm => ({
    pos: cyc(['int32', 'float64'], nm), rot: cyc(['int16', 'float64'], nm),
    scale: cyc(['float32', 'int32', 'float64'], nm), sh: cyc(['int16', 'float64', 'uint16'], nm)
}[groupOf(nm)]), { chain: FINITE_CHAIN, chain_inf: INF_CHAIN });

// one column of a group missing: transform() skips the group and leaves its other columns alone
const lacking = [['no_pos', 'y'], ['no_rot', 'rot_2'], ['no_scale', 'scale_0']];
lacking.forEach(([name, drop], k) => {
    addCase(name, 7400 + k, names(3).filter(nm => nm !== drop),
        nm => cyc(['float64', 'int16', 'float32'], nm), { chain: FINITE_CHAIN });
});
fx.meta.tables = tables;
fx.meta.kinds = KINDS;

// ---------------------------------------------------------------------------
// ordering: clumps whose members differ by less than a float32 can hold (1e-12 on values near 1),
// so the float64 keys sort inside a clump where the float32 casts are all equal
const ordering = [];
const addOrdering = (name, seed, n, ctors, gen) => {
    const u = mulberry32(seed);
    const data = ctors.map(C => new C(n));
    for (let i = 0; i < n; ++i) gen(u, i).forEach((v, a) => { data[a][i] = v; });
    const table = new DataTable(POS.map((nm, a) => new Column(nm, data[a])));
    POS.forEach((nm, a) => fx.add(`${name}_${nm}`, data[a]));
    const idx = new Uint32Array(n);
    for (let i = 0; i < n; ++i) idx[i] = i;
    fx.add(`${name}_order`, generateOrdering(table, idx));
    // an index list that repeats rows and leaves others out
    const sub = new Uint32Array(Math.floor(n * 0.7));
    for (let i = 0; i < sub.length; ++i) sub[i] = Math.floor(u() * n);
    fx.add(`${name}_sub`, sub.slice());
    fx.add(`${name}_sub_order`, generateOrdering(table, sub));
    ordering.push({ name, n, types: data.map(typeOf) });
};
const wide = u => (u() + u() + u() + u() - 2) * 6;
addOrdering('ord_f64', 7501, 3000, [Float64Array, Float64Array, Float64Array], (u, i) => {
    if (u() < 0.2) return [wide(u), wide(u), wide(u)];
    const c = Math.floor(u() * 5);  // five clumps of about 480 members
    return [1 + c * 0.125 + u() * 1e-12, 1 - c * 0.0625 + u() * 1e-12, 1 + u() * 1e-12];
});
addOrdering('ord_mixed', 7502, 3000, [Int16Array, Float64Array, Int32Array], (u, i) => {
    if (u() < 0.2) return [Math.floor(wide(u) * 100), wide(u), Math.floor(wide(u) * 1e5)];
    return [Math.floor(u() * 2), 1 + u() * 1e-12, 1000 * Math.floor(u() * 2)];
});
fx.meta.ordering = ordering;
fx.save();
