'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/readers.{json,bin}.
//
// Runs the reference's .splat / .ksplat / .spz readers (type-erased into $ST_REF_JS by
// build_ref_readers.py, never committed) on seeded input files built here and records the
// input bytes and every output column, and for the inputs the readers reject, the message
// of the error they throw.
//
//   python3 tests/golden/gen/build_ref_readers.py && node tests/golden/gen/make_golden_readers.js
//
// Reference call sites exercised:
//   readers/read-splat.ts:14-148   readers/read-ksplat.ts:29-60,103-384   readers/read-spz.ts:16-241
//
// read-spz.ts inflates through the web platform's Blob / DecompressionStream / Response, which
// Node 12 does not have: the three globals below stand in for them over zlib.gunzipSync (this
// file's own code; the reader itself runs unchanged).

const fs = require('fs');
const path = require('path');
const zlib = require('zlib');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const OUT = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');

global.Blob = class Blob {
    constructor(parts) { this.parts = parts.map(p => Buffer.from(p)); }
    stream() {
        const bytes = Buffer.concat(this.parts);
        return { pipeThrough: ds => ({ inflated: ds.inflate(bytes) }) };
    }
};
global.DecompressionStream = class DecompressionStream {
    constructor(format) { if (format !== 'gzip') throw new Error(`unsupported format ${format}`); }
    inflate(bytes) { return zlib.gunzipSync(bytes); }
};
global.Response = class Response {
    constructor(stream) { this.stream = stream; }
    async arrayBuffer() {
        const b = this.stream.inflated;
        return b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength);   // an ArrayBuffer of exactly the inflated size
    }
};

const { readSplat } = require(path.join(REF, 'readers/read-splat.js'));
const { readKsplat } = require(path.join(REF, 'readers/read-ksplat.js'));
const { readSpz } = require(path.join(REF, 'readers/read-spz.js'));
const READERS = { splat: readSplat, ksplat: readKsplat, spz: readSpz };

// ---------------------------------------------------------------------------
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

class Gen {
    constructor(seed) { this.u = mulberry32(seed); }
    int(n) { return Math.floor(this.u() * n); }
    bell(sigma) { return (this.u() + this.u() + this.u() + this.u() - 2) * sigma; }
    // half-float bits of an ordinary value: exponent field in [lo, hi]
    half(lo, hi, signed) { return ((signed && this.u() < 0.5) ? 0x8000 : 0) | ((lo + this.int(hi - lo + 1)) << 10) | this.int(1024); }
}

class Fixture {
    constructor(name, generator) {
        this.name = name; this.arrays = {}; this.chunks = []; this.offset = 0; this.meta = {};
        this.generator = generator || 'tests/golden/gen/make_golden_readers.js';
    }
    add(key, arr, shape) {
        const dtype = { Float32Array: 'f4', Uint8Array: 'u1' }[arr.constructor.name];
        if (!dtype) throw new Error(`bad array type for ${key}`);
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
            generator: `${this.generator} (reference modules type-erased by build_ref_readers.py)`,
            reference: '@playcanvas/splat-transform 0.10.1 @ /root/reference',
            meta: this.meta,
            arrays: this.arrays
        }, null, 1));
        process.stderr.write(`  ${this.name}: ${Object.keys(this.arrays).length} arrays, ${(this.offset / 1024).toFixed(1)} KiB\n`);
    }
}

// ---------------------------------------------------------------------------
// .splat: 32-byte rows  x y z (f32)  scale (3 f32)  r g b a  q0..q3 (u8)
const F32_SPECIAL_ROWS = [
    // scale bits x3, opacity byte, quaternion bytes
    { scale: [0x00000000, 0xbf800000, 0x80000000], op: 0, q: [127, 127, 127, 127] },       // 0, -1, -0
    { scale: [0x7f800000, 0x7fc00000, 0x00000007], op: 255, q: [128, 128, 128, 128] },     // Inf, NaN, subnormal
    { scale: [0xffc00000, 0x7f800001, 0xff800000], op: 1, q: [127, 128, 127, 128] },       // -NaN, sNaN, -Inf
    { scale: null, op: 254, q: [0, 0, 0, 0], pos: [0x7f800001, 0xff800000, 0x80000000] },  // sNaN, -Inf, -0 positions
    { scale: null, op: 128, q: [255, 255, 255, 255] },
    { scale: null, op: 127, q: [128, 127, 127, 127] }
];

const makeSplat = (n, seed) => {
    const g = new Gen(seed);
    const b = Buffer.alloc(n * 32);
    for (let i = 0; i < n; ++i) {
        const o = i * 32;
        for (let k = 0; k < 3; ++k) b.writeFloatLE(g.bell(4), o + 4 * k);
        for (let k = 0; k < 3; ++k) b.writeFloatLE(Math.exp(g.bell(2) - 3), o + 12 + 4 * k);
        for (let k = 24; k < 32; ++k) b[o + k] = g.int(256);
        const sp = F32_SPECIAL_ROWS[i];
        if (sp) {
            if (sp.scale) sp.scale.forEach((v, k) => b.writeUInt32LE(v, o + 12 + 4 * k));
            if (sp.pos) sp.pos.forEach((v, k) => b.writeUInt32LE(v, o + 4 * k));
            b[o + 27] = sp.op;
            sp.q.forEach((v, k) => { b[o + 28 + k] = v; });
        }
    }
    return b;
};

// ---------------------------------------------------------------------------
// .ksplat: 4096-byte main header, 1024 bytes per section header, then per section the partial
// bucket sizes (u32), the bucket centres (3 f32 per bucket) and maxSplats records
const KS_MODES = [
    { base: 44, scale: 12, rot: 24, color: 40, sh: 44, shBytes: 4 },
    { base: 24, scale: 6, rot: 12, color: 20, sh: 24, shBytes: 2 },
    { base: 24, scale: 6, rot: 12, color: 20, sh: 24, shBytes: 1 }
];
const SH_COUNT = [0, 9, 24, 45];
const HALF_SPECIALS = [0x0000, 0x8000, 0x0001, 0x03ff, 0x8001, 0x83ff, 0x0200, 0x7c00, 0xfc00, 0x7e00, 0x7c01, 0xfe00,
    0x0400, 0x7bff, 0x3c00, 0xbc00];
const F32_SPECIALS = [0x7f800001, 0xffc00000, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001, 0xbf800000];

// one record; `special` (a counter or null) picks special scale / rotation / SH encodings
const ksRecord = (g, mode, degree, special) => {
    const M = KS_MODES[mode], D = SH_COUNT[degree];
    const r = Buffer.alloc(M.base + D * M.shBytes);
    const sp = (k) => special !== null && ((special + k) % 3 === 0);
    if (mode === 0) {
        for (let k = 0; k < 3; ++k) r.writeFloatLE(g.bell(4), 4 * k);
        for (let k = 0; k < 3; ++k) {
            if (sp(k)) r.writeUInt32LE(F32_SPECIALS[(special + k) % F32_SPECIALS.length], M.scale + 4 * k);
            else r.writeFloatLE(Math.exp(g.bell(2) - 3), M.scale + 4 * k);
        }
        for (let k = 0; k < 4; ++k) {
            if (sp(k + 1)) r.writeUInt32LE(F32_SPECIALS[(special + k + 3) % F32_SPECIALS.length], M.rot + 4 * k);
            else r.writeFloatLE(g.bell(1), M.rot + 4 * k);
        }
        if (special !== null) r.writeUInt32LE(F32_SPECIALS[special % F32_SPECIALS.length], 4 * (special % 3));
        for (let k = 0; k < D; ++k) {
            if (sp(k + 2)) r.writeUInt32LE(F32_SPECIALS[(special + k) % F32_SPECIALS.length], M.sh + 4 * k);
            else r.writeFloatLE(g.bell(0.3), M.sh + 4 * k);
        }
    } else {
        for (let k = 0; k < 3; ++k) r.writeUInt16LE(special !== null && k === special % 3 ? 32767 : g.int(65536), 2 * k);
        for (let k = 0; k < 3; ++k) {
            r.writeUInt16LE(sp(k) ? HALF_SPECIALS[(special + k) % HALF_SPECIALS.length] : g.half(4, 18, false), M.scale + 2 * k);
        }
        for (let k = 0; k < 4; ++k) {
            r.writeUInt16LE(sp(k + 1) ? HALF_SPECIALS[(special + k + 5) % HALF_SPECIALS.length] : g.half(8, 15, true), M.rot + 2 * k);
        }
        for (let k = 0; k < D; ++k) {
            if (mode === 1) {
                r.writeUInt16LE(sp(k + 2) ? HALF_SPECIALS[(special + k) % HALF_SPECIALS.length] : g.half(6, 14, true), M.sh + 2 * k);
            } else {
                r[M.sh + k] = sp(k + 2) ? [0, 255, 128][k % 3] : g.int(256);
            }
        }
    }
    for (let k = 0; k < 4; ++k) r[M.color + k] = special !== null && k === 3 ? [0, 255, 1, 254][special % 4] : g.int(256);
    return r;
};

// spec: { mode, major, minor, numSplats (header; default the sections' total), minH, maxH, seed,
//         sections: [{ count, max, degree, capacity, buckets, full, partial: [sizes], block, storage, quant,
//                      centres: [f32 bit patterns] (optional), specialEvery }] }
const makeKsplat = (spec) => {
    const g = new Gen(spec.seed);
    const ns = spec.sections.length;
    const head = Buffer.alloc(4096 + 1024 * ns);
    head[0] = spec.major === undefined ? 0 : spec.major;
    head[1] = spec.minor === undefined ? 1 : spec.minor;
    head.writeUInt32LE(ns, 4);
    head.writeUInt32LE(ns, 8);
    const total = spec.sections.reduce((a, s) => a + s.count, 0);
    head.writeUInt32LE(spec.numSplats === undefined ? total : spec.numSplats, 16);
    head.writeUInt16LE(spec.mode, 20);
    head.writeFloatLE(spec.minH || 0, 36);
    head.writeFloatLE(spec.maxH || 0, 40);
    const parts = [head];
    spec.sections.forEach((s, si) => {
        const o = 4096 + 1024 * si;
        const storage = s.storage === undefined ? 12 : s.storage;
        head.writeUInt32LE(s.count, o);
        head.writeUInt32LE(s.max, o + 4);
        head.writeUInt32LE(s.capacity, o + 8);
        head.writeUInt32LE(s.buckets, o + 12);
        head.writeFloatLE(s.block, o + 16);
        head.writeUInt16LE(storage, o + 20);
        head.writeUInt32LE(s.quant || 0, o + 24);
        head.writeUInt32LE(s.full, o + 32);
        head.writeUInt32LE(s.partial.length, o + 36);
        head.writeUInt16LE(s.degree, o + 40);
        const sizes = Buffer.alloc(4 * s.partial.length);
        s.partial.forEach((v, k) => sizes.writeUInt32LE(v, 4 * k));
        const centres = Buffer.alloc(storage * s.buckets);
        for (let k = 0; k < Math.floor(centres.length / 4); ++k) {
            if (s.centres && s.centres[k] !== undefined) centres.writeUInt32LE(s.centres[k], 4 * k);
            else centres.writeFloatLE(g.bell(20), 4 * k);
        }
        const stride = KS_MODES[spec.mode].base + SH_COUNT[s.degree] * KS_MODES[spec.mode].shBytes;
        const data = Buffer.alloc(stride * s.max);
        for (let i = 0; i < s.max; ++i) {   // the slack records past `count` are filled too
            const special = s.specialEvery && i % s.specialEvery === 0 ? i / s.specialEvery : null;
            ksRecord(g, spec.mode, s.degree, special).copy(data, i * stride);
        }
        parts.push(sizes, centres, data);
    });
    return Buffer.concat(parts);
};

const ksOne = (mode, degree, seed) => ({
    mode, seed,
    minH: degree === 2 ? -2.25 : 0, maxH: degree === 2 ? 1.75 : 0,
    sections: [{ count: 200, max: 200, degree, capacity: 32, buckets: 6, full: 4, partial: [40, 32], block: 5.0,
        quant: degree === 1 ? 4095 : 0, specialEvery: 17 }]
});

// ---------------------------------------------------------------------------
// .spz (inflated): 16-byte header, then planes: positions 9n, alphas n, colours 3n, scales 3n, rotations 3n, SH Dn
const makeSpzRaw = ({ version, n, degree, fb, seed, magic }) => {
    const g = new Gen(seed);
    const D = SH_COUNT[degree] || 0;
    const b = Buffer.alloc(16 + n * (19 + D));
    b.write(magic || 'NGSP', 0, 'ascii');
    b.writeUInt32LE(version, 4);
    b.writeUInt32LE(n, 8);
    b[12] = degree; b[13] = fb; b[14] = 1; b[15] = 0;
    for (let k = 16; k < b.length; ++k) b[k] = g.int(256);
    if (n >= 4) {   // alpha bytes 0 and 255, a zero and an all-ones position
        b[16 + 9 * n] = 0; b[16 + 9 * n + 1] = 255;
        for (let k = 0; k < 3; ++k) { b[16 + k] = 0; b[16 + 3 + k] = 255; }
        b[16 + 6] = 0; b[16 + 7] = 0; b[16 + 8] = 0x80;   // the most negative 24-bit value
    }
    return b;
};
const gz = (raw) => zlib.gzipSync(raw, { level: 9 });

// ---------------------------------------------------------------------------
const dir = fs.mkdtempSync('/tmp/st_readers_');
const run = async (format, bytes) => {
    const p = path.join(dir, `f.${format}`);
    fs.writeFileSync(p, bytes);
    const fh = await fs.promises.open(p, 'r');
    try { return await READERS[format](fh); } finally { await fh.close(); }
};

// the two recorders of a fixture set: ok() runs a file the reader accepts and records its bytes and
// columns, bad() one it rejects and records the message
const recorders = (fx) => {
    fx.meta.cases = [];
    fx.meta.errors = [];

    const ok = async (name, format, bytes, note) => {
        const res = await run(format, bytes);
        if (res.comments.length !== 0 || res.elements.length !== 1 || res.elements[0].name !== 'vertex') throw new Error(name);
        const cols = res.elements[0].dataTable.columns;
        const n = cols.length ? cols[0].data.length : 0;
        const all = new Float32Array(cols.length * n);
        cols.forEach((c, k) => {
            if (!(c.data instanceof Float32Array) || c.data.length !== n) throw new Error(`${name}: column ${c.name}`);
            all.set(c.data, k * n);
        });
        fx.add(`${name}_file`, new Uint8Array(bytes));
        fx.add(`${name}_cols`, all, [cols.length, n]);
        fx.meta.cases.push({ name, format, n, nsh: cols.length - 14, columns: cols.map(c => c.name), note: note || '' });
    };
    const bad = async (name, format, bytes, note) => {
        let message = null;
        try { await run(format, bytes); } catch (e) { message = e.message; }
        if (message === null) throw new Error(`${name}: the reference accepted the file`);
        if (bytes.length) fx.add(`${name}_file`, new Uint8Array(bytes));
        fx.meta.errors.push({ name, format, size: bytes.length, message, note: note || '' });
    };
    return { ok, bad };
};

const main = async () => {
    const fx = new Fixture('readers');
    const { ok, bad } = recorders(fx);

    // ---- .splat
    for (const n of [1, 255, 257, 1025]) {
        await ok(`splat_n${n}`, 'splat', makeSplat(n, 100 + n),
            'rows 0-5: scales 0 / -1 / -0 / Inf / NaN / subnormal / sNaN / -Inf, opacity bytes 0 255 1 254, quaternion bytes all ' +
            '127, all 128, mixed 127/128, all 0, all 255.  The zero-length quaternion branch (read-splat.ts:131-137) cannot be ' +
            'reached from bytes: (b / 255) * 2 - 1 = 0 has no byte solution (127 gives -1/255, 128 gives +1/255), so it has no row');
    }
    await bad('splat_err_size', 'splat', makeSplat(2, 1).subarray(0, 33));
    await bad('splat_err_empty', 'splat', Buffer.alloc(0));

    // ---- .ksplat
    let seed = 200;
    for (const mode of [0, 1, 2]) {
        for (const degree of [0, 1, 2]) await ok(`ksplat_m${mode}_d${degree}`, 'ksplat', makeKsplat(ksOne(mode, degree, ++seed)));
    }
    const sec = (o) => Object.assign({ capacity: 8, buckets: 3, full: 1, partial: [4, 100], block: 3.5, specialEvery: 7 }, o);
    await ok('ksplat_two_sections', 'ksplat', makeKsplat({ mode: 1, seed: ++seed, sections: [
        sec({ count: 40, max: 48, degree: 1 }), sec({ count: 60, max: 64, degree: 2, quant: 1000 })] }),
        'degrees 1 and 2, maxSectionSplats > count: the degree-1 section lands in columns channel * 3 + coeff of 24');
    await ok('ksplat_empty_middle', 'ksplat', makeKsplat({ mode: 2, seed: ++seed, minH: -0.75, maxH: 3, sections: [
        sec({ count: 30, max: 32, degree: 1 }), sec({ count: 0, max: 8, degree: 2, buckets: 2, partial: [5] }),
        sec({ count: 20, max: 20, degree: 0 })] }),
        'the empty section is skipped by the degree scan but its storage is stepped over');
    await ok('ksplat_partial_walk', 'ksplat', makeKsplat({ mode: 1, seed: ++seed, sections: [
        { count: 5, max: 8, degree: 0, capacity: 2, buckets: 4, full: 1, partial: [0, 0, 3], block: 2.0 }] }),
        'one bucket step per splat: splats 2, 3, 4 take buckets 2, 3, 3');
    await ok('ksplat_partial_short', 'ksplat', makeKsplat({ mode: 1, seed: ++seed, sections: [
        { count: 12, max: 12, degree: 0, capacity: 4, buckets: 3, full: 1, partial: [2, 1], block: 2.0 }] }),
        'partial sizes sum below the partial splat count: bucket index 3 of 3 gives NaN positions');
    await ok('ksplat_fp16_specials', 'ksplat', makeKsplat({ mode: 1, seed: ++seed, sections: [
        sec({ count: 48, max: 48, degree: 1, specialEvery: 1 })] }), '+-0, subnormals, +-Inf, NaN in scale / rotation / SH');
    await ok('ksplat_nonfinite_block', 'ksplat', makeKsplat({ mode: 2, seed: ++seed, minH: -Infinity, maxH: Infinity, sections: [
        sec({ count: 16, max: 16, degree: 1, block: Infinity, quant: 32767, specialEvery: 2, buckets: 3, full: 1, partial: [4, 100],
            centres: [0x7f800000, 0xff800000, 0x7fc00001, 0xff800000, 0x7f800000, 0x7f800001] })] }),
        'an infinite block size and harmonics range: 0 * Inf and Inf - Inf give the sign-set NaN');

    const okFile = () => makeKsplat(ksOne(2, 1, 999));
    await bad('ksplat_err_short', 'ksplat', okFile().subarray(0, 100));
    await bad('ksplat_err_version', 'ksplat', makeKsplat(Object.assign(ksOne(2, 1, 999), { major: 1, minor: 0 })));
    { const f = okFile(); f.writeUInt16LE(3, 20); await bad('ksplat_err_mode', 'ksplat', f); }
    { const f = okFile(); f.writeUInt32LE(0, 16); await bad('ksplat_err_zero', 'ksplat', f); }
    await bad('ksplat_err_mismatch', 'ksplat', makeKsplat(Object.assign(ksOne(2, 1, 999), { numSplats: 210 })));
    { const f = okFile(); await bad('ksplat_err_truncated', 'ksplat', f.subarray(0, f.length - 10)); }
    await bad('ksplat_err_misaligned', 'ksplat', makeKsplat({ mode: 2, seed: 998, sections: [
        sec({ count: 5, max: 5, degree: 1 }), sec({ count: 4, max: 4, degree: 0 })] }),
        'the second section starts at an odd offset (5 records of 33 bytes)');

    // ---- .spz
    for (const version of [2, 3]) {
        for (const degree of [0, 1, 2, 3]) {
            for (const n of [4, 300]) {
                const fb = n === 4 ? 33 : 12;
                await ok(`spz_v${version}_d${degree}_n${n}`, 'spz', gz(makeSpzRaw({ version, n, degree, fb, seed: ++seed })),
                    `fractional bits ${fb}`);
            }
        }
    }
    await ok('spz_v2_fb31', 'spz', gz(makeSpzRaw({ version: 2, n: 4, degree: 0, fb: 31, seed: ++seed })), '1 << 31 is negative');
    await ok('spz_v3_fb33_n300', 'spz', gz(makeSpzRaw({ version: 3, n: 300, degree: 0, fb: 33, seed: ++seed })), 'the shift count is taken mod 32');
    await ok('spz_empty', 'spz', gz(makeSpzRaw({ version: 2, n: 0, degree: 1, fb: 12, seed: ++seed })), 'n = 0: an empty table');
    await ok('spz_degree5', 'spz', gz(makeSpzRaw({ version: 2, n: 4, degree: 5, fb: 12, seed: ++seed })),
        'a degree past 3 has no component count: the reader makes no f_rest columns and does not throw');

    await bad('spz_err_magic', 'spz', gz(makeSpzRaw({ version: 2, n: 4, degree: 0, fb: 12, seed: 1, magic: 'NGSQ' })));
    await bad('spz_err_version', 'spz', gz(makeSpzRaw({ version: 4, n: 4, degree: 0, fb: 12, seed: 1 })));
    await bad('spz_err_raw', 'spz', makeSpzRaw({ version: 2, n: 4, degree: 0, fb: 12, seed: 1 }),
        'not gzipped: the reader sizes itself from the 4-byte magic buffer');
    { const raw = makeSpzRaw({ version: 2, n: 40, degree: 1, fb: 12, seed: 1 }); await bad('spz_err_truncated', 'spz', gz(raw.subarray(0, raw.length - 7))); }
    await bad('spz_err_v3_n1', 'spz', gz(makeSpzRaw({ version: 3, n: 1, degree: 0, fb: 12, seed: 1 })),
        'the 4-byte rotation read at offset 0 of a 3-byte plane');

    fx.save();
    fs.rmdirSync(dir, { recursive: true });
};

// (make_golden_readers_edges.js builds its files with the same functions)
module.exports = { Gen, Fixture, recorders, makeKsplat, makeSpzRaw, gz, dir };

if (require.main === module) main().catch((e) => { console.error(e); process.exit(1); });
