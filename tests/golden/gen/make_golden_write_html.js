'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/write_html.{json,bin}.
//
// Runs the reference's writeHtml (type-erased into $ST_REF_JS by build_ref_html.py, never
// committed) on seeded tables and tiny viewer templates of our own, into a scratch file, and
// records the three template strings, the camera and target, every input column and the bytes of
// the file it wrote.  The page text is therefore V8's own String.prototype.replace and
// JSON.stringify, the payload Node's Buffer.toString('base64') of the reference's own
// writeCompressedPly file.
//
// The viewer package ('@playcanvas/supersplat-viewer': html, css, js) is not used: a stand-in
// module of that name is written into $ST_REF_JS/node_modules (the staging directory, never the
// repository) and exports the current case's three strings.  The reference writes its
// intermediate temp.ply into os.tmpdir(): TMPDIR points into the staging directory meanwhile.
//
//   python3 tests/golden/gen/build_ref_html.py && node tests/golden/gen/make_golden_write_html.js
//
// Reference call site exercised: writers/write-html.ts:10-59 (and write-compressed-ply.ts:31-115).

const fs = require('fs');
const path = require('path');

const REF = process.env.ST_REF_JS || '/tmp/st_ref_js';
const OUT = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');

const SCRATCH = path.join(REF, '__tmp');
fs.mkdirSync(SCRATCH, { recursive: true });
process.env.TMPDIR = SCRATCH;

const VIEWER = path.join(REF, 'node_modules', '@playcanvas', 'supersplat-viewer');
fs.mkdirSync(VIEWER, { recursive: true });
fs.writeFileSync(path.join(VIEWER, 'index.js'), 'module.exports = global.__st_viewer_case;\n');

const { Column, DataTable } = require(path.join(REF, 'data-table.js'));
const { Vec3 } = require(path.join(REF, '__stubs/playcanvas.js'));

// writeHtml binds html / css / js when its module loads: load it afresh for every case
const loadWriteHtml = (viewer) => {
    global.__st_viewer_case = viewer;
    for (const k of Object.keys(require.cache)) {
        if (k.endsWith(path.join('writers', 'write-html.js')) || k.startsWith(VIEWER)) delete require.cache[k];
    }
    return require(path.join(REF, 'writers/write-html.js')).writeHtml;
};

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

const DTYPES = { Uint8Array: 'u1', Float32Array: 'f4', Float64Array: 'f8' };

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
            generator: 'tests/golden/gen/make_golden_write_html.js (reference modules type-erased by build_ref_html.py)',
            reference: '@playcanvas/splat-transform 0.10.1',
            meta: this.meta,
            arrays: this.arrays
        }, null, 1));
        process.stderr.write(`  ${this.name}: ${Object.keys(this.arrays).length} arrays, ${(this.offset / 1024).toFixed(1)} KiB\n`);
    }
}

const gsNames = coeffs => ['x', 'y', 'z', 'f_dc_0', 'f_dc_1', 'f_dc_2']
    .concat(Array.from({ length: 3 * coeffs }, (_, i) => `f_rest_${i}`))
    .concat(['opacity', 'scale_0', 'scale_1', 'scale_2', 'rot_0', 'rot_1', 'rot_2', 'rot_3']);

const splats = (n, coeffs, u) => gsNames(coeffs).map((nm) => {
    const a = new Float32Array(n);
    const s = nm.startsWith('f_rest_') ? 0.5 : 3;
    for (let i = 0; i < n; ++i) a[i] = (u() + u() + u() + u() - 2) * s;
    return [nm, a];
});

// the four patterns of write-html.ts:46-49
const STYLE = '<link rel="stylesheet" href="./index.css">';
const SCRIPT = '<script type="module" src="./index.js"></script>';
const SETTINGS = 'settings: fetch(settingsUrl).then(response => response.json())';
const CONTENT = 'fetch(contentUrl)';

const PAGE = `<!DOCTYPE html>
<html>
    <head>
        <title>viewer</title>
        ${STYLE}
    </head>
    <body>
        <canvas id="c"></canvas>
        ${SCRIPT}
        <script type="module">
            import { main } from './index.js';
            const settingsUrl = './settings.json', contentUrl = './scene.compressed.ply';
            main({ ${SETTINGS}, content: ${CONTENT} });
        </script>
    </body>
</html>
`;
const CSS = 'body {\n    margin: 0;\n}\n\n\ncanvas { width: 100%; }\n';
const JS = 'const main = (o) => {\n\n    return o;\n};\nexport { main };\n';

// name -> { html, css, js, n, coeffs, camera, target }
const CASES = {
    // the four targets once each; css / js with empty lines and a trailing newline; two chunks, the
    // last partial
    plain: { html: PAGE, css: CSS, js: JS, n: 300, coeffs: 0 },
    // file lengths 1, 2, 0 modulo 3 apart from a header of one length: '=', '==' and no padding
    mod3_1: { html: PAGE, css: 'a{}', js: ';', n: 1, coeffs: 0 },
    mod3_2: { html: PAGE, css: 'a{}', js: ';', n: 2, coeffs: 0 },
    mod3_3: { html: PAGE, css: 'a{}', js: ';', n: 3, coeffs: 0 },
    // band 3: the sh element
    sh3: { html: PAGE, css: CSS, js: JS, n: 257, coeffs: 15 },
    // the replacement patterns of String.prototype.replace inside the inserted text
    dollars: {
        html: PAGE,
        css: 'a::after { content: "$$ $& $1 $<a> $0 $"; }\n.b { c: "$`"; }\n.d$',
        js: 'const t = `cost: $$5 [$&] [$\'] $1 $<a>`;\nconst r = /x$/;\nlet u = "$',
        n: 5,
        coeffs: 0
    },
    // inserted text holds later patterns; the html holds each pattern twice
    nested: {
        html: `<html>\n${STYLE}\n${STYLE}\n${SCRIPT}\n${SCRIPT}\n<script>go({ ${SETTINGS}, ${SETTINGS} }, ${CONTENT}, ${CONTENT});</script>\n</html>`,
        css: `/* ${SCRIPT} */\n.x::before { content: '${CONTENT}'; }\n/* ${SETTINGS} */`,
        js: `load(${CONTENT});\n// ${STYLE}`,
        n: 7,
        coeffs: 0
    },
    // neither the style link nor fetch(contentUrl): nothing is embedded
    missing: {
        html: `<html>\n<head></head>\n<body>\n${SCRIPT}\n<script>go({ ${SETTINGS} });</script>\n</body>\n</html>\n`,
        css: CSS,
        js: JS,
        n: 4,
        coeffs: 0
    },
    // JSON.stringify of numbers
    camera: { html: PAGE, css: 'a{}', js: ';', n: 6, coeffs: 0, camera: [-0, 1e21, 1e-7], target: [0.1, NaN, Infinity] },
    // multi-byte text before and between the patterns
    utf8: {
        html: `<html lang="de">\n<!-- größe µ — 視点 🎥 -->\n${STYLE}\n<p>naïve café ✓</p>\n${SCRIPT}\n<script>/* ünï */ go({ ${SETTINGS} /* λ */, c: ${CONTENT} }); // конец\n</script>\n</html>\n`,
        css: 'p::after { content: "→ ✓"; }\n/* 日本語 */',
        js: 'const s = "ß🎥";\n// é',
        n: 9,
        coeffs: 0,
        camera: [1.5, -2.25, 3],
        target: [0, 0.5, -1]
    }
};

const utf8 = s => new Uint8Array(Buffer.from(s, 'utf8'));

const main = async () => {
    const fx = new Fixture('write_html');
    const tmp = path.join(SCRATCH, `st_write_html_${process.pid}.html`);
    let seed = 9100;
    for (const [name, spec] of Object.entries(CASES)) {
        const cols = splats(spec.n, spec.coeffs, mulberry32(seed++));
        const dataTable = new DataTable(cols.map(([nm, data]) => new Column(nm, data)));
        const camera = spec.camera || [2, 2, -2], target = spec.target || [0, 0, 0];
        const writeHtml = loadWriteHtml({ html: spec.html, css: spec.css, js: spec.js });
        const fh = await fs.promises.open(tmp, 'w');
        try {
            await writeHtml(fh, { comments: [], elements: [{ name: 'vertex', dataTable }] },
                new Vec3(camera[0], camera[1], camera[2]), new Vec3(target[0], target[1], target[2]));
        } finally {
            await fh.close();
        }
        const file = fs.readFileSync(tmp);
        fs.unlinkSync(tmp);
        fx.add(`${name}_file`, new Uint8Array(file.buffer, file.byteOffset, file.length));
        fx.add(`${name}_html`, utf8(spec.html));
        fx.add(`${name}_css`, utf8(spec.css));
        fx.add(`${name}_js`, utf8(spec.js));
        fx.add(`${name}_camera`, new Float64Array(camera));
        fx.add(`${name}_target`, new Float64Array(target));
        fx.meta[name] = { rows: spec.n, sh_coeffs: spec.coeffs, columns: cols.map(([nm]) => nm) };
        cols.forEach(([, data], i) => fx.add(`${name}_col${i}`, data));
    }
    fx.save();
};

main().catch((e) => { console.error(e); process.exit(1); });
