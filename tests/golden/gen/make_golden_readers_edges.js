'use strict';
// TEST INFRASTRUCTURE ONLY: generates tests/golden/readers_edges.{json,bin}.
//
// A second set of reader fixtures, made as make_golden_readers.js makes `readers` (the
// reference's own readers, type-erased into $ST_REF_JS, run on files built here with that script's
// builders), at the places where a device decode that stages unaligned byte ranges can go wrong:
//
//   .spz      row counts 257, 258, 259 (every plane offset 16 + 9n, + 10n, + 13n, + 19n and the file
//             length take every residue mod 4; two 256-row tiles, the second of 1-3 rows), both
//             versions, tiny files (n = 1, 2, 3, 5) and directed version-3 rotation words
//   .ksplat   a bucketStorageSizeBytes of 13 or 14 (the records start at an offset that is 1, 2 or 3
//             mod 4), sections of 257 records with 20 partial buckets, a second section that starts
//             mid-tile, records of fully random bytes
//
//   python3 tests/golden/gen/build_ref_readers.py && node tests/golden/gen/make_golden_readers_edges.js

const fs = require('fs');
const path = require('path');
const assert = require('assert');
const { Gen, Fixture, recorders, makeKsplat, makeSpzRaw, gz, dir } = require('./make_golden_readers.js');

// file offset of record 0 of the only section of a one-section file
const ksDataOff = (s) => 4096 + 1024 + 4 * s.partial.length + (s.storage === undefined ? 12 : s.storage) * s.buckets;

// the records (slack ones included) of a one-section file overwritten with random bytes
const randomRecords = (file, spec, seed) => {
    const g = new Gen(seed);
    for (let k = ksDataOff(spec.sections[0]); k < file.length; ++k) file[k] = g.int(256);
    return file;
};

const main = async () => {
    const fx = new Fixture('readers_edges', 'tests/golden/gen/make_golden_readers_edges.js');
    const { ok } = recorders(fx);
    let seed = 5000;

    // ---- .spz: n = 257, 258, 259 (n mod 4 = 1, 2, 3).  Plane skews (offset mod 4) at these n:
    //        n    alpha colour scale rot sh   length mod 4 at degree 0 / 2
    //        257    1     2     1    0   3        3 / 3
    //        258    2     0     2    0   2        2 / 2
    //        259    3     2     3    0   1        1 / 1
    const spz = async (version, degree, n, fb, note) => {
        const raw = makeSpzRaw({ version, n, degree, fb, seed: ++seed });
        await ok(`spz_v${version}_d${degree}_n${n}`, 'spz', gz(raw), `fractional bits ${fb}; inflated length ${raw.length}${note ? '; ' + note : ''}`);
    };
    for (const n of [257, 258, 259]) await spz(2, 2, n, 12);   // version 2, degree 2, every residue
    await spz(3, 1, 257, 10);                                  // version 3 with SH at every residue:
    await spz(3, 1, 258, 14);                                  //   degree 1 (an odd n among them)
    await spz(3, 3, 259, 12);                                  //   degree 3 at an odd n
    await spz(2, 0, 257, 23);                                  // degree 0 at every residue
    await spz(3, 0, 258, 12);
    await spz(2, 0, 259, 0);
    await spz(3, 2, 259, 12);                                  // and each degree in the other version too
    await spz(2, 3, 257, 12);
    await spz(2, 1, 259, 31);
    await spz(2, 0, 1, 12, 'one row');
    await spz(3, 0, 2, 12, 'the smallest version-3 file the reader accepts');
    await spz(3, 2, 3, 12);
    await spz(2, 2, 5, 12);
    {
        // version 3 reads the big-endian word at byte `row` of the rotation plane.  Rows 0, 4, 8, 12:
        //   3f ff ff ff  largest 0, three magnitudes 511 (negative): 1 - sum_squares < 0
        //   5f f7 fd ff  largest 1, three magnitudes 511 (positive): the same
        //   bf ff ff ff  top bits 10: `>> 30` of the int32 gives -2, no component is skipped
        //   df f7 fd ff  top bits 11: -1
        // and the rows between them read the same bytes shifted by one, two and three
        const n = 17;
        const raw = makeSpzRaw({ version: 3, n, degree: 0, fb: 12, seed: ++seed });
        const rot = 16 + 16 * n;
        [0x3f, 0xff, 0xff, 0xff, 0x5f, 0xf7, 0xfd, 0xff, 0xbf, 0xff, 0xff, 0xff, 0xdf, 0xf7, 0xfd, 0xff].forEach((v, k) => { raw[rot + k] = v; });
        await ok('spz_v3_rot_directed', 'spz', gz(raw), 'rotation words with each value of the two top bits and all three magnitudes 511');
    }

    // ---- .ksplat: records at an offset that is not a multiple of 4
    const unaligned = [
        { mode: 0, degree: 1, storage: 13, buckets: 3, max: 131 },   // data_off = 3 mod 4
        { mode: 1, degree: 2, storage: 14, buckets: 3, max: 131 },   //            2
        { mode: 2, degree: 1, storage: 13, buckets: 5, max: 130 }    //            1
    ];
    for (const u of unaligned) {
        const spec = { mode: u.mode, seed: ++seed, minH: -1.25, maxH: 2.5, sections: [
            { count: 129, max: u.max, degree: u.degree, capacity: 32, buckets: u.buckets, full: 2, partial: [40, 30], block: 4.0,
                storage: u.storage, specialEvery: 13 }] };
        const file = makeKsplat(spec);
        assert(ksDataOff(spec.sections[0]) % 4 !== 0 && file.length % 4 !== 0);
        await ok(`ksplat_m${u.mode}_storage${u.storage}`, 'ksplat', file,
            `bucketStorageSizeBytes ${u.storage} x ${u.buckets} buckets: record 0 at file offset ${ksDataOff(spec.sections[0])}, ` +
            `file length ${file.length}`);
    }

    // ---- .ksplat: three tiles of records, twenty partial buckets (32 splats in two full buckets, 225 in the partial ones)
    const walkLong = [10, 0, 0, 25, 40, 30, 0, 17, 20, 0, 0, 33, 29, 12, 15, 3, 0, 4, 1, 2];    // sum 241: runs cross records 128 and 256
    const walkShort = [10, 0, 0, 25, 40, 30, 0, 17, 20, 0, 0, 14, 9, 0, 6, 3, 0, 4, 1, 2];    // sum 181 < 225
    await ok('ksplat_m1_walk257', 'ksplat', makeKsplat({ mode: 1, seed: ++seed, sections: [
        { count: 257, max: 260, degree: 1, capacity: 16, buckets: 22, full: 2, partial: walkLong, block: 3.0, specialEvery: 31 }] }),
        'partial sizes with zeros whose runs cross records 128 and 256');
    await ok('ksplat_m2_walk257_short', 'ksplat', makeKsplat({ mode: 2, seed: ++seed, sections: [
        { count: 257, max: 257, degree: 0, capacity: 16, buckets: 22, full: 2, partial: walkShort, block: 3.0, specialEvery: 31 }] }),
        'partial sizes sum to 181 of 225 partial splats: the tail takes bucket 22 of 22 (NaN centre) in the second and third tile');

    // ---- .ksplat: the second section starts mid-tile and has the higher degree
    await ok('ksplat_two_sections_midtile', 'ksplat', makeKsplat({ mode: 2, seed: ++seed, minH: -2, maxH: 1.5, sections: [
        { count: 70, max: 72, degree: 1, capacity: 8, buckets: 12, full: 4, partial: [9, 0, 20, 100], block: 3.5, specialEvery: 7 },
        { count: 200, max: 200, degree: 2, capacity: 8, buckets: 30, full: 10, partial: [50, 0, 0, 31, 64], block: 2.5, quant: 1000, specialEvery: 11 }] }),
        'rows 70..269 come from the second section; the first leaves f_rest columns 9..23 at +0');

    // ---- .ksplat: records of random bytes (arbitrary f32 / half bit patterns, NaN payloads included)
    for (const [mode, degree] of [[0, 1], [1, 2], [2, 3]]) {
        const spec = { mode, seed: ++seed, minH: -3, maxH: 0.5, sections: [
            { count: 129, max: 129, degree, capacity: 32, buckets: 6, full: 2, partial: [30, 0, 50], block: 6.0 }] };
        await ok(`ksplat_m${mode}_random`, 'ksplat', randomRecords(makeKsplat(spec), spec, ++seed), 'every record byte random');
    }

    fx.save();
    const out = process.env.ST_GOLDEN_OUT || path.join(__dirname, '..');
    assert(fx.offset + fs.statSync(path.join(out, 'readers_edges.json')).size < (1 << 20), 'the set must stay under 1 MiB');
    fs.rmdirSync(dir, { recursive: true });
};

main().catch((e) => { console.error(e); process.exit(1); });
