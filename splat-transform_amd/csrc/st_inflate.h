// st_inflate.h -- the chunked INFLATE (RFC 1951 decoder) of include/st_abi.h, "inflating a gzip
// member on the device": the rules that the kernels (st_inflate.hip) and a serial host
// implementation of the SAME chunked method share, all __host__ __device__, so a host program
// (tests/native/inflate_cpu_check.cpp) walks the steps the device walks and reports the same
// numbers.
//
//   Bits / take / decode_sym     the LSB-first bit reader (never past the stream) and the canonical
//                                decode: one bit per step, first code and count per length
//   count_code / build_code      lengths -> counts per length, completeness, symbols in code order
//   read_dynamic                 a dynamic block's header: HLIT, HDIST, the code-length code, the
//                                length sequence, with every check zlib makes
//   candidate_at                 the finder's predicate for one bit position
//   decode_block                 one block into a sink (SizeSink counts, WriteSink writes 16-bit
//                                symbols and markers, HeadSink writes the first bytes)
//   joins                        the stop rule after a block
//   size_decoder / write_decoder one decoder's two passes
//   chain_walk                   the walk from chunk 0 along the JOINED links (host)
//   marker / resolve_sym         marker encoding and window resolution
//   inflate_chunked              the serial whole-stream form (host)
//
// What is accepted is never more than zlib accepts: a header or code zlib refuses is refused here,
// and some things zlib takes are refused too (bytes after the final block).  Refusing costs a
// "declined", never a wrong byte.
#pragma once

#include <cstdint>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#include <vector>

#define ST_HD __host__ __device__ inline

namespace st {
namespace infl {

constexpr uint32_t WIN = 32768;           // the window: no distance is greater
constexpr uint32_t CHUNK_DEFAULT = 65536; // ST_INFLATE_CHUNK
constexpr uint32_t CHUNK_MIN = 256;
constexpr uint32_t BUDGET_MULT = 512;     // ST_INFLATE_BUDGET: coded symbols per decoder, in chunk_bytes
constexpr uint64_t NONE = ~0ull;          // a chunk without a candidate
constexpr int NLENS = 320;                // 288 + 32: the lengths of both codes of a block

enum : uint32_t { S_IDLE = 0, S_FINAL = 1, S_JOINED = 2, S_ERROR = 3 };

// ---- bits ----------------------------------------------------------------------------------------
struct Bits {
    const uint8_t *in;
    uint64_t n, next;  // the stream's bytes; the next byte to load
    uint64_t buf;
    uint32_t cnt;      // valid bits in buf
};
ST_HD void refill(Bits &b) {
    if (b.cnt <= 56 && b.next + 8 <= b.n) {
        // one 8-byte load (any alignment) in place of up to eight dependent byte loads; the bits above
        // cnt that come along are the stream's own next bits, ORed in again unchanged by the next refill
        uint64_t w;
        __builtin_memcpy(&w, b.in + b.next, 8);
        b.buf |= w << b.cnt;
        const uint32_t k = (63u - b.cnt) >> 3;
        b.next += k;
        b.cnt += 8 * k;
        return;
    }
    while (b.cnt <= 56 && b.next < b.n) {
        b.buf |= (uint64_t)b.in[b.next++] << b.cnt;
        b.cnt += 8;
    }
}
ST_HD uint64_t bit_pos(const Bits &b) { return 8 * b.next - b.cnt; }
// the reader at bit position pos <= 8n
ST_HD void bits_at(Bits &b, const uint8_t *in, uint64_t n, uint64_t pos) {
    b.in = in, b.n = n, b.buf = 0, b.cnt = 0;
    b.next = pos >> 3 < n ? pos >> 3 : n;
    refill(b);
    const uint32_t drop = (uint32_t)(pos & 7);
    if (b.cnt >= drop) b.buf >>= drop, b.cnt -= drop;
}
// k <= 32 bits; false at the end of the stream
ST_HD bool take(Bits &b, uint32_t k, uint32_t &v) {
    if (b.cnt < k) {
        refill(b);
        if (b.cnt < k) return false;
    }
    v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
    b.buf >>= k;
    b.cnt -= k;
    return true;
}

// ---- codes ---------------------------------------------------------------------------------------
// count[0..15] of the n lengths; returns what the code leaves unused in units of 2^-15 of the code
// space, negative when it is over-subscribed
ST_HD int count_code(uint16_t *count, const uint8_t *lens, int n) {
    for (int l = 0; l <= 15; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s]];
    if (count[0] == n) return 0;  // no code at all: whatever is decoded with it fails
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
    }
    return left;
}
// zlib's rule for a literal/length or distance code: complete, or a single code of length 1
ST_HD bool code_accepted(const uint16_t *count, int n, int left) {
    return left == 0 || (left > 0 && n - count[0] == 1 && count[1] == 1);
}
// symbol[] = the symbols in code order (canonical: by length, then by symbol)
ST_HD int build_code(uint16_t *count, uint16_t *symbol, const uint8_t *lens, int n) {
    const int left = count_code(count, lens, n);
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s]) symbol[offs[lens[s]]++] = (uint16_t)s;
    return left;
}
// one symbol: at least one bit is consumed, or -1 (no such code, or the stream ends)
ST_HD int decode_sym(Bits &b, const uint16_t *count, const uint16_t *symbol) {
    if (b.cnt < 15) refill(b);
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        if (b.cnt < len) return -1;
        code |= (uint32_t)(b.buf >> (len - 1)) & 1u;
        const uint32_t c = count[len];
        if (code < first + c) {
            b.buf >>= len;
            b.cnt -= len;
            return symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// length symbol i = 0..28 (257 + i) and distance symbol d = 0..29: base value and extra bits (RFC 1951 3.2.5)
ST_HD uint32_t len_extra(uint32_t i) { return i < 8 || i == 28 ? 0u : (i >> 2) - 1u; }
ST_HD uint32_t len_base(uint32_t i) { return i < 8 ? 3u + i : i == 28 ? 258u : 3u + ((4u + (i & 3u)) << ((i >> 2) - 1u)); }
ST_HD uint32_t dist_extra(uint32_t d) { return d < 4 ? 0u : (d >> 1) - 1u; }
ST_HD uint32_t dist_base(uint32_t d) { return d < 4 ? 1u + d : 1u + ((2u + (d & 1u)) << ((d >> 1) - 1u)); }

// ---- a dynamic block's header (after BFINAL and BTYPE) ------------------------------------------------
// lens[0..nlen) the literal/length lengths, lens[nlen..nlen + ndist) the distance lengths.  False
// for everything zlib refuses: HLIT or HDIST above 29, a code-length code that is not complete, a
// repeat without a predecessor, a repeat past the end, no code for symbol 256.
ST_HD bool read_dynamic(Bits &b, uint8_t *lens, uint32_t &nlen, uint32_t &ndist) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v = 0;
    if (!take(b, 14, v)) return false;
    nlen = (v & 31u) + 257u;
    ndist = ((v >> 5) & 31u) + 1u;
    const uint32_t ncode = (v >> 10) + 4u;
    if (nlen > 286 || ndist > 30) return false;
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; ++i) {
        if (!take(b, 3, v)) return false;
        cl[order[i]] = (uint8_t)v;
    }
    uint16_t ccount[16], csym[19];
    if (build_code(ccount, csym, cl, 19) != 0) return false;
    const uint32_t total = nlen + ndist;
    uint32_t i = 0;
    while (i < total) {  // every turn adds at least one length
        const int s = decode_sym(b, ccount, csym);
        if (s < 0) return false;
        if (s < 16) {
            lens[i++] = (uint8_t)s;
            continue;
        }
        uint32_t prev = 0, rep = 0;
        if (s == 16) {
            if (i == 0 || !take(b, 2, v)) return false;
            prev = lens[i - 1], rep = 3 + v;
        } else if (s == 17) {
            if (!take(b, 3, v)) return false;
            rep = 3 + v;
        } else {
            if (!take(b, 7, v)) return false;
            rep = 11 + v;
        }
        if (i + rep > total) return false;
        while (rep--) lens[i++] = (uint8_t)prev;
    }
    return lens[256] != 0;
}

// The finder's predicate: a NON-FINAL dynamic block header parses completely at bit position pos
// (BFINAL = 0, BTYPE = 2, read_dynamic's checks, both codes accepted).  It accepts every position
// at which zlib would start such a block; what else it accepts only costs a decoder.
ST_HD bool candidate_at(const uint8_t *in, uint64_t n, uint64_t pos) {
    const uint64_t by = pos >> 3;
    if (by + 3 <= n) {  // the first 13 bits from three bytes: nine positions in ten end here
        const uint32_t w = ((uint32_t)in[by] | (uint32_t)in[by + 1] << 8 | (uint32_t)in[by + 2] << 16) >> (pos & 7);
        if ((w & 7u) != 4u || ((w >> 3) & 31u) > 29u || ((w >> 8) & 31u) > 29u) return false;
    }
    Bits b;
    bits_at(b, in, n, pos);
    uint32_t v = 0;
    if (!take(b, 3, v) || v != 4u) return false;
    uint8_t lens[NLENS];
    uint32_t nlen = 0, ndist = 0;
    if (!read_dynamic(b, lens, nlen, ndist)) return false;
    uint16_t count[16];
    int left = count_code(count, lens, (int)nlen);
    if (!code_accepted(count, (int)nlen, left)) return false;
    left = count_code(count, lens + nlen, (int)ndist);
    return code_accepted(count, (int)ndist, left);
}
// the first candidate in [lo, hi), tested in order (the serial form of the finder's rounds)
ST_HD uint64_t find_candidate(const uint8_t *in, uint64_t n, uint64_t lo, uint64_t hi) {
    for (uint64_t p = lo; p < hi; ++p)
        if (candidate_at(in, n, p)) return p;
    return NONE;
}
// the bit range the finder searches for chunk c >= 1
ST_HD void chunk_bits(uint64_t n, uint32_t chunk_bytes, uint32_t c, uint64_t &lo, uint64_t &hi) {
    lo = 8ull * c * chunk_bytes;
    hi = lo + 8ull * chunk_bytes;
    if (hi > 8 * n) hi = 8 * n;
}

// ---- the decoder's tables: 1,024 bytes per decoder ------------------------------------------------
struct Tables {
    uint8_t *lens;      // NLENS
    uint16_t *lcount;   // 16
    uint16_t *dcount;   // 16
    uint16_t *lsym;     // 288
    uint16_t *dsym;     // 32
};
constexpr uint32_t TABLE_BYTES = NLENS + 32 + 32 + 576 + 64;
// the tables over TABLE_BYTES bytes at an even address
ST_HD Tables tables_at(uint8_t *p) {
    Tables T;
    T.lens = p;
    T.lcount = reinterpret_cast<uint16_t *>(p + NLENS);
    T.dcount = reinterpret_cast<uint16_t *>(p + NLENS + 32);
    T.lsym = reinterpret_cast<uint16_t *>(p + NLENS + 64);
    T.dsym = reinterpret_cast<uint16_t *>(p + NLENS + 64 + 576);
    return T;
}

// ---- markers and windows ----------------------------------------------------------------------------
// A decoder that starts in the middle of the stream does not have the 32 KiB before its first
// byte.  A reference of distance dist made at its own output position j < dist becomes the marker
// 256 + (index into that window); a byte it knows is the symbol 0..255.
ST_HD uint16_t marker(uint32_t dist, uint64_t j) { return (uint16_t)(256u + (WIN - (dist - (uint32_t)j))); }
// the byte of a symbol of the decoder whose first byte is out[base]: out[base - WIN ..) is its window
ST_HD uint8_t resolve_sym(uint16_t s, const uint8_t *out, uint64_t base) {
    return s < 256 ? (uint8_t)s : out[base + (uint64_t)(s - 256u) - WIN];
}

// ---- sinks ------------------------------------------------------------------------------------------
// the size pass: bytes are counted, none is kept.  base_known: the decoder starts at output byte 0,
// so a distance past the start of the output is seen here
struct SizeSink {
    uint64_t count, limit;
    bool base_known;
    ST_HD bool lit(uint32_t) { return ++count <= limit; }
    ST_HD bool match(uint32_t len, uint32_t dist) {
        if (base_known && dist > count) return false;
        count += len;
        return count <= limit;
    }
    ST_HD bool stored(const uint8_t *, uint32_t len) {
        count += len;
        return count <= limit;
    }
};
// the write pass: symbols at sym[0..total), the decoder's first byte being output byte base
struct WriteSink {
    uint16_t *sym;
    uint64_t j, total, base, markers;
    ST_HD bool lit(uint32_t v) {
        if (j >= total) return false;
        sym[j++] = (uint16_t)v;
        return true;
    }
    ST_HD bool match(uint32_t len, uint32_t dist) {
        if (j + len > total || dist > base + j) return false;  // past the start of the output
        for (uint32_t k = 0; k < len; ++k, ++j) {
            const uint16_t s = dist <= j ? sym[j - dist] : marker(dist, j);
            markers += s >= 256;
            sym[j] = s;
        }
        return true;
    }
    ST_HD bool stored(const uint8_t *p, uint32_t len) {
        if (j + len > total) return false;
        for (uint32_t k = 0; k < len; ++k) sym[j++] = p[k];
        return true;
    }
};
// the first `total` bytes of a stream from its start: full is set when they are there
struct HeadSink {
    uint8_t *out;
    uint64_t j, total;
    bool full;
    ST_HD bool lit(uint32_t v) {
        if (j < total) out[j] = (uint8_t)v;
        ++j;
        return !(full = j >= total);
    }
    ST_HD bool match(uint32_t len, uint32_t dist) {
        if (dist > j) return false;
        for (uint32_t k = 0; k < len && j < total; ++k, ++j) out[j] = out[j - dist];
        return !(full = j >= total);
    }
    ST_HD bool stored(const uint8_t *p, uint32_t len) {
        for (uint32_t k = 0; k < len && j < total; ++k) out[j++] = p[k];
        return !(full = j >= total);
    }
};

// ---- one block --------------------------------------------------------------------------------------
// Reads one block at b into the sink.  *final = BFINAL, *btype = 0..2.  budget: the coded symbols
// this decoder may still read; a stored block costs none.  False: a parse error, the end of the
// stream, the budget, or the sink's refusal.
template <class Sink>
ST_HD bool decode_block(Bits &b, Tables &T, Sink &s, uint64_t &budget, bool &final, uint32_t &btype) {
    uint32_t v = 0;
    if (!take(b, 3, v)) return false;
    final = v & 1u;
    btype = v >> 1;
    if (btype == 3) return false;
    if (btype == 0) {
        if (!take(b, b.cnt & 7u, v)) return false;  // to the byte boundary
        uint32_t len = 0, nlen = 0;
        if (!take(b, 16, len) || !take(b, 16, nlen) || len != (~nlen & 0xffffu)) return false;
        const uint64_t p = bit_pos(b) >> 3;
        if (p + len > b.n) return false;
        if (!s.stored(b.in + p, len)) return false;
        bits_at(b, b.in, b.n, 8 * (p + len));
        return true;
    }
    uint32_t nlen = 288, ndist = 30;
    if (btype == 1) {
        for (int i = 0; i < 288; ++i) T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 30; ++i) T.lens[288 + i] = 5;
        build_code(T.lcount, T.lsym, T.lens, 288);
        build_code(T.dcount, T.dsym, T.lens + 288, 30);
    } else {
        if (!read_dynamic(b, T.lens, nlen, ndist)) return false;
        int left = build_code(T.lcount, T.lsym, T.lens, (int)nlen);
        if (!code_accepted(T.lcount, (int)nlen, left)) return false;
        left = build_code(T.dcount, T.dsym, T.lens + nlen, (int)ndist);
        if (!code_accepted(T.dcount, (int)ndist, left)) return false;
    }
    for (;;) {  // every turn takes one of the budget's symbols
        if (budget == 0) return false;
        --budget;
        int sym = decode_sym(b, T.lcount, T.lsym);
        if (sym < 0) return false;
        if (sym < 256) {
            if (!s.lit((uint32_t)sym)) return false;
            continue;
        }
        if (sym == 256) return true;
        sym -= 257;
        if (sym >= 29) return false;
        uint32_t len = len_base((uint32_t)sym);
        if (!take(b, len_extra((uint32_t)sym), v)) return false;
        len += v;
        const int ds = decode_sym(b, T.dcount, T.dsym);
        if (ds < 0 || ds >= 30) return false;
        uint32_t dist = dist_base((uint32_t)ds);
        if (!take(b, dist_extra((uint32_t)ds), v)) return false;
        dist += v;
        if (!s.match(len, dist)) return false;
    }
}

// ---- the stop rule ----------------------------------------------------------------------------------
// After a non-final block that ends at bit p: j moves past the later chunks whose candidate lies
// below p (or is none); true when chunk j's candidate IS p, and the decoder stops there.
ST_HD bool joins(const uint64_t *cand, uint32_t nchunks, uint32_t &j, uint64_t p) {
    while (j < nchunks && (cand[j] == NONE || cand[j] < p)) ++j;
    return j < nchunks && cand[j] == p;
}

// ---- one decoder ------------------------------------------------------------------------------------
struct DecRec {
    uint64_t start, end, bytes;  // bit positions; output bytes
    uint64_t markers;            // the write pass: symbols that are markers
    uint32_t status, link;       // S_*; the chunk joined
    uint32_t blocks[3];          // by BTYPE
    uint32_t wrote;              // the write pass: 1 = every byte written
};
// no block is shorter than 3 bits
ST_HD uint64_t max_blocks(uint64_t n) { return 8 * n / 3 + 1; }

// the size pass of chunk c's decoder (chunk 0 starts at bit 0)
ST_HD void size_decoder(const uint8_t *in, uint64_t n, const uint64_t *cand, uint32_t nchunks, uint32_t c, uint64_t expect,
                        uint32_t chunk_bytes, Tables &T, DecRec &R) {
    R.start = c ? cand[c] : 0;
    R.end = R.start, R.bytes = 0, R.markers = 0, R.status = S_IDLE, R.link = 0, R.wrote = 0;
    R.blocks[0] = R.blocks[1] = R.blocks[2] = 0;
    if (R.start == NONE) return;
    Bits b;
    bits_at(b, in, n, R.start);
    SizeSink s{0, expect, c == 0};
    uint64_t budget = (uint64_t)BUDGET_MULT * chunk_bytes;
    uint32_t j = c + 1;
    R.status = S_ERROR;
    for (uint64_t k = max_blocks(n); k; --k) {
        bool final = false;
        uint32_t btype = 0;
        if (!decode_block(b, T, s, budget, final, btype)) return;
        ++R.blocks[btype];
        R.end = bit_pos(b), R.bytes = s.count;
        if (final) {
            R.status = S_FINAL;
            return;
        }
        if (joins(cand, nchunks, j, R.end)) {
            R.status = S_JOINED, R.link = j;
            return;
        }
    }
}
// the write pass of a kept decoder: the same blocks again, R.bytes symbols at sym (the decoder's
// own first symbol), base = its first byte's place in the output
ST_HD void write_decoder(const uint8_t *in, uint64_t n, uint16_t *sym, uint64_t base, uint32_t chunk_bytes, Tables &T,
                         DecRec &R) {
    Bits b;
    bits_at(b, in, n, R.start);
    WriteSink s{sym, 0, R.bytes, base, 0};
    uint64_t budget = (uint64_t)BUDGET_MULT * chunk_bytes;
    R.wrote = 0;
    for (uint64_t k = max_blocks(n); k; --k) {
        bool final = false;
        uint32_t btype = 0;
        if (!decode_block(b, T, s, budget, final, btype)) return;
        const uint64_t p = bit_pos(b);
        if (p > R.end) return;
        if (p == R.end) break;
    }
    R.markers = s.markers;
    R.wrote = s.j == R.bytes;
}

struct Stats {  // st_inflate_stats
    uint64_t chunks, candidates, kept, discarded, markers, stored_blocks, fixed_blocks, dynamic_blocks;
};

// ---- the chain (host) -------------------------------------------------------------------------------
// From chunk 0 along the JOINED links to FINAL.  kept = the chunks on the walk, off[i] = the output
// byte at which kept[i] starts, off[kept.size()] = the total.  False (declined): a decoder on the
// walk failed, the total is not expect, or bytes follow the final block.  Every link points to a
// later chunk, so the walk ends.
inline bool chain_walk(const DecRec *rec, uint32_t nchunks, uint64_t n, uint64_t expect, std::vector<uint32_t> &kept,
                       std::vector<uint64_t> &off, Stats &st) {
    kept.clear(), off.clear();
    uint64_t total = 0;
    st.candidates = st.stored_blocks = st.fixed_blocks = st.dynamic_blocks = 0;
    for (uint32_t c = 1; c < nchunks; ++c) st.candidates += rec[c].status != S_IDLE;
    bool ok = false;
    for (uint32_t c = 0; c < nchunks;) {
        const DecRec &R = rec[c];
        if (R.status != S_FINAL && R.status != S_JOINED) break;
        kept.push_back(c), off.push_back(total);
        total += R.bytes;
        st.stored_blocks += R.blocks[0], st.fixed_blocks += R.blocks[1], st.dynamic_blocks += R.blocks[2];
        if (R.status == S_FINAL) {
            ok = (R.end + 7) / 8 == n;
            break;
        }
        if (R.link <= c) break;
        c = R.link;
    }
    off.push_back(total);
    st.chunks = nchunks;
    st.kept = kept.size();
    st.discarded = 1 + st.candidates - st.kept;
    st.markers = 0;
    return ok && total == expect;
}

inline uint32_t chunk_count(uint64_t n, uint32_t chunk_bytes) { return n ? (uint32_t)((n + chunk_bytes - 1) / chunk_bytes) : 1u; }

// ---- the whole method, serially (host) ----------------------------------------------------------------
// The raw deflate stream in[0..n) into out[0..expect) by the device's steps in the device's order.
// False = declined; out then holds nothing promised.  No byte outside out[0..expect) is written.
inline bool inflate_chunked(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t expect, uint32_t chunk_bytes, Stats &st) {
    st = Stats{};
    if (chunk_bytes == 0) chunk_bytes = CHUNK_DEFAULT;
    if (chunk_bytes < CHUNK_MIN || n == 0 || n >= (1ull << 40) || (n + chunk_bytes - 1) / chunk_bytes >= (1ull << 31)) return false;
    const uint32_t nchunks = chunk_count(n, chunk_bytes);
    // 1. find
    std::vector<uint64_t> cand(nchunks, NONE);
    cand[0] = 0;
    for (uint32_t c = 1; c < nchunks; ++c) {
        uint64_t lo, hi;
        chunk_bits(n, chunk_bytes, c, lo, hi);
        cand[c] = find_candidate(in, n, lo, hi);
    }
    // 2. size pass
    std::vector<uint8_t> tab(TABLE_BYTES);
    Tables T = tables_at(tab.data());
    std::vector<DecRec> rec(nchunks);
    for (uint32_t c = 0; c < nchunks; ++c) size_decoder(in, n, cand.data(), nchunks, c, expect, chunk_bytes, T, rec[c]);
    // 3. chain
    std::vector<uint32_t> kept;
    std::vector<uint64_t> off;
    if (!chain_walk(rec.data(), nchunks, n, expect, kept, off, st)) return false;
    // 4. write pass
    std::vector<uint16_t> sym(expect ? expect : 1);
    for (size_t i = 0; i < kept.size(); ++i) {
        DecRec &R = rec[kept[i]];
        write_decoder(in, n, sym.data() + off[i], off[i], chunk_bytes, T, R);
        if (!R.wrote) return false;
        st.markers += R.markers;
    }
    // 5. windows: the last WIN bytes of every kept chunk, in order (a shorter chunk's window is
    // completed by the one before it, which already stands in out)
    for (size_t i = 0; i < kept.size(); ++i) {
        const uint64_t end = off[i + 1], from = end - off[i] > WIN ? end - WIN : off[i];
        for (uint64_t q = from; q < end; ++q) out[q] = resolve_sym(sym[q], out, off[i]);
    }
    // 6. resolve: everything before those tails
    for (size_t i = 0; i < kept.size(); ++i) {
        const uint64_t end = off[i + 1];
        for (uint64_t q = off[i]; q + WIN < end; ++q) out[q] = resolve_sym(sym[q], out, off[i]);
    }
    return true;
}

// the first `want` bytes of the raw deflate stream in[0..n), serially: *got = how many there are
// (fewer when the stream ends first).  False: the stream is broken before them.
inline bool inflate_head(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t want, uint64_t *got) {
    std::vector<uint8_t> tab(TABLE_BYTES);
    Tables T = tables_at(tab.data());
    Bits b;
    bits_at(b, in, n, 0);
    HeadSink s{out, 0, want, want == 0};
    *got = 0;
    if (s.full) return true;
    for (uint64_t k = max_blocks(n); k; --k) {
        bool final = false;
        uint32_t btype = 0;
        uint64_t budget = ~0ull;
        const bool ok = decode_block(b, T, s, budget, final, btype);
        if (s.full) break;
        if (!ok) return false;
        if (final) break;
    }
    *got = s.j < want ? s.j : want;
    return true;
}

// ---- the gzip member (RFC 1952), host ------------------------------------------------------------------
struct Member {
    uint64_t stream_off, stream_len;
    uint32_t crc, isize;
};
// The header of a member whose first `avail` bytes are at p: *hdr = its length.  False (declined):
// no gzip magic, a method other than 8, reserved FLG bits, a header that does not end inside
// `avail`.  FEXTRA, FNAME, FCOMMENT and FHCRC are stepped over (the header CRC is not checked).
inline bool member_header(const uint8_t *p, uint64_t avail, uint64_t *hdr) {
    if (avail < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return false;
    const uint32_t flg = p[3];
    if (flg & 0xe0u) return false;
    uint64_t o = 10;
    if (flg & 4u) {
        if (o + 2 > avail) return false;
        o += 2 + ((uint64_t)p[o] | (uint64_t)p[o + 1] << 8);
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1)  // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (o < avail && p[o]) ++o;
            ++o;
        }
    if (flg & 2u) o += 2;
    if (o > avail) return false;
    *hdr = o;
    return true;
}
// the member of n bytes with that header and the trailer at tail8: the stream is what lies between
// (two bytes at least)
inline bool member_of(uint64_t hdr, const uint8_t *tail8, uint64_t n, Member &M) {
    if (hdr > n || n - hdr < 8 + 2) return false;
    M.stream_off = hdr;
    M.stream_len = n - hdr - 8;
    M.crc = (uint32_t)tail8[0] | (uint32_t)tail8[1] << 8 | (uint32_t)tail8[2] << 16 | (uint32_t)tail8[3] << 24;
    M.isize = (uint32_t)tail8[4] | (uint32_t)tail8[5] << 8 | (uint32_t)tail8[6] << 16 | (uint32_t)tail8[7] << 24;
    return true;
}
inline bool member_layout(const uint8_t *p, uint64_t n, Member &M) {
    uint64_t hdr = 0;
    return n >= 18 && member_header(p, n, &hdr) && member_of(hdr, p + n - 8, n, M);
}

}  // namespace infl
}  // namespace st
