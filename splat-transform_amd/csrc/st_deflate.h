// st_deflate.h -- the DEFLATE (RFC 1951) encoder of include/st_abi.h, "the gzip member around a
// .spz image": the pieces that the kernels (st_deflate.hip) and a host program share, all
// __host__ __device__, and a serial whole-segment encoder made of nothing else, so a host program
// produces the stream that the device produces, byte for byte
// (tests/native/deflate_cpu_check.cpp).
//
//   token_at         the token of one position from its run: (offset in the run, run length)
//   len_symbol       match length -> length symbol, extra-bit count and value
//   code_lengths     counts -> length-limited code lengths, from the used symbols in
//                    (count, symbol) order: rank_of gives a symbol's place, so a wave ranks all
//                    symbols at once and one lane merges
//   canonical_codes  lengths -> canonical codes, bit-reversed for the LSB-first stream
//   plan_segment     a segment's histogram -> its three sizes, the choice, the code table and the
//                    block header bits
//   encode_segment / encode_stream   the serial encoder
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

namespace st {
namespace defl {

// ST_DEFLATE_SEG: the bytes of the stream depend on it.  ST_DEFL_SEG_TRIAL builds a library with
// another segment size (16 to 64 KiB) to be measured beside this one (tools/bench_spz_deflate.py)
#ifdef ST_DEFL_SEG_TRIAL
constexpr uint32_t SEG = ST_DEFL_SEG_TRIAL;
#else
constexpr uint32_t SEG = 65536;
#endif
constexpr uint32_t STORED_MAX = 65535;
constexpr int NLIT = 286, NCL = 19, LIT_LIMIT = 15, CL_LIMIT = 7, EOB = 256;
constexpr int HDR_WORDS = 80;        // a dynamic block's header is at most 3 + 14 + 57 + 288 * 7 = 2,090 bits

// ---- tokens ------------------------------------------------------------------------------------
// the token that starts at offset o of a maximal run of L equal bytes: 0 = none (the position is
// inside a match), 1 = a literal, 3..258 = a match of that length at distance 1.  The run's first
// byte is a literal, the other L - 1 are cut greedily into matches of 258, a remainder of at
// least 3 is one match, a remainder of 1 or 2 is literals.
__host__ __device__ inline uint32_t token_at(uint32_t o, uint32_t L) {
    if (o == 0 || L <= 3) return 1;
    const uint32_t k = o - 1, R = L - 1;
    const uint32_t full = R / 258, rem = R - full * 258;
    const uint32_t q = k / 258, r = k - q * 258;
    if (q < full) return r == 0 ? 258u : 0u;
    if (rem >= 3) return r == 0 ? rem : 0u;
    return 1;
}

// length 3..258 -> symbol 257..285; *ebits extra bits of value *eval (RFC 1951 3.2.5)
__host__ __device__ inline uint32_t len_symbol(uint32_t len, uint32_t *ebits, uint32_t *eval) {
    const uint32_t l = len - 3;
    if (l < 8 || len == 258) {
        *ebits = 0, *eval = 0;
        return len == 258 ? 285u : 257u + l;
    }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    *ebits = e;
    *eval = l & ((1u << e) - 1u);
    return 257u + 4u * e + (l >> e);
}
// the extra bits of length symbol s (257..285)
__host__ __device__ inline uint32_t len_extra_bits(uint32_t s) {
    const uint32_t i = s - 257u;
    return i < 8 || i == 28 ? 0u : (i >> 2) - 1u;
}
// the fixed code of literal/length symbol s (RFC 1951 3.2.6): length << 16 | code bit-reversed
__host__ __device__ inline uint32_t bit_reverse(uint32_t c, uint32_t n) { return __builtin_bitreverse32(c) >> (32 - n); }
__host__ __device__ inline uint32_t fixed_length(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
__host__ __device__ inline uint32_t fixed_entry(uint32_t s) {
    const uint32_t n = fixed_length(s);
    const uint32_t c = s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? s - 256 : 0xC0u + (s - 280);
    return n << 16 | bit_reverse(c, n);
}

// ---- the code builder --------------------------------------------------------------------------
// the place of used symbol s among the used symbols in (count, symbol) order
__host__ __device__ inline uint32_t rank_of(const uint32_t *cnt, int n, int s) {
    const uint32_t c = cnt[s];
    uint32_t r = 0;
    for (int t = 0; t < n; ++t) {
        const uint32_t d = cnt[t];
        r += d != 0 && (d < c || (d == c && t < s));
    }
    return r;
}
// order[rank] = symbol for every used symbol; returns how many are used (the serial form)
__host__ __device__ inline int sort_used(const uint32_t *cnt, int n, uint16_t *order) {
    int m = 0;
    for (int s = 0; s < n; ++s)
        if (cnt[s]) order[rank_of(cnt, n, s)] = (uint16_t)s, ++m;
    return m;
}

// Huffman's tree over the m >= 2 used symbols in `order`, whose counts are lw[0..m) (the sorted
// weights, gathered once), every count raised to at least `floor_`:
// two queues, the sorted leaves and the internal nodes in the order they are made; of two equal
// weights the internal node goes first (every such choice costs the same bits; this one gives the
// deepest of those trees, and the limit below is then the one place that decides the depth).
// w: m words, par: 2m entries.  len[symbol] = depth; returns the greatest depth.
__host__ __device__ inline uint32_t huffman_depths(const uint32_t *lw_, const uint16_t *order, int m, uint32_t floor_,
                                                   uint32_t *w, uint16_t *par, uint8_t *len) {
    int li = 0, ii = 0;
    for (int ni = 0; ni < m - 1; ++ni) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; ++k) {
            uint32_t lw = 0;
            if (li < m) {
                lw = lw_[li];
                if (lw < floor_) lw = floor_;
            }
            if (li < m && (ii >= ni || lw < w[ii])) {
                sum += lw;
                par[li++] = (uint16_t)(m + ni);
            } else {
                sum += w[ii];
                par[m + ii] = (uint16_t)(m + ni);
                ++ii;
            }
        }
        w[ni] = sum;
    }
    // depths of the internal nodes from the root down, kept where their weights were
    w[m - 2] = 0;
    for (int j = m - 3; j >= 0; --j) w[j] = w[par[m + j] - m] + 1;
    uint32_t deepest = 0;
    for (int i = 0; i < m; ++i) {
        const uint32_t d = w[par[i] - m] + 1;
        len[order[i]] = (uint8_t)d;
        if (d > deepest) deepest = d;
    }
    return deepest;
}

// code lengths of at most `limit` bits for an alphabet of n >= 2 symbols, from order[0..m) = the used
// symbols in (count, symbol) order and lw[0..m) = their counts in that order.  Huffman's lengths
// where they fit; else small counts are raised to a floor that doubles from
// max(2, total >> (limit + 2)) until the tree fits -- still a full tree, so the code is complete (Kraft sum exactly 1).  One used symbol: it and the lowest other symbol get
// length 1, the way zlib avoids a one-symbol code; that partner is the only unused symbol whose
// length is not 0.  m = 0: all 0.  Counts are at most 2^20 each (the sums stay in 32 bits).
// Returns the greatest depth of the unlimited tree.
__host__ __device__ inline uint32_t code_lengths(const uint32_t *lw, int n, const uint16_t *order, int m, uint32_t limit,
                                                 uint32_t *w, uint16_t *par, uint8_t *len) {
    for (int s = 0; s < n; ++s) len[s] = 0;
    if (m == 0) return 0;
    if (m == 1) {
        len[order[0]] = 1;
        len[order[0] == 0 ? 1 : 0] = 1;
        return 1;
    }
    const uint32_t free_depth = huffman_depths(lw, order, m, 1, w, par, len);
    if (free_depth > limit) {
        uint32_t total = 0;
        for (int i = 0; i < m; ++i) total += lw[i];
        uint32_t floor_ = total >> (limit + 2);
        if (floor_ < 2) floor_ = 2;
        while (huffman_depths(lw, order, m, floor_, w, par, len) > limit) floor_ *= 2;
    }
    return free_depth;
}

// canonical codes of len[0..n) (RFC 1951 3.2.2): tab[s] = len << 16 | the code bit-reversed; scr: 34 words
__host__ __device__ inline void canonical_codes(const uint8_t *len, int n, uint32_t *tab, uint32_t *scr) {
    uint32_t *bl = scr, *next = scr + 17;
    for (int b = 0; b < 34; ++b) scr[b] = 0;
    for (int s = 0; s < n; ++s) bl[len[s]]++;
    bl[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= 16; ++b) {
        code = (code + bl[b - 1]) << 1;
        next[b] = code;
    }
    for (int s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        tab[s] = l ? l << 16 | bit_reverse(next[l]++, l) : 0u;
    }
}

// ---- bits --------------------------------------------------------------------------------------
// LSB-first bits into zeroed 32-bit words
struct WordBits {
    uint32_t *w;
    uint32_t nbits;
    __host__ __device__ void put(uint32_t v, uint32_t n) {
        if (!n) return;
        const uint32_t i = nbits >> 5, sh = nbits & 31u;
        w[i] |= v << sh;
        if (sh + n > 32) w[i + 1] |= v >> (32 - sh);
        nbits += n;
    }
};

// the code lengths lens[0..total) as code-length-code tokens (RFC 1951 3.2.7), one sequence over
// the literal/length and distance lengths: f(symbol, extra bits, extra value).  A run of zeros is
// cut greedily into 18s (11..138), then a 17 (3..10), then single 0s; a run of another length is
// that length once, then 16s (3..6), then the length again for what is left.
template <class F>
__host__ __device__ inline void cl_tokens(const uint8_t *lens, int total, F f) {
    for (int i = 0; i < total;) {
        const uint32_t v = lens[i];
        int run = 1;
        while (i + run < total && lens[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 3) {
                const int t = run > 138 ? 138 : run;
                if (t >= 11) f(18u, 7u, (uint32_t)(t - 11));
                else f(17u, 3u, (uint32_t)(t - 3));
                run -= t;
            }
        } else {
            f(v, 0u, 0u);
            --run;
            while (run >= 3) {
                const int t = run > 6 ? 6 : run;
                f(16u, 2u, (uint32_t)(t - 3));
                run -= t;
            }
        }
        for (; run > 0; --run) f(v, 0u, 0u);
    }
}

// ---- a segment's plan ----------------------------------------------------------------------------
struct Work {
    uint32_t w[NLIT];
    uint16_t par[2 * NLIT];
    uint16_t order[NLIT];
    uint8_t lens[NLIT + 2];  // literal/length lengths, then the two distance lengths
    uint32_t lw[NLIT];       // the used symbols' counts in `order`
    uint32_t clcnt[NCL], cltab[NCL], scr[34];
    uint16_t clorder[NCL];
    uint8_t cllen[NCL];
};
struct Plan {
    uint32_t btype;     // 0 stored, 1 fixed, 2 dynamic
    uint32_t bytes;     // the segment's bytes in the stream, its byte-boundary trailer included
    uint32_t hdr_bits;  // block header bits in hdr[] (btype 1: 3, btype 2: 3 + the code description)
    uint32_t bits;      // btype 1, 2: header + tokens + end-of-block
    uint32_t dist_bits; // bits of the distance symbol: 5 fixed, 1 dynamic (the code is all zeros)
    uint32_t free_depth;  // the deepest literal/length leaf before the 15-bit limit (recorded by tests)
};

__host__ __device__ inline uint32_t stored_bytes(uint32_t n) { return n + 5u * ((n + STORED_MAX - 1) / STORED_MAX); }
// bytes of a fixed or dynamic block of `bits` bits once it ends on a byte boundary: the last
// segment pads with zeros; any other is followed by an empty stored block (000, padding, 00 00 FF FF)
__host__ __device__ inline uint32_t coded_bytes(uint32_t bits, bool final) {
    return final ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
}

// the order in which a dynamic block lists its code-length-code lengths (RFC 1951 3.2.7)
__host__ __device__ inline uint32_t cl_order(int i) {
    const uint8_t o[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// cnt[0..286): the histogram of a segment of n >= 1 bytes, end-of-block counted once; order[0..m):
// its used symbols in (count, symbol) order (in W.order) and W.lw[0..m) their counts in that order.  tab[0..286): the chosen code (btype 1, 2);
// hdr[0..HDR_WORDS): the block header bits.  The smallest of the three codings, ties to the simpler.
__host__ __device__ inline void plan_segment(const uint32_t *cnt, uint32_t n, bool final, int m, Work &W, uint32_t *tab,
                                             uint32_t *hdr, Plan &P) {
    // dynamic: the code, then its description
    P.free_depth = code_lengths(W.lw, NLIT, W.order, m, LIT_LIMIT, W.w, W.par, W.lens);
    int hlit = NLIT;
    while (hlit > 257 && W.lens[hlit - 1] == 0) --hlit;
    W.lens[hlit] = W.lens[hlit + 1] = 1;  // distance symbols 0 and 1: part of the described sequence, not of the code
    const int total = hlit + 2;
    for (int i = 0; i < NCL; ++i) W.clcnt[i] = 0;
    uint32_t *clcnt = W.clcnt;
    cl_tokens(W.lens, total, [clcnt](uint32_t s, uint32_t, uint32_t) { ++clcnt[s]; });
    const int clm = sort_used(W.clcnt, NCL, W.clorder);
    uint32_t *cllw = W.scr;  // (NCL <= 34 words; canonical_codes takes them over afterwards)
    for (int i = 0; i < clm; ++i) cllw[i] = W.clcnt[W.clorder[i]];
    code_lengths(cllw, NCL, W.clorder, clm, CL_LIMIT, W.w, W.par, W.cllen);
    canonical_codes(W.cllen, NCL, W.cltab, W.scr);
    int hclen = NCL;
    while (hclen > 4 && W.cllen[cl_order(hclen - 1)] == 0) --hclen;
    uint32_t dyn = 3 + 14 + 3 * (uint32_t)hclen, fix = 3;
    for (int s = 0; s < NCL; ++s) dyn += W.clcnt[s] * (W.cllen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    const uint32_t dyn_hdr = dyn;
    for (int s = 0; s < NLIT; ++s) {
        const uint32_t e = s > EOB ? len_extra_bits(s) : 0u;
        dyn += cnt[s] * (W.lens[s] + e + (s > EOB ? 1u : 0u));
        fix += cnt[s] * (fixed_length(s) + e + (s > EOB ? 5u : 0u));
    }
    const uint32_t sb = stored_bytes(n), fb = coded_bytes(fix, final), db = coded_bytes(dyn, final);
    for (int i = 0; i < HDR_WORDS; ++i) hdr[i] = 0;
    WordBits hb{hdr, 0};
    if (sb <= fb && sb <= db) {
        P.btype = 0, P.bytes = sb, P.hdr_bits = 0, P.bits = 0, P.dist_bits = 0;
    } else if (fb <= db) {
        P.btype = 1, P.bytes = fb, P.hdr_bits = 3, P.bits = fix, P.dist_bits = 5;
        hb.put(final ? 1u : 0u, 1), hb.put(1, 2);
        for (int s = 0; s < NLIT; ++s) tab[s] = fixed_entry(s);
    } else {
        P.btype = 2, P.bytes = db, P.hdr_bits = dyn_hdr, P.bits = dyn, P.dist_bits = 1;
        hb.put(final ? 1u : 0u, 1), hb.put(2, 2);
        hb.put((uint32_t)hlit - 257, 5), hb.put(1, 5), hb.put((uint32_t)hclen - 4, 4);
        for (int i = 0; i < hclen; ++i) hb.put(W.cllen[cl_order(i)], 3);
        const uint32_t *cltab = W.cltab;
        WordBits *hp = &hb;
        cl_tokens(W.lens, total, [cltab, hp](uint32_t s, uint32_t eb, uint32_t ev) {
            hp->put(cltab[s] & 0xffffu, cltab[s] >> 16);
            hp->put(ev, eb);
        });
        // the literal/length code is its hlit lengths alone: the two distance lengths behind them in
        // W.lens belong to another code and must not enter the count of codes per length
        canonical_codes(W.lens, hlit, tab, W.scr);
        for (int s = hlit; s < NLIT; ++s) tab[s] = 0;
    }
}

// ---- sizes ---------------------------------------------------------------------------------------
// the all-stored size, the stream's worst case
__host__ __device__ inline uint64_t deflate_bound(uint64_t n) {
    if (n == 0) return 2;
    const uint64_t full = n / SEG;
    const uint32_t rest = (uint32_t)(n - full * SEG);
    return full * stored_bytes(SEG) + (rest ? stored_bytes(rest) : 0);
}
__host__ __device__ inline uint64_t gzip_bound(uint64_t n) { return deflate_bound(n) + 18; }

// ---- the serial encoder --------------------------------------------------------------------------
// LSB-first bits into bytes
struct ByteBits {
    uint8_t *p;
    uint64_t acc = 0;
    uint32_t nacc = 0;
    __host__ __device__ void put(uint32_t v, uint32_t n) {
        acc |= (uint64_t)v << nacc;
        nacc += n;
        while (nacc >= 8) *p++ = (uint8_t)acc, acc >>= 8, nacc -= 8;
    }
    __host__ __device__ void align() {
        if (nacc) *p++ = (uint8_t)acc, acc = 0, nacc = 0;
    }
};

// the length of the maximal run that starts at in[s] inside in[0..n)
__host__ __device__ inline uint32_t run_length(const uint8_t *in, uint32_t n, uint32_t s) {
    uint32_t e = s + 1;
    while (e < n && in[e] == in[s]) ++e;
    return e - s;
}

// one segment in[0..n), 1 <= n <= SEG, to out; returns its bytes (P.bytes)
__host__ __device__ inline uint32_t encode_segment(const uint8_t *in, uint32_t n, bool final, uint8_t *out, Work &W,
                                                   uint32_t *cnt, uint32_t *tab, uint32_t *hdr, Plan &P) {
    for (int s = 0; s < NLIT; ++s) cnt[s] = 0;
    cnt[EOB] = 1;
    for (uint32_t s = 0; s < n;) {
        const uint32_t L = run_length(in, n, s);
        for (uint32_t o = 0; o < L; ++o) {
            const uint32_t t = token_at(o, L);
            uint32_t eb, ev;
            if (t == 1) ++cnt[in[s]];
            else if (t) ++cnt[len_symbol(t, &eb, &ev)];
        }
        s += L;
    }
    const int m = sort_used(cnt, NLIT, W.order);
    for (int i = 0; i < m; ++i) W.lw[i] = cnt[W.order[i]];
    plan_segment(cnt, n, final, m, W, tab, hdr, P);
    if (P.btype == 0) {
        uint8_t *o = out;
        for (uint32_t b = 0; b < n; b += STORED_MAX) {
            const uint32_t len = n - b < STORED_MAX ? n - b : STORED_MAX;
            *o++ = final && b + len == n ? 1 : 0;
            *o++ = (uint8_t)len, *o++ = (uint8_t)(len >> 8), *o++ = (uint8_t)~len, *o++ = (uint8_t)(~len >> 8);
            for (uint32_t i = 0; i < len; ++i) *o++ = in[b + i];
        }
        return P.bytes;
    }
    ByteBits bb{out};
    for (uint32_t b = 0; b < P.hdr_bits; b += 32) bb.put(hdr[b >> 5], P.hdr_bits - b < 32 ? P.hdr_bits - b : 32);
    for (uint32_t s = 0; s < n;) {
        const uint32_t L = run_length(in, n, s);
        for (uint32_t o = 0; o < L; ++o) {
            const uint32_t t = token_at(o, L);
            if (t == 1) {
                bb.put(tab[in[s]] & 0xffffu, tab[in[s]] >> 16);
            } else if (t) {
                uint32_t eb, ev;
                const uint32_t e = tab[len_symbol(t, &eb, &ev)];
                bb.put(e & 0xffffu, e >> 16);
                bb.put(ev, eb);
                bb.put(0, P.dist_bits);
            }
        }
        s += L;
    }
    bb.put(tab[EOB] & 0xffffu, tab[EOB] >> 16);
    if (!final) {
        bb.put(0, 3);
        bb.align();
        *bb.p++ = 0, *bb.p++ = 0, *bb.p++ = 0xff, *bb.p++ = 0xff;
    } else {
        bb.align();
    }
    return P.bytes;
}

// the whole stream of in[0..n) to out (deflate_bound(n) bytes of room); returns its size
inline uint64_t encode_stream(const uint8_t *in, uint64_t n, uint8_t *out) {
    if (n == 0) {
        out[0] = 3, out[1] = 0;
        return 2;
    }
    Work W;
    Plan P;
    uint32_t cnt[NLIT], tab[NLIT], hdr[HDR_WORDS];
    uint64_t o = 0;
    for (uint64_t b = 0; b < n; b += SEG) {
        const uint32_t len = n - b < SEG ? (uint32_t)(n - b) : SEG;
        o += encode_segment(in + b, len, b + len == n, out + o, W, cnt, tab, hdr, P);
    }
    return o;
}

}  // namespace defl
}  // namespace st
