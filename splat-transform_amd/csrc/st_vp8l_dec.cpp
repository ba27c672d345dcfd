// st_vp8l_dec.cpp -- WebP lossless (VP8L) decoder on the host, written from RFC 9649.
//
// The reader of .sog inputs (st_sog_read.hip) decodes the seven textures with it; the files come
// from libwebp (the reference's writer) as well as from this library's encoder (st_vp8l.cpp,
// st_webp.hip), so the whole format is covered:
//
//   container   RIFF....WEBP with a VP8L chunk, alone or inside a VP8X file (RFC 9649 2.5-2.7);
//               a lossy "VP8 " chunk is ST_ERR_UNSUPPORTED
//   header      signature 0x2f, 14-bit width-1 / height-1, alpha hint, 3-bit version 0      (3.2)
//   transforms  predictor (14 modes, top row = L, left column = T, pixel 0 = opaque black),
//               cross-colour, subtract-green, colour-indexing with 8/4/2 pixels bundled per
//               green byte for <= 2/4/16 colours; each at most once, undone in reverse order (4)
//   image data  colour cache of 1..11 bits, meta prefix codes (entropy image), simple and normal
//               prefix-code descriptions (code-length code order, repeat codes 16/17/18,
//               max_symbol, one-symbol codes of zero bits), LZ77 length / distance prefix coding
//               with the 120-entry short-distance map                                        (5, 6)
//
// Prefix codes decode through a two-level table: 8 root bits, second-level tables for longer
// codes.  The bit reader never reads past the buffer: bits past the end read as zero and raise
// `eos`, which every loop checks.  A truncated or corrupt stream returns ST_ERR_ARG (incomplete or
// over-subscribed code lengths, a distance before the start, a transform repeated, a cache index
// past the cache); nothing asserts and nothing is read or written out of bounds.
//
// Plain C++ (no HIP): tests/native/sog_read_cpu_check.cpp compiles this file alone, under
// AddressSanitizer, and supplies st::set_last_error itself.
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/st_abi.h"

namespace st {
void set_last_error(const std::string &msg);

namespace vp8l_dec {
namespace {

struct Fail {
    int code;
    std::string msg;
};
[[noreturn]] void fail(const char *m) { throw Fail{ST_ERR_ARG, std::string("webp: ") + m}; }

uint32_t le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// LSB-first bit reader over [p, p + n)
struct BitReader {
    const uint8_t *p;
    uint64_t n, pos = 0;  // pos: bytes loaded so far (zero bytes once past n)
    uint64_t acc = 0;
    int nacc = 0;
    BitReader(const uint8_t *data, uint64_t len) : p(data), n(len) {}
    void fill() {
        while (nacc <= 56) {
            if (pos < n) acc |= (uint64_t)p[pos] << nacc;
            ++pos;
            nacc += 8;
        }
    }
    // up to 32 bits, without consuming
    uint32_t peek(int nb) {
        if (nacc < nb) fill();
        return (uint32_t)(acc & ((1ull << nb) - 1));
    }
    void drop(int nb) {
        acc >>= nb;
        nacc -= nb;
    }
    uint32_t bits(int nb) {
        if (nb == 0) return 0;
        const uint32_t v = peek(nb);
        drop(nb);
        return v;
    }
    // true once a consumed bit lay past the end of the buffer
    bool past_end() const { return pos > n && (pos - n) * 8 > (uint64_t)nacc; }
};

constexpr int kRootBits = 8;
constexpr int kMaxLen = 15;
constexpr int kCodeLengthCodes = 19;
const uint8_t kCodeLengthOrder[kCodeLengthCodes] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// one prefix code.  Root entries: len <= kRootBits -> (symbol << 8) | len; a longer code's root
// entry links its second-level table: kLink | (offset << 8) | sub_bits
struct Code {
    std::vector<uint32_t> tab;
    bool single = false;  // one symbol: no bits
    uint32_t symbol = 0;
    static constexpr uint32_t kLink = 0x80000000u;

    // len[0..n): canonical code lengths; a complete code, or exactly one symbol
    void build(const uint8_t *len, int n) {
        int count[kMaxLen + 1] = {0};
        int used = 0, last = 0;
        for (int s = 0; s < n; ++s) {
            if (len[s] > kMaxLen) fail("bad code length");
            if (len[s]) {
                ++count[len[s]];
                ++used;
                last = s;
            }
        }
        if (used == 0) fail("prefix code without symbols");
        if (used == 1) {
            single = true;
            symbol = (uint32_t)last;
            return;
        }
        // Kraft: the lengths must fill the code space exactly
        uint32_t space = 0;
        for (int l = 1; l <= kMaxLen; ++l) space += (uint32_t)count[l] << (kMaxLen - l);
        if (space != (1u << kMaxLen)) fail("incomplete or over-subscribed prefix code");
        uint32_t next[kMaxLen + 2] = {0};
        {
            uint32_t c = 0;
            for (int l = 1; l <= kMaxLen; ++l) {
                c = (c + (uint32_t)count[l - 1]) << 1;
                next[l] = c;
            }
        }
        // per symbol: the code's bits reversed (the stream is LSB-first, codes MSB-first)
        std::vector<uint16_t> rev((size_t)n);
        for (int s = 0; s < n; ++s) {
            const int l = len[s];
            if (!l) continue;
            uint32_t c = next[l]++, r = 0;
            for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);
            rev[s] = (uint16_t)r;
        }
        // second-level sizes: the longest code under each root prefix
        uint8_t sub[1 << kRootBits] = {0};
        for (int s = 0; s < n; ++s)
            if (len[s] > kRootBits) {
                const uint32_t root = rev[s] & ((1u << kRootBits) - 1);
                const uint8_t need = (uint8_t)(len[s] - kRootBits);
                if (need > sub[root]) sub[root] = need;
            }
        size_t total = (size_t)1 << kRootBits;
        uint32_t off[1 << kRootBits];
        for (int r = 0; r < (1 << kRootBits); ++r) {
            off[r] = (uint32_t)total;
            if (sub[r]) total += (size_t)1 << sub[r];
        }
        tab.assign(total, 0);
        for (int r = 0; r < (1 << kRootBits); ++r)
            if (sub[r]) tab[r] = kLink | (off[r] << 8) | sub[r];
        for (int s = 0; s < n; ++s) {
            const int l = len[s];
            if (!l) continue;
            if (l <= kRootBits) {
                for (uint32_t k = rev[s]; k < (1u << kRootBits); k += 1u << l) tab[k] = ((uint32_t)s << 8) | (uint32_t)l;
            } else {
                const uint32_t root = rev[s] & ((1u << kRootBits) - 1), hi = rev[s] >> kRootBits;
                const int sl = l - kRootBits;
                for (uint32_t k = hi; k < (1u << sub[root]); k += 1u << sl)
                    tab[off[root] + k] = ((uint32_t)s << 8) | (uint32_t)sl;
            }
        }
    }

    uint32_t read(BitReader &br) const {
        if (single) return symbol;
        uint32_t e = tab[br.peek(kRootBits)];
        if (e & kLink) {
            br.drop(kRootBits);
            const uint32_t o = (e & 0x7fffffffu) >> 8, sb = e & 0xffu;
            e = tab[o + br.peek((int)sb)];
        }
        // a complete code leaves no empty entry, so e's length is 1..15 here
        br.drop((int)(e & 0xffu));
        return e >> 8;
    }
};

// the description of one prefix code over `alphabet` symbols (RFC 9649 6.2.1)
void read_code(BitReader &br, int alphabet, Code &out, std::vector<uint8_t> &len) {
    len.assign((size_t)alphabet, 0);
    if (br.bits(1)) {  // simple: one or two symbols
        const int nsym = (int)br.bits(1) + 1;
        const uint32_t s0 = br.bits(br.bits(1) ? 8 : 1);
        if ((int)s0 >= alphabet) fail("simple code symbol outside the alphabet");
        len[s0] = 1;
        if (nsym == 2) {
            const uint32_t s1 = br.bits(8);
            if ((int)s1 >= alphabet) fail("simple code symbol outside the alphabet");
            len[s1] = 1;
        }
    } else {
        uint8_t cl[kCodeLengthCodes] = {0};
        const int ncl = 4 + (int)br.bits(4);
        for (int i = 0; i < ncl; ++i) cl[kCodeLengthOrder[i]] = (uint8_t)br.bits(3);
        Code clc;
        clc.build(cl, kCodeLengthCodes);
        int max_symbol = alphabet;
        if (br.bits(1)) {
            const int nb = 2 + 2 * (int)br.bits(3);
            max_symbol = 2 + (int)br.bits(nb);
            if (max_symbol > alphabet) fail("max_symbol above the alphabet");
        }
        int s = 0;
        uint8_t prev = 8;
        while (s < alphabet) {
            if (max_symbol-- == 0) break;
            if (br.past_end()) fail("truncated prefix code");
            const uint32_t c = clc.read(br);
            if (c < 16) {
                len[s++] = (uint8_t)c;
                if (c) prev = (uint8_t)c;
            } else {
                const int rep = c == 16 ? 3 + (int)br.bits(2) : c == 17 ? 3 + (int)br.bits(3) : 11 + (int)br.bits(7);
                if (s + rep > alphabet) fail("code length repeat past the alphabet");
                const uint8_t v = c == 16 ? prev : 0;
                for (int k = 0; k < rep; ++k) len[s++] = v;
            }
        }
    }
    if (br.past_end()) fail("truncated prefix code");
    out = Code();
    out.build(len.data(), alphabet);
}

struct Group {
    Code c[5];  // green + length prefixes + cache, red, blue, alpha, distance
};

const int8_t kDistMap[120][2] = {
    {0, 1},  {1, 0},  {1, 1},  {-1, 1}, {0, 2},  {2, 0},  {1, 2},  {-1, 2}, {2, 1},  {-2, 1}, {2, 2},  {-2, 2},
    {0, 3},  {3, 0},  {1, 3},  {-1, 3}, {3, 1},  {-3, 1}, {2, 3},  {-2, 3}, {3, 2},  {-3, 2}, {0, 4},  {4, 0},
    {1, 4},  {-1, 4}, {4, 1},  {-4, 1}, {3, 3},  {-3, 3}, {2, 4},  {-2, 4}, {4, 2},  {-4, 2}, {0, 5},  {3, 4},
    {-3, 4}, {4, 3},  {-4, 3}, {5, 0},  {1, 5},  {-1, 5}, {5, 1},  {-5, 1}, {2, 5},  {-2, 5}, {5, 2},  {-5, 2},
    {4, 4},  {-4, 4}, {3, 5},  {-3, 5}, {5, 3},  {-5, 3}, {0, 6},  {6, 0},  {1, 6},  {-1, 6}, {6, 1},  {-6, 1},
    {2, 6},  {-2, 6}, {6, 2},  {-6, 2}, {4, 5},  {-4, 5}, {5, 4},  {-5, 4}, {3, 6},  {-3, 6}, {6, 3},  {-6, 3},
    {0, 7},  {7, 0},  {1, 7},  {-1, 7}, {5, 5},  {-5, 5}, {7, 1},  {-7, 1}, {4, 6},  {-4, 6}, {6, 4},  {-6, 4},
    {2, 7},  {-2, 7}, {7, 2},  {-7, 2}, {3, 7},  {-3, 7}, {7, 3},  {-7, 3}, {5, 6},  {-5, 6}, {6, 5},  {-6, 5},
    {8, 0},  {4, 7},  {-4, 7}, {7, 4},  {-7, 4}, {8, 1},  {8, 2},  {6, 6},  {-6, 6}, {8, 3},  {5, 7},  {-5, 7},
    {7, 5},  {-7, 5}, {8, 4},  {6, 7},  {-6, 7}, {7, 6},  {-7, 6}, {8, 5},  {7, 7},  {-7, 7}, {8, 6},  {8, 7}};

// the value of an LZ77 length or distance prefix symbol (RFC 9649 5.2.2)
uint32_t prefix_value(BitReader &br, uint32_t sym) {
    if (sym < 4) return sym + 1;
    const int extra = (int)((sym - 2) >> 1);
    const uint32_t offset = (2 + (sym & 1)) << extra;
    return offset + br.bits(extra) + 1;
}

using Pixels = std::unique_ptr<uint32_t[]>;
Pixels alloc_pixels(uint64_t n) {
    // (not value-initialised: every pixel is written before it is read)
    return Pixels(new uint32_t[n ? n : 1]);
}
inline uint32_t div_up(uint32_t v, int bits) { return (v + (1u << bits) - 1) >> bits; }

// an entropy-coded image of w x h ARGB pixels (RFC 9649 5, 6): the main image (`main`: meta
// prefix codes allowed) or a sub-image of a transform / the entropy image
Pixels read_image(BitReader &br, uint32_t w, uint32_t h, bool main) {
    int cache_bits = 0;
    if (br.bits(1)) {
        cache_bits = (int)br.bits(4);
        if (cache_bits < 1 || cache_bits > 11) fail("colour cache bits outside 1..11");
    }
    Pixels meta;
    int meta_bits = 0;
    uint32_t meta_w = 0, ngroups = 1;
    if (main && br.bits(1)) {
        meta_bits = (int)br.bits(3) + 2;
        meta_w = div_up(w, meta_bits);
        const uint32_t meta_h = div_up(h, meta_bits);
        meta = read_image(br, meta_w, meta_h, false);
        for (uint64_t i = 0; i < (uint64_t)meta_w * meta_h; ++i) {
            meta[i] = (meta[i] >> 8) & 0xffffu;
            if (meta[i] + 1 > ngroups) ngroups = meta[i] + 1;
        }
    }
    if (br.past_end()) fail("truncated stream");
    const int cache_size = cache_bits ? 1 << cache_bits : 0;
    const int alphabets[5] = {256 + 24 + cache_size, 256, 256, 256, 40};
    std::vector<Group> groups(ngroups);
    std::vector<uint8_t> len;
    for (uint32_t g = 0; g < ngroups; ++g)
        for (int k = 0; k < 5; ++k) read_code(br, alphabets[k], groups[g].c[k], len);
    std::vector<uint32_t> cache((size_t)cache_size);
    const int cache_shift = 32 - cache_bits;
    const uint64_t n = (uint64_t)w * h;
    Pixels px = alloc_pixels(n);
    uint64_t i = 0, cached = 0;  // pixels [cached, i) are not in the cache yet
    uint32_t x = 0, y = 0;
    const Group *G = &groups[0];
    const uint32_t meta_mask = meta ? (1u << meta_bits) - 1 : ~0u;
    auto flush_cache = [&] {
        if (cache_size)
            for (; cached < i; ++cached) cache[(px[cached] * 0x1e35a7bdu) >> cache_shift] = px[cached];
    };
    while (i < n) {
        if (br.past_end()) fail("truncated stream");
        if (meta && ((x & meta_mask) == 0)) G = &groups[meta[(uint64_t)(y >> meta_bits) * meta_w + (x >> meta_bits)]];
        const uint32_t s = G->c[0].read(br);
        if (s < 256) {
            const uint32_t r = G->c[1].read(br), b = G->c[2].read(br), a = G->c[3].read(br);
            px[i++] = (a << 24) | (r << 16) | (s << 8) | b;
            if (++x == w) x = 0, ++y;
        } else if (s < 280) {
            const uint32_t length = prefix_value(br, s - 256);
            const uint32_t dcode = prefix_value(br, G->c[4].read(br));
            uint64_t dist;
            if (dcode > 120) {
                dist = dcode - 120;
            } else {
                const int64_t d = (int64_t)kDistMap[dcode - 1][0] + (int64_t)kDistMap[dcode - 1][1] * (int64_t)w;
                dist = d < 1 ? 1 : (uint64_t)d;
            }
            if (dist > i) fail("backward reference before the start of the image");
            if (length > n - i) fail("backward reference past the end of the image");
            for (uint32_t k = 0; k < length; ++k, ++i) px[i] = px[i - dist];
            x += length;
            while (x >= w) x -= w, ++y;
            if (meta && i < n) G = &groups[meta[(uint64_t)(y >> meta_bits) * meta_w + (x >> meta_bits)]];
        } else {
            const uint32_t idx = s - 280;
            if ((int)idx >= cache_size) fail("colour cache index past the cache");
            flush_cache();
            px[i++] = cache[idx];
            if (++x == w) x = 0, ++y;
        }
        flush_cache();
    }
    if (br.past_end()) fail("truncated stream");
    return px;
}

// ---- transforms (RFC 9649 4) -------------------------------------------------------------------
inline uint32_t add_px(uint32_t a, uint32_t b) {
    return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
inline uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
inline int ch(uint32_t v, int k) { return (int)((v >> (8 * k)) & 0xffu); }
inline int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
inline uint32_t select_px(uint32_t L, uint32_t T, uint32_t TL) {
    int pl = 0, pt = 0;
    for (int k = 0; k < 4; ++k) {
        const int a = ch(T, k) - ch(TL, k), b = ch(L, k) - ch(TL, k);
        pl += a < 0 ? -a : a;
        pt += b < 0 ? -b : b;
    }
    return pl < pt ? L : T;
}
inline uint32_t clamp_full(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)clamp8(ch(a, k) + ch(b, k) - ch(c, k)) << (8 * k);
    return r;
}
inline uint32_t clamp_half(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)clamp8(ch(a, k) + (ch(a, k) - ch(b, k)) / 2) << (8 * k);
    return r;
}
inline uint32_t predict(int m, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (m) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return avg2(avg2(L, TR), T);
        case 6: return avg2(L, TL);
        case 7: return avg2(L, T);
        case 8: return avg2(TL, T);
        case 9: return avg2(T, TR);
        case 10: return avg2(avg2(L, TL), avg2(T, TR));
        case 11: return select_px(L, T, TL);
        case 12: return clamp_full(L, T, TL);
        case 13: return clamp_half(avg2(L, T), TL);
        default: return 0xff000000u;  // mode 0 (and the two unused codes)
    }
}

struct Transform {
    int type = 0;        // 0 predictor, 1 cross-colour, 2 subtract-green, 3 colour-indexing
    int bits = 0;        // block size bits (0, 1) / pixels-per-byte bits (3)
    uint32_t w = 0;      // the image width this transform's inverse produces
    Pixels data;         // sub-image (0, 1) / colour table padded to 256 entries (3)
};

// in place over px (w x h, residuals -> pixels)
void undo_predictor(const Transform &t, uint32_t *px, uint32_t w, uint32_t h) {
    const uint32_t bw = div_up(w, t.bits);
    for (uint32_t y = 0; y < h; ++y) {
        uint32_t *row = px + (uint64_t)y * w;
        if (y == 0) {
            row[0] = add_px(row[0], 0xff000000u);
            for (uint32_t x = 1; x < w; ++x) row[x] = add_px(row[x], row[x - 1]);
            continue;
        }
        const uint32_t *up = row - w;
        row[0] = add_px(row[0], up[0]);
        const uint32_t *modes = t.data.get() + (uint64_t)(y >> t.bits) * bw;
        for (uint32_t x = 1; x < w; ++x) {
            const int m = (int)((modes[x >> t.bits] >> 8) & 0xfu);
            // the rightmost pixel's top-right neighbour is the leftmost pixel of the current row
            const uint32_t TR = x + 1 < w ? up[x + 1] : row[0];
            row[x] = add_px(row[x], predict(m, row[x - 1], up[x], up[x - 1], TR));
        }
    }
}

inline int cdelta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }
void undo_cross_colour(const Transform &t, uint32_t *px, uint32_t w, uint32_t h) {
    const uint32_t bw = div_up(w, t.bits);
    for (uint32_t y = 0; y < h; ++y) {
        uint32_t *row = px + (uint64_t)y * w;
        const uint32_t *el = t.data.get() + (uint64_t)(y >> t.bits) * bw;
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t e = el[x >> t.bits], v = row[x];
            const uint32_t g2r = e & 0xffu, g2b = (e >> 8) & 0xffu, r2b = (e >> 16) & 0xffu;
            const uint32_t green = (v >> 8) & 0xffu;
            const uint32_t red = (((v >> 16) & 0xffu) + (uint32_t)cdelta(g2r, green)) & 0xffu;
            const uint32_t blue = ((v & 0xffu) + (uint32_t)cdelta(g2b, green) + (uint32_t)cdelta(r2b, red)) & 0xffu;
            row[x] = (v & 0xff00ff00u) | (red << 16) | blue;
        }
    }
}

void undo_subtract_green(uint32_t *px, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t v = px[i], g = (v >> 8) & 0xffu;
        px[i] = (v & 0xff00ff00u) | ((((v >> 16) & 0xffu) + g) & 0xffu) << 16 | (((v & 0xffu) + g) & 0xffu);
    }
}

// src: div_up(w, bits) x h packed indices -> dst: w x h colours
void undo_colour_index(const Transform &t, const uint32_t *src, uint32_t *dst, uint32_t w, uint32_t h) {
    const uint32_t sw = div_up(w, t.bits);
    const int bpp = 8 >> t.bits;
    const uint32_t pmask = (1u << t.bits) - 1, vmask = (1u << bpp) - 1;
    for (uint32_t y = 0; y < h; ++y) {
        const uint32_t *s = src + (uint64_t)y * sw;
        uint32_t *d = dst + (uint64_t)y * w;
        for (uint32_t x = 0; x < w; ++x) {
            const uint32_t g = (s[x >> t.bits] >> 8) & 0xffu;
            d[x] = t.data[(g >> ((x & pmask) * bpp)) & vmask];  // the table is zero past its colours
        }
    }
}

// the VP8L chunk payload -> ARGB pixels of *w x *h (decode == false: the size only)
Pixels decode_stream(const uint8_t *p, uint64_t n, uint32_t *w, uint32_t *h, bool decode) {
    if (n < 5) fail("VP8L chunk shorter than its header");
    if (p[0] != 0x2f) fail("bad VP8L signature");
    BitReader br(p + 1, n - 1);
    *w = br.bits(14) + 1;
    *h = br.bits(14) + 1;
    br.bits(1);  // alpha_is_used: a hint
    if (br.bits(3) != 0) fail("unknown VP8L version");
    if (!decode) return Pixels();
    std::vector<Transform> ts;
    uint32_t cw = *w;  // the width of the image still to be read
    bool seen[4] = {false, false, false, false};
    while (br.bits(1)) {
        if (br.past_end()) fail("truncated stream");
        Transform t;
        t.type = (int)br.bits(2);
        if (seen[t.type]) fail("a transform appears twice");
        seen[t.type] = true;
        t.w = cw;
        if (t.type == 0 || t.type == 1) {
            t.bits = (int)br.bits(3) + 2;
            t.data = read_image(br, div_up(cw, t.bits), div_up(*h, t.bits), false);
        } else if (t.type == 3) {
            const uint32_t ncol = br.bits(8) + 1;
            Pixels tab = read_image(br, ncol, 1, false);
            t.data = alloc_pixels(256);
            for (uint32_t k = 0; k < 256; ++k) t.data[k] = 0;
            t.data[0] = tab[0];
            for (uint32_t k = 1; k < ncol; ++k) t.data[k] = add_px(tab[k], t.data[k - 1]);
            t.bits = ncol <= 2 ? 3 : ncol <= 4 ? 2 : ncol <= 16 ? 1 : 0;
            cw = div_up(cw, t.bits);
        }
        ts.push_back(std::move(t));
    }
    if (br.past_end()) fail("truncated stream");
    Pixels px = read_image(br, cw, *h, true);
    for (size_t k = ts.size(); k-- > 0;) {
        const Transform &t = ts[k];
        if (t.type == 0) {
            undo_predictor(t, px.get(), t.w, *h);
        } else if (t.type == 1) {
            undo_cross_colour(t, px.get(), t.w, *h);
        } else if (t.type == 2) {
            undo_subtract_green(px.get(), (uint64_t)t.w * *h);
        } else {
            Pixels out = alloc_pixels((uint64_t)t.w * *h);
            undo_colour_index(t, px.get(), out.get(), t.w, *h);
            px = std::move(out);
        }
    }
    return px;
}

// the VP8L chunk of a RIFF/WEBP file (RFC 9649 2.5-2.7)
void find_chunk(const uint8_t *d, uint64_t len, const uint8_t **chunk, uint64_t *size) {
    if (len < 12 || std::memcmp(d, "RIFF", 4) != 0 || std::memcmp(d + 8, "WEBP", 4) != 0) fail("not a RIFF WEBP file");
    uint64_t end = 8 + (uint64_t)le32(d + 4);
    if (end > len) end = len;  // a truncated file: its chunks are checked against what is there
    uint64_t o = 12;
    while (o + 8 <= end) {
        const uint64_t sz = le32(d + o + 4);
        if (std::memcmp(d + o, "VP8L", 4) == 0) {
            if (sz > end - (o + 8)) fail("VP8L chunk runs past the file");
            *chunk = d + o + 8;
            *size = sz;
            return;
        }
        if (std::memcmp(d + o, "VP8 ", 4) == 0) throw Fail{ST_ERR_UNSUPPORTED, "webp: lossy VP8 image (lossless only)"};
        o += 8 + sz + (sz & 1);
    }
    fail("no VP8L chunk");
}

template <typename F>
int guarded(F &&f) {
    try {
        f();
        return ST_OK;
    } catch (const Fail &e) {
        set_last_error(e.msg);
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("webp: host allocation failed");
        return ST_ERR_NOMEM;
    }
}

}  // namespace
}  // namespace vp8l_dec
}  // namespace st

using namespace st::vp8l_dec;

extern "C" {

int st_webp_info(const uint8_t *data, uint64_t len, int32_t *width, int32_t *height) {
    return guarded([&] {
        if (!data || !width || !height) fail("NULL argument");
        const uint8_t *chunk = nullptr;
        uint64_t size = 0;
        find_chunk(data, len, &chunk, &size);
        uint32_t w = 0, h = 0;
        decode_stream(chunk, size, &w, &h, false);
        *width = (int32_t)w;
        *height = (int32_t)h;
    });
}

int st_webp_decode_lossless(const uint8_t *data, uint64_t len, uint8_t *rgba_out, int32_t stride) {
    return guarded([&] {
        if (!data || !rgba_out) fail("NULL argument");
        const uint8_t *chunk = nullptr;
        uint64_t size = 0;
        find_chunk(data, len, &chunk, &size);
        uint32_t w = 0, h = 0;
        decode_stream(chunk, size, &w, &h, false);
        if (stride < 0 || (uint64_t)stride < (uint64_t)w * 4) fail("stride below the row size");
        Pixels px = decode_stream(chunk, size, &w, &h, true);
        for (uint32_t y = 0; y < h; ++y) {
            uint8_t *o = rgba_out + (uint64_t)y * (uint64_t)stride;
            const uint32_t *s = px.get() + (uint64_t)y * w;
            for (uint32_t x = 0; x < w; ++x) {
                const uint32_t v = s[x];
                o[4 * x + 0] = (uint8_t)(v >> 16);
                o[4 * x + 1] = (uint8_t)(v >> 8);
                o[4 * x + 2] = (uint8_t)v;
                o[4 * x + 3] = (uint8_t)(v >> 24);
            }
        }
    });
}

}  // extern "C"
