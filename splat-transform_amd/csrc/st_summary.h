// st_summary.h -- the column summary of include/st_abi.h ("column summary"): every rule as a
// host/device function, and a plain serial host form of the whole summary (summarize_host).  The
// kernels of st_summary.hip, the library's host epilogue and tests/native/summary_cpu_check.cpp
// all go through these functions, so they cannot disagree on a key, a limb or a rounding.
//
// THE SUPERACCUMULATOR.  A sum of doubles is kept exactly as NL = 70 signed 64-bit limbs at 32-bit
// spacing: limb j counts units of 2^(32 j - 1088), so bit 14 of limb 0 is 2^-1074, the smallest
// subnormal, and the limbs reach 2^1152: 2^53 values below 2^1024 stay below 2^1077.  A finite
// double is a 53-bit integer times a power of two; shifted to its place it spans three limbs and
// adds less than 2^32 in magnitude to each (acc_chunks).  HEADROOM: a limb that starts normalised
// (below 2^32) takes 2^31 - 1 such additions before it can leave int64; FLUSH_DEFAULT = 2^30
// additions between two normalisations (on the device: of one wave, into all of its copies
// together, which therefore also fold into one without leaving int64) keeps a factor of two below
// that, with the at most 1,024 additions one loop step of a wave overshoots by.  Normalising (acc_normalise)
// carries every limb but the top one into [0, 2^32); the top limb keeps the sign.  Limb-wise
// integer addition is associative, so partial accumulators merge in any order -- with atomics too
// -- and the merged limbs are the same bits every time.  acc_round rounds once, to nearest-even,
// with a sticky bit over everything below the round bit; a magnitude of 2^1024 - 2^970 or more
// gives an infinity.  An excursion beyond the double range on the way never exists: no double
// partial sum is ever formed.
//
// THE FAST PATH.  When the classify pass found every finite non-zero element's lowest set bit at
// 2^e_lo or above and its highest at 2^e_hi or below, an element is an integer of at most
// e_hi - e_lo + 1 bits in units of 2^e_lo; with bitlen(m) more bits for m of them the whole sum
// fits a signed __int128 when that total is at most 126 (fast_ok), and so does every partial.
// The int128 total goes into an empty limb array (acc_add_i128) and through the same acc_round.
#ifndef ST_SUMMARY_H
#define ST_SUMMARY_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/st_abi.h"
#include "st_numfmt.h"

#if defined(__HIPCC__)
#define ST_SM_HD __host__ __device__ inline
#else
#define ST_SM_HD inline
#endif

namespace st {
namespace sm {

constexpr int NL = 70;       // limbs
constexpr int BASE = 1088;   // limb j: units of 2^(32 j - BASE)
constexpr uint64_t FLUSH_DEFAULT = 1ull << 30;  // additions per accumulator between normalisations
constexpr uint64_t FLUSH_MAX = 1ull << 30;
constexpr int E_NONE_LO = 1 << 20, E_NONE_HI = -(1 << 20);  // e_lo / e_hi of a column without a finite non-zero element

ST_SM_HD int elem_size(int32_t type) {
    switch (type) {
        case ST_PLY_CHAR:
        case ST_PLY_UCHAR: return 1;
        case ST_PLY_SHORT:
        case ST_PLY_USHORT: return 2;
        case ST_PLY_INT:
        case ST_PLY_UINT:
        case ST_PLY_FLOAT: return 4;
        case ST_PLY_DOUBLE: return 8;
        default: return 0;
    }
}
ST_SM_HD int key_bits(int32_t type) { return 8 * elem_size(type); }

// 0: finite, 1: NaN (any sign or payload), 2: +-Infinity.  bits: the element zero-extended
ST_SM_HD int classify(int32_t type, uint64_t bits) {
    if (type == ST_PLY_FLOAT) {
        const uint32_t a = (uint32_t)bits & 0x7fffffffu;
        return a > 0x7f800000u ? 1 : (a == 0x7f800000u ? 2 : 0);
    }
    if (type == ST_PLY_DOUBLE) {
        const uint64_t a = bits & 0x7fffffffffffffffull;
        return a > 0x7ff0000000000000ull ? 1 : (a == 0x7ff0000000000000ull ? 2 : 0);
    }
    return 0;
}

// the order-preserving key of a finite element in key_bits(type) bits: signed integers with the
// sign bit flipped, floats with the sign bit set (positive) or all bits flipped (negative) -- -0
// lands just below +0.  NaN and the infinities never reach here (a negative NaN would sort lowest)
ST_SM_HD uint64_t key_of(int32_t type, uint64_t bits) {
    switch (type) {
        case ST_PLY_CHAR: return bits ^ 0x80u;
        case ST_PLY_SHORT: return bits ^ 0x8000u;
        case ST_PLY_INT: return bits ^ 0x80000000u;
        case ST_PLY_FLOAT: return (bits & 0x80000000u) ? (~bits & 0xffffffffu) : (bits | 0x80000000u);
        case ST_PLY_DOUBLE: return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
        default: return bits;
    }
}
ST_SM_HD uint64_t key_inv(int32_t type, uint64_t key) {
    switch (type) {
        case ST_PLY_CHAR: return key ^ 0x80u;
        case ST_PLY_SHORT: return key ^ 0x8000u;
        case ST_PLY_INT: return key ^ 0x80000000u;
        case ST_PLY_FLOAT: return (key & 0x80000000u) ? (key & 0x7fffffffu) : (~key & 0xffffffffu);
        case ST_PLY_DOUBLE: return (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
        default: return key;
    }
}

ST_SM_HD double f64_of_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
ST_SM_HD uint64_t bits_of_f64(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

// the element as a JS number: every one of the eight types widens to a double exactly
ST_SM_HD double widen(int32_t type, uint64_t bits) {
    switch (type) {
        case ST_PLY_CHAR: return (double)(int8_t)(uint8_t)bits;
        case ST_PLY_UCHAR: return (double)(uint8_t)bits;
        case ST_PLY_SHORT: return (double)(int16_t)(uint16_t)bits;
        case ST_PLY_USHORT: return (double)(uint16_t)bits;
        case ST_PLY_INT: return (double)(int32_t)(uint32_t)bits;
        case ST_PLY_UINT: return (double)(uint32_t)bits;
        case ST_PLY_FLOAT: {
            const uint32_t b = (uint32_t)bits;
            float f;
            memcpy(&f, &b, 4);
            return (double)f;
        }
        default: return f64_of_bits(bits);
    }
}

// a finite non-zero double as (-1)^neg * m * 2^e with m odd or not, m < 2^53 (the stored significand)
struct Parts {
    uint64_t m;
    int e;
    bool neg;
};
ST_SM_HD Parts parts_of(double v) {
    const uint64_t b = bits_of_f64(v);
    const uint32_t ex = (uint32_t)(b >> 52) & 0x7ffu;
    const uint64_t man = b & 0xfffffffffffffull;
    Parts p;
    p.m = ex ? (man | (1ull << 52)) : man;
    p.e = ex ? (int)ex - 1075 : -1074;
    p.neg = (b >> 63) != 0;
    return p;
}
ST_SM_HD int ctz64(uint64_t x) { return __builtin_ctzll(x); }
ST_SM_HD int bitlen64(uint64_t x) { return x ? 64 - __builtin_clzll(x) : 0; }
// exponents of the lowest and the highest set bit of a finite non-zero double
ST_SM_HD void bit_span(double v, int *lo, int *hi) {
    const Parts p = parts_of(v);
    *lo = p.e + ctz64(p.m);
    *hi = p.e + bitlen64(p.m) - 1;
}

// the whole sum of m elements between 2^e_lo and 2^e_hi, and every partial of it, fits an int128
ST_SM_HD bool fast_ok(int e_lo, int e_hi, uint64_t m) {
    if (e_lo > e_hi) return true;  // nothing but zeros
    return (int64_t)e_hi - e_lo + 1 + bitlen64(m) <= 126;
}
// v (finite, every set bit at 2^e_lo or above) in units of 2^e_lo
ST_SM_HD __int128 units_of(double v, int e_lo) {
    if (v == 0) return 0;
    const Parts p = parts_of(v);
    const int tz = ctz64(p.m);
    const __int128 u = (__int128)(p.m >> tz) << (p.e + tz - e_lo);
    return p.neg ? -u : u;
}

// a finite non-zero double as three signed addends for limbs j, j + 1, j + 2 (each below 2^32 in
// magnitude); j + 2 <= 66
ST_SM_HD void acc_chunks(double v, int *j, int64_t c[3]) {
    const Parts p = parts_of(v);
    const int pos = p.e + BASE;  // >= 14
    *j = pos >> 5;
    const unsigned __int128 w = (unsigned __int128)p.m << (pos & 31);
    c[0] = (int64_t)(uint32_t)w;
    c[1] = (int64_t)(uint32_t)(w >> 32);
    c[2] = (int64_t)(uint64_t)(w >> 64);
    if (p.neg) c[0] = -c[0], c[1] = -c[1], c[2] = -c[2];
}
ST_SM_HD void acc_add(int64_t *limbs, double v) {
    if (v == 0) return;
    int j;
    int64_t c[3];
    acc_chunks(v, &j, c);
    limbs[j] += c[0];
    limbs[j + 1] += c[1];
    limbs[j + 2] += c[2];
}
// V * 2^e_lo into limbs that hold nothing yet (the fast path's total); e_lo >= -1074
ST_SM_HD void acc_add_i128(int64_t *limbs, __int128 V, int e_lo) {
    if (V == 0) return;
    const bool neg = V < 0;
    const unsigned __int128 mag = neg ? (unsigned __int128)0 - (unsigned __int128)V : (unsigned __int128)V;
    const int pos = e_lo + BASE, j = pos >> 5, s = pos & 31;
    for (int k = 0; k < 4; ++k) {
        const int64_t d = (int64_t)((uint64_t)(uint32_t)(mag >> (32 * k)) << s);  // below 2^63
        limbs[j + k] += neg ? -d : d;
    }
}
// carries: limbs 0 .. NL-2 into [0, 2^32), the top limb keeps the rest and the sign
ST_SM_HD void acc_normalise(int64_t *limbs) {
    int64_t carry = 0;
    for (int j = 0; j < NL - 1; ++j) {
        const int64_t x = limbs[j] + carry;
        carry = x >> 32;  // arithmetic: floor
        limbs[j] = x & 0xffffffffll;
    }
    limbs[NL - 1] += carry;
}
// the limbs' value rounded once to double, nearest-even; +0 for an exact zero
ST_SM_HD double acc_round(const int64_t *in) {
    int64_t d[NL];
    for (int j = 0; j < NL; ++j) d[j] = in[j];
    acc_normalise(d);
    const bool neg = d[NL - 1] < 0;
    if (neg) {  // two's complement over the digits
        uint64_t carry = 1;
        for (int j = 0; j < NL - 1; ++j) {
            const uint64_t v = (~(uint64_t)d[j] & 0xffffffffull) + carry;
            d[j] = (int64_t)(v & 0xffffffffull);
            carry = v >> 32;
        }
        d[NL - 1] = (int64_t)(~(uint64_t)d[NL - 1] + carry);
    }
    uint32_t dig[NL + 4];
    for (int j = 0; j < NL - 1; ++j) dig[j] = (uint32_t)d[j];
    dig[NL - 1] = (uint32_t)(uint64_t)d[NL - 1];
    dig[NL] = (uint32_t)((uint64_t)d[NL - 1] >> 32);
    dig[NL + 1] = dig[NL + 2] = dig[NL + 3] = 0;
    int h = NL;
    while (h >= 0 && dig[h] == 0) --h;
    if (h < 0) return 0.0;
    const int bl = 32 * h + 32 - __builtin_clz(dig[h]);  // the magnitude is below 2^(bl - BASE)
    const int p = bl - 53 > 14 ? bl - 53 : 14;           // the result's ulp is bit p (2^-1074 is bit 14)
    const int j = p >> 5, s = p & 31;
    const unsigned __int128 w = (unsigned __int128)dig[j] | ((unsigned __int128)dig[j + 1] << 32) |
                                ((unsigned __int128)dig[j + 2] << 64) | ((unsigned __int128)dig[j + 3] << 96);
    uint64_t M = (uint64_t)(w >> s) & ((1ull << 53) - 1);  // bits [p, p + 53): nothing is set above bl
    if (p > 14) {
        const int r = p - 1, rj = r >> 5, rs = r & 31;
        const bool round = (dig[rj] >> rs) & 1u;
        bool sticky = (dig[rj] & ((1u << rs) - 1u)) != 0;
        for (int k = 0; k < rj && !sticky; ++k) sticky = dig[k] != 0;
        if (round && (sticky || (M & 1))) ++M;
    }
    // biased exponent p - 13 for a normal M (bit 52 set adds the 1), 0 for a subnormal; M = 2^53 carries
    uint64_t bits = ((uint64_t)(p - 14) << 52) + M;
    if ((bits >> 52) >= 2047) bits = 0x7ff0000000000000ull;
    return f64_of_bits(bits | (neg ? 0x8000000000000000ull : 0));
}

// ---- the scalar epilogue: every operation rounds once, in this order -------------------------------
// what the passes leave for one column
struct Gathered {
    uint64_t rows, nan_count, inf_count;
    uint64_t kmin, kmax;   // keys of the finite elements' extremes (m > 0)
    uint64_t kmed[2];      // keys of ranks (m - 1) / 2 and m / 2
};
inline void finish_counts(int32_t type, const Gathered &g, st_col_summary *o) {
    o->rows = g.rows;
    o->nan_count = g.nan_count;
    o->inf_count = g.inf_count;
    const uint64_t m = g.rows - g.nan_count - g.inf_count;
    const double nan = f64_of_bits(0x7ff8000000000000ull);
    if (m == 0) {
        o->min = o->max = o->mean = o->std_dev = o->median = nan;
        o->sum = o->ssd = 0.0;
        return;
    }
    o->min = widen(type, key_inv(type, g.kmin));
    o->max = widen(type, key_inv(type, g.kmax));
    const double a = widen(type, key_inv(type, g.kmed[0])), b = widen(type, key_inv(type, g.kmed[1]));
    o->median = (m & 1) ? a : (a + b) / 2;
}
inline double mean_of(double sum, uint64_t m) { return sum / (double)m; }
inline void finish_ssd(double ssd, uint64_t m, st_col_summary *o) {
    o->ssd = ssd;
    o->std_dev = std::sqrt(ssd / (double)m);
}

// ---- the serial host form --------------------------------------------------------------------
inline uint64_t load_elem(const void *col, int z, uint64_t i) {
    uint64_t b = 0;
    memcpy(&b, (const char *)col + i * (uint64_t)z, (size_t)z);  // little-endian host
    return b;
}
// one column, serially: classify, the sum (fast path unless exact or the span declines), the
// deviation, the median by a sort of the keys.  flush: additions between normalisations.
// *fast (nullable): the sum took the int128 path
inline void summarize_host(int32_t type, const void *col, uint64_t n, bool exact, uint64_t flush, st_col_summary *o,
                           bool *fast) {
    const int z = elem_size(type);
    Gathered g{n, 0, 0, ~0ull, 0, {0, 0}};
    int e_lo = E_NONE_LO, e_hi = E_NONE_HI;
    std::vector<uint64_t> keys;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t b = load_elem(col, z, i);
        const int c = classify(type, b);
        if (c) {
            (c == 1 ? g.nan_count : g.inf_count) += 1;
            continue;
        }
        const uint64_t k = key_of(type, b);
        keys.push_back(k);
        g.kmin = std::min(g.kmin, k);
        g.kmax = std::max(g.kmax, k);
        const double v = widen(type, b);
        if (v != 0) {
            int lo, hi;
            bit_span(v, &lo, &hi);
            e_lo = std::min(e_lo, lo);
            e_hi = std::max(e_hi, hi);
        }
    }
    const uint64_t m = keys.size();
    if (m) {
        std::sort(keys.begin(), keys.end());
        g.kmed[0] = keys[(m - 1) / 2];
        g.kmed[1] = keys[m / 2];
    }
    finish_counts(type, g, o);
    const bool use_fast = !exact && fast_ok(e_lo, e_hi, m);
    if (fast) *fast = use_fast;
    if (m == 0) return;
    int64_t limbs[NL] = {0};
    if (use_fast) {
        __int128 V = 0;
        for (uint64_t k : keys) V += units_of(widen(type, key_inv(type, k)), e_lo);
        acc_add_i128(limbs, V, e_lo);
    } else {
        uint64_t adds = 0;
        for (uint64_t k : keys) {
            acc_add(limbs, widen(type, key_inv(type, k)));
            if (++adds >= flush) acc_normalise(limbs), adds = 0;
        }
    }
    o->sum = acc_round(limbs);
    o->mean = mean_of(o->sum, m);
    for (int j = 0; j < NL; ++j) limbs[j] = 0;
    bool tinf = false;
    uint64_t adds = 0;
    for (uint64_t k : keys) {
        const double d = widen(type, key_inv(type, k)) - o->mean;
        const double t = d * d;
        if (std::isinf(t)) {
            tinf = true;
            continue;
        }
        acc_add(limbs, t);
        if (++adds >= flush) acc_normalise(limbs), adds = 0;
    }
    finish_ssd(tinf ? f64_of_bits(0x7ff0000000000000ull) : acc_round(limbs), m, o);
}

// ---- st_summary_text ---------------------------------------------------------------------------------
inline void put_f64(std::string &s, double v, const uint64_t *tab) {
    char buf[numfmt::MAX_CELL + 8];
    const uint64_t bits = bits_of_f64(v);
    const uint32_t n = numfmt::len(ST_PLY_DOUBLE, bits, tab);
    numfmt::put(ST_PLY_DOUBLE, bits, tab, buf);
    s.append(buf, n);
}
// tab: st_numfmt.h's power-of-ten table
inline std::string summary_text(const st_ttable *t, const st_col_summary *s, const uint64_t *tab) {
    std::string out = "column,rows,nanCount,infCount,min,max,mean,stdDev,median\n";
    for (int p = 0; p < t->ncol; ++p) {
        out += t->names[p];
        const uint64_t counts[3] = {s[p].rows, s[p].nan_count, s[p].inf_count};
        for (uint64_t c : counts) out += ',' + std::to_string((unsigned long long)c);
        const double vals[5] = {s[p].min, s[p].max, s[p].mean, s[p].std_dev, s[p].median};
        for (double v : vals) {
            out += ',';
            put_f64(out, v, tab);
        }
        out += '\n';
    }
    return out;
}

}  // namespace sm
}  // namespace st

#endif /* ST_SUMMARY_H */
