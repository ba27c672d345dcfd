// st_numfmt.h -- the text of a typed-array element as JavaScript prints it ('' + column[i],
// writers/write-csv.ts:16-20): ECMA-262 Number::toString, radix 10.  One set of functions for the
// host and the device, integer arithmetic only.
//
// A value becomes a Dec first -- its sign, its decimal digits as an integer and the position n of
// the decimal point (value = 0.d1d2...dk x 10^n) -- and dec_len / dec_put turn a Dec into the
// byte count and the bytes.  len and put of every type go through the same Dec, so they cannot
// disagree.
//
// Digits of a double: Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020),
// written from the paper.  With v = c * 2^q, the rounding interval's ends and v itself are
// multiplied by 10^-k (k = floor(log10 2^q), so that the products have 16-17 digits), as
// 128 x 64 bit products with a 128-bit approximation of the power of ten, rounded to odd; two
// bits below the integer part decide which decimal of the shortest length lies in the interval and
// which of two is closer.  The table holds, for e = -292 .. 324,
//     g(e) = ceil(10^e * 2^(127 - floor(log2 10^e)))          (2^127 <= g(e) < 2^128)
// as (high, low) 64-bit halves: 617 entries, 9872 bytes.  numfmt_build_table computes it with
// exact big-integer arithmetic; nothing is typed in.  A float32 is widened to the double of the
// same value (exactly, by shifting its significand) and printed as that double, as JS does.
#ifndef ST_NUMFMT_H
#define ST_NUMFMT_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ST_HD __host__ __device__ inline
#else
#define ST_HD inline
#endif

namespace st {
namespace numfmt {

constexpr int POW10_MIN = -292, POW10_MAX = 324;
constexpr int POW10_ENTRIES = POW10_MAX - POW10_MIN + 1;  // 617 entries of two uint64_t (high, low)
// a float32 widened: q in [-201, 75], k in [-61, 22]: entries -22 .. 61 only
constexpr int MAX_CELL = 25;  // -0.0000012345678901234567

enum DecKind : uint32_t { DEC_NUM = 0, DEC_ZERO, DEC_NAN, DEC_INF };

// value = (-1)^neg * 0.d1..dk * 10^n, d = the k digits as an integer (d1 != 0; integers keep their
// trailing zeros and have n == k)
struct Dec {
    uint64_t d;
    int32_t k, n;
    uint32_t kind, neg;
};

// ---- the table, on the host ------------------------------------------------------------------
// tab[2 * (e - POW10_MIN)] = high half, [.. + 1] = low half of g(e)
inline void numfmt_build_table(uint64_t *tab) {
    constexpr int L = 36;  // 32-bit limbs: 10^324 < 2^1077
    struct Big {
        uint32_t w[L];
    };
    auto bitlen = [](const Big &a) {
        for (int i = L - 1; i >= 0; --i)
            if (a.w[i]) {
                int b = 0;
                for (uint32_t v = a.w[i]; v; v >>= 1) ++b;
                return i * 32 + b;
            }
        return 0;
    };
    auto bit = [](const Big &a, int i) { return i < 0 ? 0u : (a.w[i >> 5] >> (i & 31)) & 1u; };
    Big p{};
    p.w[0] = 1;  // 10^m
    for (int m = 0; m <= POW10_MAX; ++m) {
        const int b = bitlen(p);
        // e = +m: the top 128 bits of 10^m, rounded up when bits are dropped
        {
            uint64_t hi = 0, lo = 0;
            for (int i = 0; i < 128; ++i) {
                hi = (hi << 1) | (lo >> 63);
                lo = (lo << 1) | bit(p, b - 1 - i);
            }
            bool sticky = false;
            for (int i = 0; i < b - 128; ++i) sticky = sticky || bit(p, i);
            if (sticky && ++lo == 0) ++hi;
            tab[2 * (m - POW10_MIN)] = hi;
            tab[2 * (m - POW10_MIN) + 1] = lo;
        }
        // e = -m: ceil(2^(127 + b) / 10^m) by 128 steps of shift-and-subtract from 2^(b - 1)
        if (m >= 1 && -m >= POW10_MIN) {
            Big r{};
            r.w[(b - 1) >> 5] = 1u << ((b - 1) & 31);
            uint64_t hi = 0, lo = 0;
            for (int s = 0; s < 128; ++s) {
                uint32_t carry = 0;
                for (int i = 0; i < L; ++i) {
                    const uint32_t v = r.w[i];
                    r.w[i] = (v << 1) | carry;
                    carry = v >> 31;
                }
                bool ge = true;
                for (int i = L - 1; i >= 0; --i)
                    if (r.w[i] != p.w[i]) {
                        ge = r.w[i] > p.w[i];
                        break;
                    }
                if (ge) {
                    uint64_t borrow = 0;
                    for (int i = 0; i < L; ++i) {
                        const uint64_t t = (uint64_t)r.w[i] - p.w[i] - borrow;
                        r.w[i] = (uint32_t)t;
                        borrow = (t >> 32) & 1;
                    }
                }
                hi = (hi << 1) | (lo >> 63);
                lo = (lo << 1) | (ge ? 1u : 0u);
            }
            if (bitlen(r) && ++lo == 0) ++hi;  // 10^m has a factor 5: never exact
            tab[2 * (-m - POW10_MIN)] = hi;
            tab[2 * (-m - POW10_MIN) + 1] = lo;
        }
        uint64_t carry = 0;  // p *= 10
        for (int i = 0; i < L; ++i) {
            const uint64_t t = (uint64_t)p.w[i] * 10 + carry;
            p.w[i] = (uint32_t)t;
            carry = t >> 32;
        }
    }
}

// ---- 64 x 64 -> 128 ----------------------------------------------------------------------------
ST_HD uint64_t mul_hi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor((g * cp) / 2^128), its lowest bit set when any lower bit of the product is ("round to odd")
ST_HD uint64_t round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    const uint64_t xhi = mul_hi64(glo, cp);
    const uint64_t ylo = ghi * cp, yhi = mul_hi64(ghi, cp);
    const uint64_t mid = ylo + xhi;
    return (yhi + (mid < ylo ? 1 : 0)) | (mid > 1 ? 1 : 0);
}

ST_HD int32_t count_digits(uint64_t d) {
    if (d >= 10000000000000000ull) return 17;
    if (d >= 1000000000000000ull) return 16;
    int32_t k = 1;
    for (uint64_t p = 10; d >= p; p *= 10) ++k;
    return k;
}

// the shortest decimal of the finite non-zero double c * 2^q (c < 2^53; c >= 2^52 unless the
// double is subnormal, q = -1074), the closest of that length; `irregular`: c == 2^52 and the
// double below is half as far away as the one above
ST_HD Dec dec_from_cq(uint32_t neg, uint64_t c, int32_t q, bool irregular, const uint64_t *tab) {
    const uint64_t cb = c << 2, cbl = cb - (irregular ? 1 : 2), cbr = cb + 2;
    // floor(log10(2^q)), or floor(log10(3/4 * 2^q)); exact for |q| <= 1500
    const int32_t k = (q * 1262611 - (irregular ? 524031 : 0)) >> 22;
    // q + floor(log2(10^-k)) + 1, in 1..4
    const int32_t h = q + ((-k * 1741647) >> 19) + 1;
    const uint64_t ghi = tab[2 * (-k - POW10_MIN)], glo = tab[2 * (-k - POW10_MIN) + 1];
    const uint64_t vbl = round_to_odd(ghi, glo, cbl << h);
    const uint64_t vb = round_to_odd(ghi, glo, cb << h);
    const uint64_t vbr = round_to_odd(ghi, glo, cbr << h);
    const uint64_t odd = c & 1;  // an even significand owns the interval's ends
    const uint64_t lower = vbl + odd, upper = vbr - odd;
    const uint64_t s = vb >> 2;
    uint64_t d;
    int32_t e = k;
    bool done = false;
    if (s >= 10) {  // one digit less
        const uint64_t sp = s / 10;
        const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
        if (up_in != wp_in) {
            d = sp + (wp_in ? 1 : 0);
            e = k + 1;
            done = true;
        }
    }
    if (!done) {
        const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
        if (u_in != w_in) {
            d = s + (w_in ? 1 : 0);
        } else {  // both or neither: the closer one, the even one on a tie
            const uint64_t mid = 4 * s + 2;
            d = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
        }
    }
    for (;;) {  // no trailing zeros
        const uint64_t t = d / 10;
        if (t * 10 != d) break;
        d = t;
        ++e;
    }
    Dec r;
    r.d = d;
    r.k = count_digits(d);
    r.n = r.k + e;
    r.kind = DEC_NUM;
    r.neg = neg;
    return r;
}

ST_HD Dec dec_special(uint32_t kind, uint32_t neg) {
    Dec r;
    r.d = 0, r.k = 1, r.n = 1, r.kind = kind, r.neg = neg;
    return r;
}

ST_HD Dec dec_f64_bits(uint64_t bits, const uint64_t *tab) {
    const uint32_t neg = (uint32_t)(bits >> 63), ex = (uint32_t)(bits >> 52) & 0x7ff;
    const uint64_t m = bits & 0xfffffffffffffull;
    if (ex == 0x7ff) return m ? dec_special(DEC_NAN, 0) : dec_special(DEC_INF, neg);
    if (ex == 0) return m ? dec_from_cq(neg, m, -1074, false, tab) : dec_special(DEC_ZERO, 0);
    return dec_from_cq(neg, m | (1ull << 52), (int32_t)ex - 1075, m == 0 && ex > 1, tab);
}

// the float32's value as a double: its significand moved up to 53 bits (a float32 subnormal is a
// normal double)
ST_HD Dec dec_f32_bits(uint32_t bits, const uint64_t *tab) {
    const uint32_t neg = bits >> 31, ex = (bits >> 23) & 0xff;
    uint32_t m = bits & 0x7fffff;
    if (ex == 0xff) return m ? dec_special(DEC_NAN, 0) : dec_special(DEC_INF, neg);
    int32_t q;
    if (ex == 0) {
        if (!m) return dec_special(DEC_ZERO, 0);
        int32_t sh = 0;
        while (!(m & 0x800000)) m <<= 1, ++sh;
        q = -149 - sh;
    } else {
        m |= 0x800000;
        q = (int32_t)ex - 150;
    }
    return dec_from_cq(neg, (uint64_t)m << 29, q - 29, m == 0x800000, tab);
}

// an integer element: its decimal digits as they are
ST_HD Dec dec_int(uint32_t neg, uint32_t mag) {
    if (!mag) return dec_special(DEC_ZERO, 0);
    Dec r;
    r.d = mag;
    r.k = r.n = count_digits(mag);
    r.kind = DEC_NUM;
    r.neg = neg;
    return r;
}

// one element of a column of st_ply_type `type` (1 = int8 .. 6 = uint32, 7 = float32, 8 = float64)
// given as its bits, zero-extended
ST_HD Dec dec_of(int32_t type, uint64_t bits, const uint64_t *tab) {
    switch (type) {
        case 1: { const int32_t v = (int8_t)bits; return dec_int(v < 0, v < 0 ? (uint32_t)-v : (uint32_t)v); }
        case 2: return dec_int(0, (uint8_t)bits);
        case 3: { const int32_t v = (int16_t)bits; return dec_int(v < 0, v < 0 ? (uint32_t)-v : (uint32_t)v); }
        case 4: return dec_int(0, (uint16_t)bits);
        case 5: { const int32_t v = (int32_t)bits; return dec_int(v < 0, v < 0 ? 0u - (uint32_t)v : (uint32_t)v); }
        case 6: return dec_int(0, (uint32_t)bits);
        case 7: return dec_f32_bits((uint32_t)bits, tab);
        default: return dec_f64_bits(bits, tab);
    }
}

// the longest text of a column type (write-csv.ts's cells): 4 3 6 5 11 10 25 25
ST_HD uint32_t max_cell(int32_t type) {
    switch (type) {
        case 1: return 4;
        case 2: return 3;
        case 3: return 6;
        case 4: return 5;
        case 5: return 11;
        case 6: return 10;
        case 7: return 25;
        case 8: return 25;
        default: return 0;
    }
}

// Number::toString's layout of 0.d1..dk x 10^n (ECMA-262 6.1.6.1.20, steps 6-10)
ST_HD uint32_t dec_len(const Dec &v) {
    if (v.kind == DEC_ZERO) return 1;
    if (v.kind == DEC_NAN) return 3;
    if (v.kind == DEC_INF) return 8 + v.neg;
    const int32_t k = v.k, n = v.n;
    if (n >= k && n <= 21) return v.neg + n;
    if (n > 0 && n <= 21) return v.neg + k + 1;
    if (n > -6 && n <= 0) return v.neg + 2 - n + k;
    const int32_t ex = n - 1 < 0 ? 1 - n : n - 1;
    return v.neg + k + (k > 1 ? 1 : 0) + 2 + (ex >= 100 ? 3 : ex >= 10 ? 2 : 1);
}

// exactly dec_len(v) bytes at dst
ST_HD void dec_put(const Dec &v, char *dst) {
    if (v.kind == DEC_ZERO) {
        dst[0] = '0';
        return;
    }
    if (v.kind == DEC_NAN) {
        dst[0] = 'N', dst[1] = 'a', dst[2] = 'N';
        return;
    }
    if (v.neg) *dst++ = '-';
    if (v.kind == DEC_INF) {
        const char *s = "Infinity";
        for (int i = 0; i < 8; ++i) dst[i] = s[i];
        return;
    }
    const int32_t k = v.k, n = v.n;
    int32_t split = 64;  // a '.' goes before digit `split`
    int32_t ex = 0;
    bool expo = false;
    if (n >= k && n <= 21) {
        for (int32_t i = k; i < n; ++i) dst[i] = '0';
    } else if (n > 0 && n <= 21) {
        split = n;
        dst[n] = '.';
    } else if (n > -6 && n <= 0) {
        dst[0] = '0', dst[1] = '.';
        for (int32_t i = 0; i < -n; ++i) dst[2 + i] = '0';
        dst += 2 - n;
    } else {
        expo = true;
        ex = n - 1;
        if (k > 1) split = 1, dst[1] = '.';
    }
    // the digits from the last: the low eight from a 32-bit part, the rest from the other
    uint32_t hi = (uint32_t)(v.d / 100000000u), lo = (uint32_t)(v.d - (uint64_t)hi * 100000000u);
    for (int32_t j = 0; j < k; ++j) {
        const int32_t i = k - 1 - j;
        uint32_t digit;
        if (j < 8) digit = lo % 10, lo /= 10;
        else digit = hi % 10, hi /= 10;
        dst[i + (i >= split ? 1 : 0)] = (char)('0' + digit);
    }
    if (expo) {
        char *p = dst + k + (k > 1 ? 1 : 0);
        *p++ = 'e';
        *p++ = ex < 0 ? '-' : '+';
        uint32_t a = (uint32_t)(ex < 0 ? -ex : ex);
        if (a >= 100) *p++ = (char)('0' + a / 100), a %= 100, *p++ = (char)('0' + a / 10), a %= 10;
        else if (a >= 10) *p++ = (char)('0' + a / 10), a %= 10;
        *p++ = (char)('0' + a);
    }
}

ST_HD uint32_t len(int32_t type, uint64_t bits, const uint64_t *tab) { return dec_len(dec_of(type, bits, tab)); }
ST_HD void put(int32_t type, uint64_t bits, const uint64_t *tab, char *dst) { dec_put(dec_of(type, bits, tab), dst); }

}  // namespace numfmt
}  // namespace st

#endif
