// st_ksplat_encode.h -- the .ksplat writer's per-value and per-record encode functions
// (include/st_abi.h, "the .ksplat writer").  __host__ __device__, as the other writers' are:
// st_ksplat_write.hip runs them on the device, tests/native/ksplat_write_cpu_check.cpp on the CPU.
//
// Arithmetic: JS numbers (f64) in the order the rules are written, one rounding per operation
// (the library is built with contraction off), V8's Math.exp (st_jsmath.h).
#pragma once

#include "st_wr_encode.h"

namespace st {

constexpr uint32_t KS_CELLS = 1u << 21;  // cells per axis of the key
__host__ __device__ inline uint32_t ksplat_stride(int mode, int C) {
    return mode == 0 ? 44u + 12u * (uint32_t)C : mode == 1 ? 24u + 6u * (uint32_t)C : 24u + 3u * (uint32_t)C;
}

// H(t): round to nearest even from the double to binary16 (|t| >= 65520: +-Inf, NaN: 0x7E00,
// subnormals produced)
__host__ __device__ inline uint32_t ks_half(double t) {
    if (t != t) return 0x7E00u;
    const uint64_t w = __builtin_bit_cast(uint64_t, t);
    const uint32_t sign = (uint32_t)(w >> 48) & 0x8000u;
    const double a = __builtin_fabs(t);
    if (a >= 65520.0) return sign | 0x7C00u;
    if (a < 6.103515625e-05) {  // below 2^-14: code = a * 2^24 (exact) rounded to nearest even, 1024 = 2^-14
        const double x = a * 16777216.0, f = __builtin_floor(x), d = x - f;
        uint32_t m = (uint32_t)f;
        if (d > 0.5 || (d == 0.5 && (m & 1u))) ++m;
        return sign | m;
    }
    const uint64_t aw = w & 0x7fffffffffffffffull;
    const uint32_t e = (uint32_t)(aw >> 52) - 1023u + 15u;  // 1..30
    const uint64_t mant = aw & 0xfffffffffffffull, rem = mant & ((1ull << 42) - 1), half = 1ull << 41;
    uint32_t code = (e << 10) | (uint32_t)(mant >> 42);
    if (rem > half || (rem == half && (code & 1u))) ++code;  // a carry runs into the exponent
    return sign | code;
}

// a float32 column's bits unchanged (NaN payloads included), else Math.fround(v)
__host__ __device__ inline uint32_t ks_f32_bits(const WrCol &col, uint64_t row) {
    return col.t == ST_PLY_FLOAT ? static_cast<const uint32_t *>(col.p)[row]
                                 : __builtin_bit_cast(uint32_t, js::f32_store(ta_load(col.p, col.t, row)));
}

// the reader's decode of a centre code (read-ksplat.ts:278) and of a mode 2 harmonic byte (:242-243)
__host__ __device__ inline double ks_centre_decode(double k, double range, double ps, double c) {
    return (double)js::f32_store((k - range) * ps + c);
}
// (by255: b / 255 for b = 0..255 computed once, the same doubles; null: divide here)
__host__ __device__ inline double ks_sh8_decode(double b, double lo, double span, const double *by255) {
    return (double)js::f32_store(lo + (by255 ? by255[(uint32_t)b] : b / 255.0) * span);
}

// the bound under which ks_sh8_code need not look at k0's neighbours.  A decode is off its exact value
// lo + b / 255 * span by less than e = M * 2^-23 + 2^-149, M = max(|sh_min|, |sh_max|): the float32
// store's half step (2^-24 M, or 2^-150 below the normal range) plus three double roundings of
// magnitudes <= 3 M.  Two neighbouring codes' decodes are therefore at least step - 2 e apart, step
// = span / 255 (taken 2^-40 smaller for its own rounding), and with d0 = |dec(k0) - v| a neighbour
// is at least step - 2 e - d0 from v: not below d0 when d0 <= (step - 2 e) / 2.  Negative for a
// range too narrow for its magnitude: then every value takes the three decodes
__host__ __device__ inline double ks_sh8_fast(double sh_min, double sh_max) {
    const double M = __builtin_fmax(__builtin_fabs(sh_min), __builtin_fabs(sh_max));
    const double step = (sh_max - sh_min) / 255.0;
    return 0.5 * (step * (1.0 - 0x1p-40) - 2.0 * (M * 0x1p-23 + 0x1p-149));
}

// of the codes k0 - 1, k0, k0 + 1 inside [0, top] the one whose decoded value is nearest v: k0
// unless a neighbour is strictly nearer; of two strictly nearer neighbours the nearer, k0 - 1 on a tie
template <typename D>
__host__ __device__ inline uint32_t ks_nearest(double v, double k0, double top, D decode) {
    const double d0 = __builtin_fabs(decode(k0) - v);
    double best = k0, bd = d0;
    if (k0 - 1.0 >= 0.0) {
        const double d = __builtin_fabs(decode(k0 - 1.0) - v);
        if (d < bd) best = k0 - 1.0, bd = d;
    }
    if (k0 + 1.0 <= top) {
        const double d = __builtin_fabs(decode(k0 + 1.0) - v);
        if (d < bd) best = k0 + 1.0, bd = d;
    }
    return (uint32_t)best;
}

// the centre code of v in a bucket of centre c: 0 where floor((v - c) / ps + 0.5) + range is NaN
// (v NaN), else that value clamped to 0..65535 and then the nearest of it and its neighbours
__host__ __device__ inline uint32_t ks_centre_code(double v, double c, double ps, double range) {
    const double f = __builtin_floor((v - c) / ps + 0.5) + range;
    if (f != f) return 0;
    const double k0 = f < 0.0 ? 0.0 : f > 65535.0 ? 65535.0 : f;
    return ks_nearest(v, k0, 65535.0, [=](double k) { return ks_centre_decode(k, range, ps, c); });
}

// the mode 2 harmonic byte of v: Q8((v - lo) / span * 255), then the nearest of it and its neighbours
// (fast: where |dec(k0) - v| <= fast no neighbour can be strictly nearer -- ks_sh8_fast -- and the
// two other decodes are skipped; the result is the same)
__host__ __device__ inline uint32_t ks_sh8_code(double v, double lo, double span, const double *by255, double fast) {
    if (v != v) return 0;
    const double k0 = (double)q8((v - lo) / span * 255.0);
    if (__builtin_fabs(ks_sh8_decode(k0, lo, span, by255) - v) <= fast) return (uint32_t)k0;
    return ks_nearest(v, k0, 255.0, [=](double b) { return ks_sh8_decode(b, lo, span, by255); });
}

// little-endian stores to a record at any byte address (a word store where the address allows)
__host__ __device__ inline void ks_put16(uint8_t *p, uint32_t v) {
    if (((uintptr_t)p & 1) == 0) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    } else {
        p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8);
    }
}
__host__ __device__ inline void ks_put32(uint8_t *p, uint32_t v) {
    if (((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p) = v;
    } else {
        p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
    }
}

struct KsRecArgs {
    double ps, range;        // block / 2 / range and the quantisation range (modes 1 and 2)
    double sh_lo, sh_span;   // the header's float32 range widened: minimum and maximum - minimum (mode 2)
    int32_t mode, c_src, c_out;  // SH coefficients per channel of the table and of the file
    const double *by255;         // b / 255 for b = 0..255 (mode 2; null: divided where needed)
    double sh_fast;              // ks_sh8_fast of the range (mode 2)
};

// the column slot of file harmonic i (read-ksplat.ts:343-360 with the table's own column count:
// filterBands' mapping keeps f_rest_{channel * c_src + coeff} as coefficient coeff of the channel)
__host__ __device__ inline uint32_t ks_sh_slot(uint32_t i, uint32_t c_src) {
    uint32_t channel, coeff;
    if (i < 9) channel = i / 3, coeff = i % 3;
    else if (i < 24) channel = (i - 9) / 5, coeff = (i - 9) % 5 + 3;
    else channel = (i - 24) / 7, coeff = (i - 24) % 7 + 8;
    return 14 + channel * c_src + coeff;
}

// one record (ksplat_stride bytes at rec, any address) from row `row`; centre: the three float32
// of the record's bucket (modes 1 and 2; not read in mode 0)
template <bool F32>
__host__ __device__ inline void ksplat_encode(const WrCols &C, const KsRecArgs &A, uint64_t row, const float *centre,
                                              uint8_t *rec) {
    double u[4];
    unit_quat<F32>(C, row, u);
    uint32_t colour_at, sh_at;
    if (A.mode == 0) {
        for (int k = 0; k < 3; ++k) ks_put32(rec + 4 * k, ks_f32_bits(C.c[k], row));
        for (int k = 0; k < 3; ++k)
            ks_put32(rec + 12 + 4 * k, __builtin_bit_cast(uint32_t, js::f32_store(js::exp(wr_load<F32>(C.c[3 + k], row)))));
        for (int k = 0; k < 4; ++k) ks_put32(rec + 24 + 4 * k, __builtin_bit_cast(uint32_t, js::f32_store(u[k])));
        colour_at = 40, sh_at = 44;
    } else {
        for (int k = 0; k < 3; ++k)
            ks_put16(rec + 2 * k, ks_centre_code(wr_load<F32>(C.c[k], row), (double)centre[k], A.ps, A.range));
        for (int k = 0; k < 3; ++k) ks_put16(rec + 6 + 2 * k, ks_half(js::exp(wr_load<F32>(C.c[3 + k], row))));
        for (int k = 0; k < 4; ++k) ks_put16(rec + 12 + 2 * k, ks_half(u[k]));
        colour_at = 20, sh_at = 24;
    }
    for (int k = 0; k < 3; ++k)
        rec[colour_at + k] = (uint8_t)q8((wr_load<F32>(C.c[6 + k], row) * SH_C0 + 0.5) * 255.0);
    rec[colour_at + 3] = (uint8_t)q8(js::sigmoid(wr_load<F32>(C.c[9], row)) * 255.0);
    // the harmonics eight at a time: the batch's column loads are all issued before the first is used
    const uint32_t nsh = 3 * (uint32_t)A.c_out;
    for (uint32_t i0 = 0; i0 < nsh; i0 += 8) {
        double v[8];
        uint32_t w[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (i0 + j >= nsh) break;
            const WrCol &col = C.c[ks_sh_slot(i0 + j, (uint32_t)A.c_src)];
            if (A.mode == 0) w[j] = F32 ? static_cast<const uint32_t *>(col.p)[row] : ks_f32_bits(col, row);
            else v[j] = wr_load<F32>(col, row);
        }
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (i0 + j >= nsh) break;
            const uint32_t i = i0 + j;
            if (A.mode == 0) ks_put32(rec + sh_at + 4 * i, w[j]);
            else if (A.mode == 1) ks_put16(rec + sh_at + 2 * i, ks_half(v[j]));
            else rec[sh_at + i] = (uint8_t)ks_sh8_code(v[j], A.sh_lo, A.sh_span, A.by255, A.sh_fast);
        }
    }
}

// ---- the grid ------------------------------------------------------------------------------------
// cell_a(v): 0 for NaN or v < lo, else min(2^21 - 1, floor((v - lo) / B)); *clamped: v is not
// finite or the unclamped cell is >= 2^21
__host__ __device__ inline uint32_t ks_cell(double v, double lo, double B, bool *clamped) {
    *clamped = !(__builtin_fabs(v) < __builtin_inf());
    if (v != v || v < lo) return 0;
    const double f = __builtin_floor((v - lo) / B);
    if (f >= (double)KS_CELLS) {
        *clamped = true;
        return KS_CELLS - 1;
    }
    return (uint32_t)f;
}
// the bucket centre of a cell on one axis: fround(lo + (cell + 0.5) * B)
__host__ __device__ inline float ks_centre(double lo, uint32_t cell, double B) {
    return js::f32_store(lo + ((double)cell + 0.5) * B);
}

}  // namespace st
