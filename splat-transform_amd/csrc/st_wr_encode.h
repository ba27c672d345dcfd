// st_wr_encode.h -- the pieces the packed-format writers share (st_writers.hip, st_ksplat_write.hip):
// a column's element as a JS number, Q8, the unit quaternion of the rules (include/st_abi.h, "the
// .splat and .spz writers") and the store of an LDS slice to an output of any alignment.
#pragma once

#include "st_internal.h"
#include "st_jsmath.h"
#include "st_typed.h"

namespace st {

constexpr double SH_C0 = 0.28209479177387814;

// element `row` of a column as a JS number; F32: every column of the table is float32
template <bool F32>
__host__ __device__ inline double wr_load(const WrCol &col, uint64_t row) {
    if (F32) return (double)static_cast<const float *>(col.p)[row];
    return ta_load(col.p, col.t, row);
}

// Q8(t) = 0 for NaN, else min(255, max(0, floor(t + 0.5)))
__host__ __device__ inline uint32_t q8(double t) {
    if (t != t) return 0;
    const double f = __builtin_floor(t + 0.5);
    return f < 0.0 ? 0u : f > 255.0 ? 255u : (uint32_t)f;
}

// the unit quaternion of the rules: r / L for a finite L > 0, else (1, 0, 0, 0)
template <bool F32>
__host__ __device__ inline void unit_quat(const WrCols &C, uint64_t row, double u[4]) {
    double r[4];
    for (int k = 0; k < 4; ++k) r[k] = wr_load<F32>(C.c[10 + k], row);
    const double L = __builtin_sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
    if (L > 0.0 && L < __builtin_inf()) {
        for (int k = 0; k < 4; ++k) u[k] = r[k] / L;
    } else {
        u[0] = 1.0, u[1] = 0.0, u[2] = 0.0, u[3] = 0.0;
    }
}

// LDS words of a slice of `len` bytes laid out at any skew 0..3
constexpr uint32_t slice_words(uint32_t len) { return (len + 6) / 4 + 1; }

#ifdef __HIPCC__
// image bytes [shift, shift + bytes) of l32 -> g[0, bytes) where shift = g & 3: whole words between,
// single bytes at the two ends (a 256-lane workgroup)
__device__ inline void slice_out(const uint32_t *l32, uint32_t shift, uint32_t bytes, uint8_t *g) {
    if (!bytes) return;
    const uint8_t *l8 = reinterpret_cast<const uint8_t *>(l32);
    uint8_t *base = g - shift;  // 4-byte aligned
    const uint32_t end = shift + bytes;
    const uint32_t w0 = (shift + 3) >> 2, w1 = end >> 2;
    for (uint32_t i = w0 + threadIdx.x; i < w1; i += 256) reinterpret_cast<uint32_t *>(base)[i] = l32[i];
    const uint32_t head_end = w0 * 4 < end ? w0 * 4 : end;
    const uint32_t tail = w1 * 4 > head_end ? w1 * 4 : head_end;
    if (shift + threadIdx.x < head_end) base[shift + threadIdx.x] = l8[shift + threadIdx.x];
    if (tail + threadIdx.x < end) base[tail + threadIdx.x] = l8[tail + threadIdx.x];
}
#endif

}  // namespace st
