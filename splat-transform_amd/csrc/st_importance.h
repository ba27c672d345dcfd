// st_importance.h -- the rules of include/st_abi.h ("importance, decimation and crops") as
// host/device functions, and a plain serial host form of the three selections (scores_host,
// order_host, top_host, box_host, sphere_host).  The kernels of st_importance.hip and
// tests/native/importance_cpu_check.cpp both go through these functions, so they cannot disagree on
// a score, a key or a verdict.
//
// Everything is IEEE double on the column's element as a JS number, each operation rounded once in
// the order written (the library and the test program are built with -ffp-contract=off).
#ifndef ST_IMPORTANCE_H
#define ST_IMPORTANCE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/st_abi.h"
#include "st_jsmath.h"

namespace st {
namespace imp {

constexpr uint64_t NAN_BITS = 0x7ff8000000000000ull;  // every NaN score is stored as this one

// the element at row i of a column of any st_ply_type as a JS number (exact)
__host__ __device__ inline double value_at(const void *p, int32_t type, uint64_t i) {
    switch (type) {
        case ST_PLY_CHAR: return (double)((const int8_t *)p)[i];
        case ST_PLY_UCHAR: return (double)((const uint8_t *)p)[i];
        case ST_PLY_SHORT: return (double)((const int16_t *)p)[i];
        case ST_PLY_USHORT: return (double)((const uint16_t *)p)[i];
        case ST_PLY_INT: return (double)((const int32_t *)p)[i];
        case ST_PLY_UINT: return (double)((const uint32_t *)p)[i];
        case ST_PLY_FLOAT: return (double)((const float *)p)[i];
        default: return ((const double *)p)[i];
    }
}

// exp(scale sum) * sigmoid(opacity).  The product of a number and a number can only be NaN as
// Infinity * 0; whichever NaN an operand carried or the multiplier made (the sign of a generated
// NaN differs between processors), the score is the one quiet NaN
__host__ __device__ inline double score(double s0, double s1, double s2, double opacity) {
    const double s = (s0 + s1) + s2;
    const double v = js::exp(s) * js::sigmoid(opacity);
    return v != v ? __builtin_bit_cast(double, NAN_BITS) : v;
}

// larger is more important; every NaN is 0, +0 is 1, +Infinity is 0x7ff0000000000001
__host__ __device__ inline uint64_t key_of_score(double v) {
    return v != v ? 0ull : __builtin_bit_cast(uint64_t, v) + 1ull;
}

__host__ __device__ inline bool in_box(double x, double y, double z, const double lo[3], const double hi[3]) {
    return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
}

__host__ __device__ inline bool in_sphere(double x, double y, double z, const double c[3], double radius) {
    const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
    return ((dx * dx + dy * dy) + dz * dz) < radius * radius;
}

// decimate's m; false: the amount is not allowed in that mode
inline bool decimate_rows(int32_t mode, double amount, uint64_t n, uint64_t *m) {
    if (mode == ST_DECIMATE_COUNT) {
        if (!(amount >= 0.0 && amount < 9007199254740992.0)) return false;  // NaN fails both
        const uint64_t k = (uint64_t)amount;
        if ((double)k != amount) return false;
        *m = std::min(k, n);
        return true;
    }
    if (mode == ST_DECIMATE_FRACTION) {
        if (!(amount >= 0.0 && amount <= 1.0)) return false;
        const double p = __builtin_floor(amount * (double)n);
        *m = std::min(n, (uint64_t)p);
        return true;
    }
    return false;
}

// ---- the serial host form --------------------------------------------------------------------------
struct Col {
    const void *ptr;  // null: the column is missing (box and sphere read NaN)
    int32_t type;
};

inline void scores_host(const Col sc[3], const Col &op, uint64_t n, double *out) {
    for (uint64_t i = 0; i < n; ++i)
        out[i] = score(value_at(sc[0].ptr, sc[0].type, i), value_at(sc[1].ptr, sc[1].type, i),
                       value_at(sc[2].ptr, sc[2].type, i), value_at(op.ptr, op.type, i));
}

// order[j] = the row of rank j
inline void order_host(const double *scores, uint64_t n, uint32_t *order) {
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::stable_sort(order, order + n,
                     [&](uint32_t a, uint32_t b) { return key_of_score(scores[a]) > key_of_score(scores[b]); });
}

// the rows of rank < m, ascending (m <= n)
inline std::vector<uint32_t> top_host(const double *scores, uint64_t n, uint64_t m) {
    std::vector<uint32_t> order(n);
    order_host(scores, n, order.data());
    std::vector<uint32_t> rows(order.begin(), order.begin() + m);
    std::sort(rows.begin(), rows.end());
    return rows;
}

inline double coord(const Col &c, uint64_t i) {
    return c.ptr ? value_at(c.ptr, c.type, i) : __builtin_bit_cast(double, NAN_BITS);
}

inline std::vector<uint32_t> box_host(const Col xyz[3], uint64_t n, const double lo[3], const double hi[3]) {
    std::vector<uint32_t> rows;
    for (uint64_t i = 0; i < n; ++i)
        if (in_box(coord(xyz[0], i), coord(xyz[1], i), coord(xyz[2], i), lo, hi)) rows.push_back((uint32_t)i);
    return rows;
}

inline std::vector<uint32_t> sphere_host(const Col xyz[3], uint64_t n, const double c[3], double radius) {
    std::vector<uint32_t> rows;
    for (uint64_t i = 0; i < n; ++i)
        if (in_sphere(coord(xyz[0], i), coord(xyz[1], i), coord(xyz[2], i), c, radius)) rows.push_back((uint32_t)i);
    return rows;
}

}  // namespace imp
}  // namespace st

#endif  // ST_IMPORTANCE_H
