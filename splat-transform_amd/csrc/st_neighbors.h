// st_neighbors.h -- the rules of include/st_abi.h ("neighbour distances and outliers") as host/device
// functions, and a plain serial host form (dist_host: brute force over every pair; outliers_host: the
// kept rows).  The kernels of st_neighbors.hip and tests/native/neighbors_cpu_check.cpp both go
// through these functions, so they cannot disagree on a distance, a bound or a verdict.
//
// Everything is IEEE double on the column's element as a JS number, each operation rounded once in
// the order written (the library and the test program are built with -ffp-contract=off).
#ifndef ST_NEIGHBORS_H
#define ST_NEIGHBORS_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/st_abi.h"
#include "st_summary.h"

namespace st {
namespace nbr {

constexpr uint64_t NAN_BITS = 0x7ff8000000000000ull;  // dist_k of a row that is not placed
constexpr uint64_t INF_BITS = 0x7ff0000000000000ull;
constexpr int K_MAX = 32;
constexpr int LEAF_DEFAULT = 64, LEAF_MIN = 4, LEAF_MAX = 64;

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

__host__ __device__ inline bool finite(double v) {
    return (__builtin_bit_cast(uint64_t, v) & 0x7fffffffffffffffull) < INF_BITS;
}
__host__ __device__ inline bool placed(double x, double y, double z) { return finite(x) && finite(y) && finite(z); }

// between two placed rows: +Infinity when a difference or a square overflows, never NaN
__host__ __device__ inline double d2(double xi, double yi, double zi, double xj, double yj, double zj) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}

// one axis of the box bound: how far the query interval [qlo, qhi] and the node interval [lo, hi] are
// apart, by the subtraction d2 itself performs on the two nearest ends
__host__ __device__ inline double gap(double lo, double hi, double qlo, double qhi) {
    const double a = lo - qhi, b = qlo - hi;
    double g = 0.0;
    if (a > g) g = a;
    if (b > g) g = b;
    return g;
}

// A lower bound of the COMPUTED d2(i, j) for every placed i inside the query box and every placed j
// inside the node box.  No epsilon: rounding to nearest is monotone (u <= v implies fl(u) <= fl(v)) and
// symmetric (fl(-u) = -fl(u)).  Take one axis with the node above the query: x_j >= lo > qhi >= x_i,
// so x_j - x_i >= lo - qhi >= 0 as real numbers, hence |fl(x_i - x_j)| = fl(x_j - x_i) >= fl(lo - qhi)
// = g >= 0; an axis on which the intervals meet has g = 0 <= |dx|.  Squaring non-negative doubles and
// adding them are monotone in each operand under the same rounding, and the bound below repeats
// d2's operations in d2's order -- so bound <= d2, +Infinity included, bit for bit, whatever the
// magnitudes.  (A query box that is one point, qlo = qhi = the query, is the bound the search uses.)
// A node is pruned for a query when bound >= its k-th best so far: every pair inside has d2 >= that
// k-th best and could at most tie with it, which leaves the k-th smallest element of the multiset as
// it is.
__host__ __device__ inline double box_bound(const double nlo[3], const double nhi[3], const double qlo[3],
                                            const double qhi[3]) {
    const double gx = gap(nlo[0], nhi[0], qlo[0], qhi[0]), gy = gap(nlo[1], nhi[1], qlo[1], qhi[1]),
                 gz = gap(nlo[2], nhi[2], qlo[2], qhi[2]);
    return (gx * gx + gy * gy) + gz * gz;
}

// v into best[0..k), ascending, when it is below best[k - 1] (stride: elements between two entries)
template <typename P>
__host__ __device__ inline void insert_best(P best, int stride, int k, double v) {
    if (!(v < best[(k - 1) * stride])) return;
    int j = k - 1;
    for (; j > 0 && best[(j - 1) * stride] > v; --j) best[j * stride] = best[(j - 1) * stride];
    best[j * stride] = v;
}

// the locality key: 10 bits per axis over the placed rows' extents [lo, hi].  An axis without extent,
// or with one that leaves the double range, gives 0.  No result depends on it
__host__ __device__ inline uint32_t cell(double v, double lo, double hi) {
    const double t = (v - lo) / (hi - lo);  // 0/0 and Infinity/Infinity are NaN, anything/Infinity is 0
    if (!(t > 0.0)) return 0;
    const double s = t * 1024.0;
    return s >= 1023.0 ? 1023u : (uint32_t)s;
}
__host__ __device__ inline uint32_t spread3(uint32_t v) {  // abcd -> a00b00c00d
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__host__ __device__ inline uint32_t morton30(uint32_t cx, uint32_t cy, uint32_t cz) {
    return spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2);
}

__host__ __device__ inline bool k_ok(int32_t k) { return k >= 1 && k <= K_MAX; }
// filterOutliers' arguments: the mode is known and the value is no NaN
__host__ __device__ inline bool outlier_args_ok(int32_t mode, double value) {
    return (mode == ST_OUTLIER_SIGMA || mode == ST_OUTLIER_DISTANCE) && value == value;
}
__host__ __device__ inline double threshold(int32_t mode, double value, double mean, double std_dev) {
    if (mode == ST_OUTLIER_DISTANCE) return value;
    const double w = value * std_dev;
    return mean + w;
}
__host__ __device__ inline bool keep(double dist, double t) { return dist <= t; }

// ---- the serial host form --------------------------------------------------------------------------
struct Col {
    const void *ptr;
    int32_t type;
};

// out[i] = dist_k(i), every pair evaluated
inline void dist_host(const Col xyz[3], uint64_t n, int k, double *out) {
    std::vector<double> x(n), y(n), z(n);
    std::vector<uint8_t> ok(n);
    for (uint64_t i = 0; i < n; ++i) {
        x[i] = value_at(xyz[0].ptr, xyz[0].type, i);
        y[i] = value_at(xyz[1].ptr, xyz[1].type, i);
        z[i] = value_at(xyz[2].ptr, xyz[2].type, i);
        ok[i] = placed(x[i], y[i], z[i]);
    }
    const double inf = __builtin_bit_cast(double, INF_BITS);
    for (uint64_t i = 0; i < n; ++i) {
        if (!ok[i]) {
            out[i] = __builtin_bit_cast(double, NAN_BITS);
            continue;
        }
        double best[K_MAX];
        for (int j = 0; j < k; ++j) best[j] = inf;
        for (uint64_t j = 0; j < n; ++j)
            if (j != i && ok[j]) insert_best(best, 1, k, d2(x[i], y[i], z[i], x[j], y[j], z[j]));
        out[i] = __builtin_sqrt(best[k - 1]);
    }
}

// the threshold of a distance column (the column summary's mean and std_dev over its finite values)
inline double threshold_host(const double *dist, uint64_t n, int32_t mode, double value) {
    if (mode == ST_OUTLIER_DISTANCE) return value;
    st_col_summary s;
    sm::summarize_host(ST_PLY_DOUBLE, dist, n, false, sm::FLUSH_DEFAULT, &s, nullptr);
    return threshold(mode, value, s.mean, s.std_dev);
}

inline std::vector<uint32_t> outliers_host(const double *dist, uint64_t n, int32_t mode, double value) {
    const double t = threshold_host(dist, n, mode, value);
    std::vector<uint32_t> rows;
    for (uint64_t i = 0; i < n; ++i)
        if (keep(dist[i], t)) rows.push_back((uint32_t)i);
    return rows;
}

}  // namespace nbr
}  // namespace st

#endif  // ST_NEIGHBORS_H
