// st_clusters.h -- the rules of include/st_abi.h ("clusters") as host/device functions, and a plain
// serial host form (clusters_host: every pair by brute force, a sequential union-find, min-index
// labels; filter_clusters_host: the kept rows).  The kernels of st_clusters.hip and
// tests/native/clusters_cpu_check.cpp both go through these functions, so they cannot disagree on a
// link, a bound or a verdict.  placed, d2 and box_bound are those of st_neighbors.h, unchanged.
//
// Everything is IEEE double on the column's element as a JS number, each operation rounded once in
// the order written (the library and the test program are built with -ffp-contract=off).
//
// The partition into components is a property of the data alone.  The LABELS additionally depend on
// the numbering of the rows, by definition: label(i) is the smallest row index of i's component.
#ifndef ST_CLUSTERS_H
#define ST_CLUSTERS_H

#include <stdint.h>

#include <vector>

#include "../../include/st_abi.h"
#include "st_neighbors.h"

namespace st {
namespace cl {

constexpr uint32_t NONE = 0xFFFFFFFFu;  // label of a row that is not placed

// any double >= 0, +Infinity included; NaN and negative values (-0 is 0) are refused
__host__ __device__ inline bool radius_ok(double radius) { return radius >= 0.0; }
// one multiplication; may be +Infinity, and 0 for a radius whose square underflows
__host__ __device__ inline double r2_of(double radius) { return radius * radius; }
// between two placed rows i != j
__host__ __device__ inline bool link(double d2, double r2) { return d2 <= r2; }

// cluster_min as decimate's count: a finite, non-negative, integer-valued double below 2^53
__host__ __device__ inline bool min_ok(double m) {
    if (!(m >= 0.0 && m < 9007199254740992.0)) return false;  // NaN fails both
    return (double)(uint64_t)m == m;
}
__host__ __device__ inline bool mode_ok(int32_t mode) { return mode == ST_CLUSTER_MIN_SIZE || mode == ST_CLUSTER_LARGEST; }
// filterClusters' arguments (cluster_min counts in ST_CLUSTER_MIN_SIZE only)
__host__ __device__ inline bool args_ok(double radius, int32_t mode, double cluster_min) {
    return radius_ok(radius) && mode_ok(mode) && (mode != ST_CLUSTER_MIN_SIZE || min_ok(cluster_min));
}
// the verdict on a row: size 0 is a row that is not placed and goes in either mode
__host__ __device__ inline bool keep(int32_t mode, uint32_t size, double cluster_min, uint32_t largest) {
    if (size == 0) return false;
    return mode == ST_CLUSTER_LARGEST ? size == largest : (double)size >= cluster_min;
}

// one axis of the far bound: the larger of the two end-to-end subtractions
__host__ __device__ inline double reach(double lo, double hi, double qlo, double qhi) {
    const double a = hi - qlo, b = qhi - lo;
    double f = a;
    if (b > f) f = b;
    return f;
}

// An upper bound of the COMPUTED d2(i, j) for every placed i inside the query box and every placed j
// inside the node box -- the counterpart of nbr::box_bound, by the same argument and again with no
// epsilon.  Take one axis: qlo <= x_i <= qhi and lo <= x_j <= hi give, as real numbers,
// x_j - x_i <= hi - qlo and x_i - x_j <= qhi - lo.  Rounding to nearest is monotone (u <= v implies
// fl(u) <= fl(v)) and symmetric (fl(-u) = -fl(u)), so |fl(x_i - x_j)| = max(fl(x_i - x_j), fl(x_j -
// x_i)) <= max(fl(qhi - lo), fl(hi - qlo)) = f, and f >= 0.  Squaring non-negative doubles and adding
// them are monotone in each operand under the same rounding, and the bound below repeats d2's
// operations in d2's order -- so bound >= d2, +Infinity included, bit for bit, whatever the
// magnitudes.  It is never NaN: the ends are finite, a difference that overflows is +-Infinity, the
// larger of the two is then +Infinity, and Infinity is only ever squared and added.
// A node with far_bound(box, box) <= r2 is a CLIQUE: every two of its rows link.  A row q with
// far_bound(node box, q, q) <= r2 links to every row of the node without one d2.
__host__ __device__ inline double far_bound(const double nlo[3], const double nhi[3], const double qlo[3],
                                            const double qhi[3]) {
    const double fx = reach(nlo[0], nhi[0], qlo[0], qhi[0]), fy = reach(nlo[1], nhi[1], qlo[1], qhi[1]),
                 fz = reach(nlo[2], nhi[2], qlo[2], qhi[2]);
    return (fx * fx + fy * fy) + fz * fz;
}

// ---- the serial host form --------------------------------------------------------------------------
// label[i], size[i] of every row (either may be null); returns the largest size.  radius_ok(radius)
// is the caller's to check
inline uint32_t clusters_host(const nbr::Col xyz[3], uint64_t n, double radius, uint32_t *label, uint32_t *size) {
    std::vector<double> x(n), y(n), z(n);
    std::vector<uint32_t> parent(n), count(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
        x[i] = nbr::value_at(xyz[0].ptr, xyz[0].type, i);
        y[i] = nbr::value_at(xyz[1].ptr, xyz[1].type, i);
        z[i] = nbr::value_at(xyz[2].ptr, xyz[2].type, i);
        parent[i] = nbr::placed(x[i], y[i], z[i]) ? (uint32_t)i : NONE;
    }
    auto find = [&](uint32_t v) {
        while (parent[v] != v) v = parent[v] = parent[parent[v]];
        return v;
    };
    const double r2 = r2_of(radius);
    for (uint64_t i = 0; i < n; ++i) {
        if (parent[i] == NONE) continue;
        for (uint64_t j = i + 1; j < n; ++j) {
            if (parent[j] == NONE || !link(nbr::d2(x[i], y[i], z[i], x[j], y[j], z[j]), r2)) continue;
            const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
            if (a < b) parent[b] = a;  // the larger root under the smaller: a root is its tree's minimum
            else if (b < a) parent[a] = b;
        }
    }
    uint32_t largest = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (parent[i] != NONE) {
            const uint32_t c = ++count[find((uint32_t)i)];
            if (c > largest) largest = c;
        }
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t l = parent[i] == NONE ? NONE : find((uint32_t)i);
        if (label) label[i] = l;
        if (size) size[i] = l == NONE ? 0u : count[l];
    }
    return largest;
}

// the rows filterClusters keeps, ascending; args_ok is the caller's to check
inline std::vector<uint32_t> filter_clusters_host(const nbr::Col xyz[3], uint64_t n, double radius, int32_t mode,
                                                  double cluster_min) {
    std::vector<uint32_t> size(n), rows;
    const uint32_t largest = clusters_host(xyz, n, radius, nullptr, size.data());
    for (uint64_t i = 0; i < n; ++i)
        if (keep(mode, size[i], cluster_min, largest)) rows.push_back((uint32_t)i);
    return rows;
}

}  // namespace cl
}  // namespace st

#endif  // ST_CLUSTERS_H
