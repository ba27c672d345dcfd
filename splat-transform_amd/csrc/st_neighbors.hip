// st_neighbors.hip -- include/st_abi.h's "neighbour distances and outliers" on the device.  The rules
// are the functions of st_neighbors.h; this file finds, for every placed row, the k smallest d2 to
// the other placed rows without evaluating every pair.
//
//   k_nb_extent    the placed rows' count and their extents per axis (order-preserving u64 keys of
//                  the doubles, wave reductions, integer atomics)
//   k_nb_keys      a 30-bit Morton key per placed row (nbr::morton30: locality only); a row that is not
//                  placed gets bit 30, so radix_sort_u32_iota leaves the P placed rows first
//   k_nb_gather    the sorted rows' positions as float4 (x, y and z all float32) or double4
//   k_nb_leaves    leaf j = sorted rows [j L, (j + 1) L): the exact min / max box of its members
//   k_nb_level     node j of level l = the boxes of nodes 8j .. 8j + 7 of level l - 1 merged: an
//                  implicit 8-ary tree, no pointers; one launch per level
//   k_nb_search    one wave (a workgroup of 64) per leaf, its members the 64 queries, a lane each.
//                  A lane's k best d2 are a sorted column of a [k][64] LDS array.  Seed: the wave's
//                  own leaf and SEED leaves either side in sorted order.  Then a depth-first walk from
//                  the root over a stack in LDS that every lane writes alike: a node is pruned when
//                  no lane has nbr::box_bound(node box, its own query) below its own k-th best (a
//                  wave vote).  That prunes whatever the bound of the leaf's box against the largest
//                  k-th best of the lanes would, and more -- see box_bound for why it needs no
//                  tolerance and why the test is >= (more than k coincident rows make the k-th best
//                  0, and everything is pruned).  A leaf that survives is staged in LDS as doubles
//                  and every lane that voted for it tests all of its members.  Both position forms
//                  compute in f64.
//   k_nb_fill      dist_k of every row starts as the NaN of a row that is not placed
//   k_nb_flags     keep iff dist <= t, t from the summary's mean and std_dev read on the host
// Nothing here depends on the order in which atomics arrive: the atomics are integer minima, maxima
// and counts.  Workspace slots carry the caller's tag.
// The build -- extent, keys, sort, gather, leaf boxes and levels -- is nbt::build_tree (st_nbtree.h):
// st_clusters.hip searches the same tree.
#include <cstdlib>
#include <cstring>

#include "st_internal.h"
#include "st_nbtree.h"
#include "st_neighbors.h"

namespace st {
namespace {

using namespace nbr;
using namespace nbt;
typedef unsigned long long ull;

constexpr int SEED = 1;          // leaves scanned either side of the wave's own before the walk

struct Extent {  // device record of k_nb_extent
    ull lo[3], hi[3];  // sm::key_of(ST_PLY_DOUBLE) of the extremes
    ull placed;
};
struct Counters {
    ull pairs, nodes;
};

__device__ inline ull dkey(double v) { return sm::key_of(ST_PLY_DOUBLE, __builtin_bit_cast(uint64_t, v)); }
__device__ inline double dkey_inv(ull k) { return __builtin_bit_cast(double, sm::key_inv(ST_PLY_DOUBLE, k)); }

__device__ inline ull wave_min(ull v) {
    for (int o = 32; o > 0; o >>= 1) {
        const ull w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ inline ull wave_max(ull v) {
    for (int o = 32; o > 0; o >>= 1) {
        const ull w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline ull wave_sum(ull v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_nb_extent(const NCols cs, uint64_t n, Extent *__restrict__ ex) {
    ull lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0}, cnt = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v[3] = {value_at(cs.p[0], cs.type[0], i), value_at(cs.p[1], cs.type[1], i),
                             value_at(cs.p[2], cs.type[2], i)};
        if (!placed(v[0], v[1], v[2])) continue;
        ++cnt;
        for (int a = 0; a < 3; ++a) {
            const ull k = dkey(v[a]);
            lo[a] = k < lo[a] ? k : lo[a];
            hi[a] = k > hi[a] ? k : hi[a];
        }
    }
    cnt = wave_sum(cnt);
    for (int a = 0; a < 3; ++a) lo[a] = wave_min(lo[a]), hi[a] = wave_max(hi[a]);
    if ((threadIdx.x & 63) == 0 && cnt) {
        atomicAdd(&ex->placed, cnt);
        for (int a = 0; a < 3; ++a) atomicMin(&ex->lo[a], lo[a]), atomicMax(&ex->hi[a], hi[a]);
    }
}

__global__ __launch_bounds__(256) void k_nb_keys(const NCols cs, uint64_t n, const Extent *__restrict__ ex,
                                                 uint32_t *__restrict__ keys) {
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = dkey_inv(ex->lo[a]), hi[a] = dkey_inv(ex->hi[a]);  // read only when a row is placed
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = value_at(cs.p[0], cs.type[0], i), y = value_at(cs.p[1], cs.type[1], i),
                     z = value_at(cs.p[2], cs.type[2], i);
        keys[i] = placed(x, y, z) ? morton30(cell(x, lo[0], hi[0]), cell(y, lo[1], hi[1]), cell(z, lo[2], hi[2]))
                                  : (1u << 30);
    }
}

template <typename T4>
__device__ inline T4 make4(double x, double y, double z);
template <>
__device__ inline float4 make4<float4>(double x, double y, double z) {
    return make_float4((float)x, (float)y, (float)z, 0.0f);  // exact: the columns are float32
}
template <>
__device__ inline double4 make4<double4>(double x, double y, double z) {
    return make_double4(x, y, z, 0.0);
}

// pos[s] = the position of sorted row s < P
template <typename T4>
__global__ __launch_bounds__(256) void k_nb_gather(const NCols cs, const uint32_t *__restrict__ order, uint64_t P,
                                                   T4 *__restrict__ pos) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < P; s += stride) {
        const uint64_t i = order[s];
        pos[s] = make4<T4>(value_at(cs.p[0], cs.type[0], i), value_at(cs.p[1], cs.type[1], i),
                           value_at(cs.p[2], cs.type[2], i));
    }
}

// one thread per leaf (at most 64 members, read in sorted order)
template <typename T4>
__global__ __launch_bounds__(256) void k_nb_leaves(const T4 *__restrict__ pos, uint64_t P, int L, uint32_t leaves,
                                                   double *__restrict__ box) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= leaves) return;
    const uint64_t s0 = j * (uint64_t)L, s1 = s0 + L < P ? s0 + L : P;  // s0 < P: leaves = ceil(P / L)
    T4 p = pos[s0];
    double lo[3] = {(double)p.x, (double)p.y, (double)p.z}, hi[3] = {lo[0], lo[1], lo[2]};
    for (uint64_t s = s0 + 1; s < s1; ++s) {
        p = pos[s];
        const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
        for (int a = 0; a < 3; ++a) lo[a] = v[a] < lo[a] ? v[a] : lo[a], hi[a] = v[a] > hi[a] ? v[a] : hi[a];
    }
    double *b = box + j * 6;
    for (int a = 0; a < 3; ++a) b[a] = lo[a], b[3 + a] = hi[a];
}

// child: cnt_child boxes; parent j merges children [8j, min(8j + 8, cnt_child))
__global__ __launch_bounds__(256) void k_nb_level(const double *__restrict__ child, uint32_t cnt_child,
                                                  double *__restrict__ parent, uint32_t cnt_parent) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt_parent) return;
    const uint64_t c0 = j * 8, c1 = c0 + 8 < cnt_child ? c0 + 8 : cnt_child;  // c0 < cnt_child
    double b[6];
    for (int a = 0; a < 6; ++a) b[a] = child[c0 * 6 + a];
    for (uint64_t c = c0 + 1; c < c1; ++c)
        for (int a = 0; a < 3; ++a) {
            const double l = child[c * 6 + a], h = child[c * 6 + 3 + a];
            b[a] = l < b[a] ? l : b[a];
            b[3 + a] = h > b[3 + a] ? h : b[3 + a];
        }
    for (int a = 0; a < 6; ++a) parent[j * 6 + a] = b[a];
}

__global__ __launch_bounds__(256) void k_nb_fill(double *__restrict__ dist, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dist[i] = __builtin_bit_cast(double, NAN_BITS);
}

// A workgroup is one wave: __syncthreads() orders the wave's LDS traffic and costs no wait.  Every
// branch around one is taken by all lanes alike (the conditions are wave votes, kernel arguments or
// stack entries every lane wrote alike).
template <typename T4, int KCAP>
__global__ __launch_bounds__(64) void k_nb_search(const T4 *__restrict__ pos, const uint32_t *__restrict__ order,
                                                  uint64_t P, int L, int k, const double *__restrict__ box,
                                                  const Tree tr, double *__restrict__ dist,
                                                  Counters *__restrict__ counters) {
    __shared__ double best[KCAP * 64];  // best[j * 64 + lane]: the lane's j-th smallest d2 so far
    __shared__ double sx[64], sy[64], sz[64];  // the staged candidate leaf
    __shared__ uint32_t stack[STACK];  // level << 28 | node is not enough for 2^30 leaves: two words
    __shared__ uint32_t stack_level[STACK];
    const int lane = threadIdx.x;
    const uint32_t leaf = blockIdx.x;  // < tr.cnt[0]
    const uint64_t q0 = (uint64_t)leaf * L;
    const int nq = (int)(P - q0 < (uint64_t)L ? P - q0 : (uint64_t)L);  // >= 1
    const bool active = lane < nq;
    double qx = 0, qy = 0, qz = 0;
    if (active) {
        const T4 p = pos[q0 + lane];
        qx = (double)p.x, qy = (double)p.y, qz = (double)p.z;
    }
    for (int j = 0; j < k; ++j) best[j * 64 + lane] = __builtin_bit_cast(double, INF_BITS);
    const double q[3] = {qx, qy, qz};
    double *mine = best + lane;
    ull pairs = 0, nodes = 0;  // pairs: this lane's; nodes: the wave's (the same in every lane)
    double kth = __builtin_bit_cast(double, INF_BITS);  // the lane's k-th best so far

    // every member of leaf c against the queries of the lanes that want it
    auto scan_leaf = [&](uint32_t c, bool wanted) {
        const uint64_t s0 = (uint64_t)c * L;
        const int m = (int)(P - s0 < (uint64_t)L ? P - s0 : (uint64_t)L);
        __syncthreads();  // the previous leaf has been read
        if (lane < m) {
            const T4 p = pos[s0 + lane];
            sx[lane] = (double)p.x, sy[lane] = (double)p.y, sz[lane] = (double)p.z;
        }
        __syncthreads();
        if (wanted) {
            const int self = c == leaf ? lane : -1;
            for (int j = 0; j < m; ++j)
                if (j != self) insert_best(mine, 64, k, d2(qx, qy, qz, sx[j], sy[j], sz[j]));
            pairs += (ull)(m - (c == leaf ? 1 : 0));
            kth = mine[(k - 1) * 64];
        }
    };

    const uint32_t leaves = tr.cnt[0];
    const uint32_t seed_lo = leaf > (uint32_t)SEED ? leaf - SEED : 0;
    const uint32_t seed_hi = leaves - 1 - leaf > (uint32_t)SEED ? leaf + SEED : leaves - 1;
    scan_leaf(leaf, active);
    for (uint32_t c = seed_lo; c <= seed_hi; ++c)
        if (c != leaf) scan_leaf(c, active);

    int sp = 0;
    stack[0] = 0, stack_level[0] = (uint32_t)(tr.levels - 1);
    sp = 1;
    while (sp > 0) {
        --sp;
        const uint32_t node = stack[sp], level = stack_level[sp];
        if (level == 0 && node >= seed_lo && node <= seed_hi) continue;  // scanned by the seed
        const double *b = box + ((uint64_t)tr.off[level] + node) * 6;
        const double nlo[3] = {b[0], b[1], b[2]}, nhi[3] = {b[3], b[4], b[5]};
        ++nodes;
        const bool wanted = active && box_bound(nlo, nhi, q, q) < kth;
        if (__ballot(wanted) == 0) continue;  // bound >= the k-th best in every lane
        if (level == 0) {
            scan_leaf(node, wanted);
            continue;
        }
        // the children in descending order: the walk meets them in sorted order.  At most 8 pushed
        // for one popped: sp <= 7 * levels + 1 <= STACK
        const uint32_t cl = level - 1, ccnt = tr.cnt[cl];
        const uint64_t c0 = (uint64_t)node * 8;
        const uint32_t nc = (uint32_t)(ccnt - c0 < 8 ? ccnt - c0 : 8);  // c0 < ccnt
        for (uint32_t c = nc; c-- > 0;) {
            stack[sp] = (uint32_t)c0 + c, stack_level[sp] = cl;
            ++sp;
        }
    }
    if (active) dist[order[q0 + lane]] = __builtin_sqrt(mine[(k - 1) * 64]);
    pairs = wave_sum(pairs);
    if (lane == 0) atomicAdd(&counters->pairs, pairs), atomicAdd(&counters->nodes, nodes);
}

__global__ __launch_bounds__(256) void k_nb_flags(const double *__restrict__ dist, uint64_t n, double t,
                                                  uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flags[i] = keep(dist[i], t) ? 1u : 0u;
}

struct Stats {
    uint64_t rows = 0, placed = 0, leaves = 0, levels = 0, pairs = 0, nodes = 0;
};
void publish(st_ctx *c, const Stats &s) {
    c->last_neighbor_stats = "{\"rows\": " + std::to_string(s.rows) + ", \"placed\": " + std::to_string(s.placed) +
                             ", \"leaves\": " + std::to_string(s.leaves) + ", \"levels\": " + std::to_string(s.levels) +
                             ", \"pairs\": " + std::to_string(s.pairs) + ", \"nodes\": " + std::to_string(s.nodes) + "}";
}

template <typename T4>
void gather_and_boxes(st_ctx *c, const NCols &cs, const std::string &tag, Built &T) {
    auto *pos = wsT<T4>(c, tag + ".nb.pos", T.P);
    T.pos = pos;
    {
        KTimer kt(c, "nb.gather");
        hipLaunchKernelGGL(k_nb_gather<T4>, dim3(grid_for(T.P, 256, 8192)), dim3(256), 0, c->stream, cs,
                           (const uint32_t *)T.order, T.P, pos);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "nb.boxes");
        const Tree &tr = T.tr;
        hipLaunchKernelGGL(k_nb_leaves<T4>, dim3(grid_for(tr.cnt[0], 256)), dim3(256), 0, c->stream, (const T4 *)pos, T.P,
                           T.L, tr.cnt[0], T.box);
        ST_LAUNCH_CHECK();
        for (int l = 1; l < tr.levels; ++l) {
            hipLaunchKernelGGL(k_nb_level, dim3(grid_for(tr.cnt[l], 256)), dim3(256), 0, c->stream,
                               (const double *)(T.box + (uint64_t)tr.off[l - 1] * 6), tr.cnt[l - 1],
                               T.box + (uint64_t)tr.off[l] * 6, tr.cnt[l]);
            ST_LAUNCH_CHECK();
        }
    }
}

template <typename T4>
void search(st_ctx *c, const Built &T, int k, double *dist, Counters *d_cnt) {
    KTimer kt(c, "nb.search");
    const dim3 g(T.tr.cnt[0]);
    if (k <= 8)
        hipLaunchKernelGGL((k_nb_search<T4, 8>), g, dim3(64), 0, c->stream, (const T4 *)T.pos, (const uint32_t *)T.order,
                           T.P, T.L, k, (const double *)T.box, T.tr, dist, d_cnt);
    else
        hipLaunchKernelGGL((k_nb_search<T4, K_MAX>), g, dim3(64), 0, c->stream, (const T4 *)T.pos,
                           (const uint32_t *)T.order, T.P, T.L, k, (const double *)T.box, T.tr, dist, d_cnt);
    ST_LAUNCH_CHECK();
}

}  // namespace

namespace nbt {

const char *const XYZ[3] = {"x", "y", "z"};

NCols xyz_cols(const st_ttable *t, const char *what) {
    NCols cs{};
    for (int k = 0; k < 3; ++k) {
        int col = -1;
        for (int i = 0; i < t->ncol && col < 0; ++i)
            if (std::strcmp(t->names[i], XYZ[k]) == 0) col = i;  // the first of a name
        if (col < 0) throw Error(ST_ERR_ARG, std::string(what) + ": the table has no column " + XYZ[k]);
        ST_REQUIRE(type_size(t->types[col]) > 0, ST_ERR_ARG, std::string("column ") + XYZ[k] + " has a bad type");
        cs.p[k] = t->cols[col];
        cs.type[k] = t->types[col];
    }
    return cs;
}

int leaf_size() {  // read per call (tests set it around one call)
    if (const char *e = getenv("ST_KNN_LEAF")) {
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && v >= LEAF_MIN && v <= LEAF_MAX) return (int)v;
    }
    return LEAF_DEFAULT;
}

void build_tree(st_ctx *c, const NCols &cs, uint64_t n, const std::string &tag, Built &T) {
    T = Built{};
    T.L = leaf_size();
    auto *ex = wsT<Extent>(c, tag + ".nb.extent", 1);
    auto *h = static_cast<Extent *>(pinned_slot(c, "nb.host.extent", 2 * sizeof(Extent)));
    Extent *h_ex0 = h, *h_ex = h + 1;  // what goes up, what comes back
    *h_ex0 = Extent{{~0ull, ~0ull, ~0ull}, {0, 0, 0}, 0};
    ST_HIP(hipMemcpyAsync(ex, h_ex0, sizeof(Extent), hipMemcpyHostToDevice, c->stream));
    {
        KTimer kt(c, "nb.extent");
        hipLaunchKernelGGL(k_nb_extent, dim3(grid_for(n, 256 * 8, 2048)), dim3(256), 0, c->stream, cs, n, ex);
        ST_LAUNCH_CHECK();
    }
    ST_HIP(hipMemcpyAsync(h_ex, ex, sizeof(Extent), hipMemcpyDeviceToHost, c->stream));
    auto *keys = wsT<uint32_t>(c, tag + ".nb.keys", n);
    auto *skeys = wsT<uint32_t>(c, tag + ".nb.skeys", n);
    T.order = wsT<uint32_t>(c, tag + ".nb.order", n);
    {
        KTimer kt(c, "nb.keys");
        hipLaunchKernelGGL(k_nb_keys, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, cs, n, (const Extent *)ex, keys);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "nb.sort");
        radix_sort_u32_iota(c, keys, n, 0, 32, skeys, T.order, tag + ".nb.sort");
    }
    ST_HIP(hipStreamSynchronize(c->stream));
    T.P = h_ex->placed;
    ST_REQUIRE(T.P <= n, ST_ERR_INTERNAL, "neighbors: more placed rows than rows");
    if (!T.P) return;
    Tree &tr = T.tr;
    uint64_t total = 0;
    uint64_t cnt = (T.P + T.L - 1) / T.L;
    for (;;) {
        ST_REQUIRE(tr.levels < MAX_LEVELS, ST_ERR_INTERNAL, "neighbors: too many tree levels");
        tr.off[tr.levels] = (uint32_t)total;
        tr.cnt[tr.levels] = (uint32_t)cnt;
        total += cnt;
        ++tr.levels;
        if (cnt == 1) break;
        cnt = (cnt + 7) / 8;
    }
    ST_REQUIRE(total < (1ull << 32), ST_ERR_INTERNAL, "neighbors: too many tree nodes");
    T.nodes = total;
    T.box = wsT<double>(c, tag + ".nb.box", total * 6);
    T.f32 = cs.type[0] == ST_PLY_FLOAT && cs.type[1] == ST_PLY_FLOAT && cs.type[2] == ST_PLY_FLOAT;
    if (T.f32) gather_and_boxes<float4>(c, cs, tag, T);
    else gather_and_boxes<double4>(c, cs, tag, T);
}

}  // namespace nbt

void neighbors_require(const st_ttable *t, int32_t k, const char *what) {
    (void)xyz_cols(t, what);
    ST_REQUIRE(k_ok(k), ST_ERR_ARG, std::string(what) + ": k must be an integer in 1..32");
}

void outliers_require(const st_ttable *t, const st_action &act) {
    neighbors_require(t, act.neighbors, "filterOutliers");
    ST_REQUIRE(act.outlier_mode == ST_OUTLIER_SIGMA || act.outlier_mode == ST_OUTLIER_DISTANCE, ST_ERR_ARG,
               "filterOutliers: unknown outlier_mode");
    ST_REQUIRE(outlier_args_ok(act.outlier_mode, act.outlier_value), ST_ERR_ARG,
               act.outlier_mode == ST_OUTLIER_SIGMA ? "filterOutliers: sigma is NaN" : "filterOutliers: distance is NaN");
}

void neighbor_dist_tdev(st_ctx *c, const st_ttable *t, int32_t k, const std::string &tag, double *dist) {
    const NCols cs = xyz_cols(t, "neighbor_dist");
    ST_REQUIRE(k_ok(k), ST_ERR_ARG, "neighbor_dist: k must be an integer in 1..32");
    const uint64_t n = t->n;
    ST_REQUIRE(n < (1ull << 32), ST_ERR_UNSUPPORTED, "neighbor_dist: 2^32 rows or more");
    Stats S;
    S.rows = n;
    if (n == 0) {
        publish(c, S);
        return;
    }
    auto *d_cnt = wsT<Counters>(c, tag + ".nb.counters", 1);
    auto *h_cnt = static_cast<Counters *>(pinned_slot(c, "nb.host", sizeof(Counters)));
    ST_HIP(hipMemsetAsync(d_cnt, 0, sizeof(Counters), c->stream));
    {
        KTimer kt(c, "nb.fill");
        hipLaunchKernelGGL(k_nb_fill, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, dist, n);
        ST_LAUNCH_CHECK();
    }
    Built T;
    build_tree(c, cs, n, tag, T);
    S.placed = T.P;
    if (T.P) {
        if (T.f32) search<float4>(c, T, k, dist, d_cnt);
        else search<double4>(c, T, k, dist, d_cnt);
        ST_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
        ST_HIP(hipStreamSynchronize(c->stream));
        S.pairs = h_cnt->pairs, S.nodes = h_cnt->nodes;
        S.leaves = T.tr.cnt[0];
        S.levels = (uint64_t)T.tr.levels;
    }
    publish(c, S);
}

uint64_t filter_outliers_tdev(st_ctx *c, const st_ttable *t, const st_action &act, const std::string &tag,
                              uint32_t *out_idx) {
    outliers_require(t, act);
    const uint64_t n = t->n;
    if (n == 0) return 0;
    auto *dist = wsT<double>(c, tag + ".nb.dist", n);
    neighbor_dist_tdev(c, t, act.neighbors, tag, dist);
    double mean = 0, std_dev = 0;
    if (act.outlier_mode == ST_OUTLIER_SIGMA) {
        st_col_summary s;
        summary_f64_dev(c, dist, n, &s);
        mean = s.mean, std_dev = s.std_dev;
    }
    const double thr = threshold(act.outlier_mode, act.outlier_value, mean, std_dev);
    auto *flags = wsT<uint32_t>(c, tag + ".nb.flags", n);
    {
        KTimer kt(c, "nb.flags");
        hipLaunchKernelGGL(k_nb_flags, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, (const double *)dist, n, thr,
                           flags);
        ST_LAUNCH_CHECK();
    }
    return compact_flags_dev(c, flags, n, out_idx);
}

}  // namespace st

using namespace st;

extern "C" {

int st_dev_neighbor_dist(st_ctx *c, const st_ttable *t, int32_t k, double *dev_dist) {
    return guard([&] {
        ST_REQUIRE(c && t && (dev_dist || t->n == 0), ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(t->ncol >= 0 && (t->ncol == 0 || (t->names && t->types && t->cols)), ST_ERR_ARG, "neighbor_dist: bad table");
        ST_REQUIRE(t->n < (1ull << 32), ST_ERR_UNSUPPORTED, "neighbor_dist: 2^32 rows or more");
        for (int p = 0; p < t->ncol; ++p) {
            ST_REQUIRE(t->names[p], ST_ERR_ARG, "neighbor_dist: NULL column name");
            const int z = type_size(t->types[p]);
            ST_REQUIRE(z > 0, ST_ERR_ARG, std::string("neighbor_dist: column '") + t->names[p] + "' has a bad type");
            ST_REQUIRE(t->n == 0 || t->cols[p], ST_ERR_ARG, std::string("neighbor_dist: column '") + t->names[p] + "' is NULL");
            ST_REQUIRE(((uintptr_t)t->cols[p] & (uintptr_t)(z - 1)) == 0, ST_ERR_ARG,
                       std::string("neighbor_dist: column '") + t->names[p] + "' is not aligned to its type");
        }
        ST_REQUIRE(((uintptr_t)dev_dist & 7u) == 0, ST_ERR_ARG, "neighbor_dist: dev_dist is not aligned to 8 bytes");
        neighbors_require(t, k, "neighbor_dist");
        use_device(c);
        neighbor_dist_tdev(c, t, k, "nbr", dev_dist);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

const char *st_ctx_last_neighbor_stats(st_ctx *c) { return c ? c->last_neighbor_stats.c_str() : "{}"; }

}  // extern "C"
