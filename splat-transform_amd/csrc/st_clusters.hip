// st_clusters.hip -- include/st_abi.h's "clusters" on the device.  The rules are the functions of
// st_clusters.h; this file finds the connected components of the link graph without evaluating every
// pair, over the tree st_neighbors.hip builds (st_nbtree.h).
//
//   k_cl_init      parent[i] = i for a placed row, 0xFFFFFFFF otherwise, indexed by ORIGINAL row: hooks
//                  put the larger root under the smaller, so a finished tree's root is the smallest
//                  row index of its component -- the label
//   k_cl_cliques   clique[node] = far_bound(box, box) <= r2: every two rows of the node link.  A child's
//                  box lies inside its parent's and far_bound is monotone in the box, so the clique
//                  ancestors of a leaf are the first few of its path to the root
//   k_cl_hook      every sorted row climbs to its maximal clique node and is united with that node's
//                  first row: P unions in all, whatever the radius
//   k_cl_link      one wave (a workgroup of 64) per leaf, its members the 64 queries, a lane each; a
//                  depth-first walk from the root over a stack in LDS that every lane writes alike.
//                  A node is PRUNED when nbr::box_bound(node, q) > r2 in every lane (strict: the link
//                  test is <=).  In a clique node a lane with cl::far_bound(node, q) <= r2 links to all
//                  of its rows: one union with the node's first row and the lane is done with the
//                  node; the node is ABSORBED when no lane is left.  Otherwise the walk descends; at
//                  a leaf every lane that still wants it tests d2 <= r2 against the staged members.
//                  link is symmetric bit for bit, so a wave walks only the nodes that hold a leaf >=
//                  its own in sorted order, and in its own leaf a lane tests the members after it.
//   unite          lock-free: both roots, then one 32-bit atomicCAS on the LARGER root's own slot; on
//                  failure it goes on from the value the CAS returned.  find splits paths: it writes
//                  only ancestors.  parent[] is read and compressed with relaxed agent-scope atomics
//                  (a plain load of a line another CU rewrote may be served stale from L1); only the
//                  CAS decides a hook.  No fences: a stale ancestor is still an ancestor, and a failed
//                  CAS repairs a stale "is a root"
//   k_cl_flatten   its own launch after k_cl_link: label[i] = find(i) with plain loads, count[label]
//                  by integer atomicAdd (one per distinct label of a wave), the largest size by
//                  atomicMax of the running counts, the components by counting label[i] == i
//   k_cl_size      size[i] = count[label[i]]
//   k_cl_flags     keep iff cl::keep(mode, size, cluster_min, largest)
// All atomics are integer CAS, maxima and sums: no result depends on the order in which they arrive.
// Workspace slots carry the caller's tag.
#include <cstring>

#include "st_clusters.h"
#include "st_internal.h"
#include "st_nbtree.h"

namespace st {
namespace {

using namespace nbr;
using namespace nbt;
typedef unsigned long long ull;

struct Counters {  // device record of one call
    ull pairs, nodes, unions;
    uint32_t components, largest;
};

__device__ inline ull wave_sum(ull v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ inline uint32_t p_load(const uint32_t *parent, uint32_t i) {
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void p_store(uint32_t *parent, uint32_t i, uint32_t v) {
    __hip_atomic_store(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above placed row v.  Path splitting: a visited row is pointed at its grandparent, an
// ancestor, and only after it was seen not to be a root -- a row that stopped being a root never is
// one again, so such a store cannot undo a hook.  parent[v] <= v always: the walk ends
__device__ inline uint32_t find(uint32_t *parent, uint32_t v) {
    uint32_t p = p_load(parent, v);
    while (p != v) {
        const uint32_t g = p_load(parent, p);
        if (g != p) p_store(parent, v, g);
        v = p, p = g;
    }
    return v;
}

// joins the trees of placed rows a and b; returns their common root as it was then
__device__ inline uint32_t unite(uint32_t *parent, uint32_t a, uint32_t b, ull &unions) {
    for (;;) {
        a = find(parent, a), b = find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const uint32_t t = a;
            a = b, b = t;
        }
        const uint32_t old = atomicCAS(parent + a, a, b);  // a > b: the larger root under the smaller
        if (old == a) {
            ++unions;
            return b;
        }
        a = old;  // a was hooked by another lane meanwhile: old is its ancestor
    }
}

__global__ __launch_bounds__(256) void k_cl_init(const NCols cs, uint64_t n, uint32_t *__restrict__ parent) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        parent[i] = placed(value_at(cs.p[0], cs.type[0], i), value_at(cs.p[1], cs.type[1], i),
                           value_at(cs.p[2], cs.type[2], i))
                        ? (uint32_t)i
                        : cl::NONE;
}

// one thread per node of any level
__global__ __launch_bounds__(256) void k_cl_cliques(const double *__restrict__ box, uint64_t nodes, double r2,
                                                    uint8_t *__restrict__ clique) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nodes) return;
    const double *b = box + j * 6;
    const double lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
    clique[j] = cl::far_bound(lo, hi, lo, hi) <= r2 ? 1 : 0;
}

// the first sorted row under node `node` of level `level`: every node but the last of a level is full
__device__ inline uint64_t first_row(uint32_t node, uint32_t level, int L) {
    return ((uint64_t)node << (3 * level)) * (uint64_t)L;  // node < 2^30 / 8^level, L <= 64: below 2^36
}

// one thread per sorted row s < P
__global__ __launch_bounds__(256) void k_cl_hook(const uint32_t *__restrict__ order, uint64_t P, int L, const Tree tr,
                                                 const uint8_t *__restrict__ clique, uint32_t *parent,
                                                 Counters *__restrict__ counters) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    ull unions = 0;
    if (s < P) {
        uint32_t node = (uint32_t)(s / (uint64_t)L), level = 0;  // < tr.cnt[0]
        if (clique[node]) {
            while ((int)level + 1 < tr.levels && clique[tr.off[level + 1] + (node >> 3)]) node >>= 3, ++level;
            const uint64_t f = first_row(node, level, L);  // <= s
            if (f != s) unite(parent, order[s], order[f], unions);
        }
    }
    unions = wave_sum(unions);
    if ((threadIdx.x & 63) == 0 && unions) atomicAdd(&counters->unions, unions);
}

// A workgroup is one wave: __syncthreads() orders the wave's LDS traffic and costs no wait.  Every
// branch around one is taken by all lanes alike (the conditions are wave votes, kernel arguments or
// stack entries every lane wrote alike).
template <typename T4>
__global__ __launch_bounds__(64) void k_cl_link(const T4 *__restrict__ pos, const uint32_t *__restrict__ order, uint64_t P,
                                                int L, double r2, const double *__restrict__ box,
                                                const uint8_t *__restrict__ clique, const Tree tr, uint32_t *parent,
                                                Counters *__restrict__ counters) {
    __shared__ double sx[64], sy[64], sz[64];  // the staged candidate leaf
    __shared__ uint32_t srow[64], spar[64];    // its members' original rows and their parents when staged
    __shared__ uint32_t stack[STACK];
    __shared__ uint32_t stack_level[STACK];
    const int lane = threadIdx.x;
    const uint32_t leaf = blockIdx.x;  // < tr.cnt[0]
    const uint64_t q0 = (uint64_t)leaf * L;
    const int nq = (int)(P - q0 < (uint64_t)L ? P - q0 : (uint64_t)L);  // >= 1
    const bool active = lane < nq;
    double qx = 0, qy = 0, qz = 0;
    uint32_t me = 0;
    if (active) {
        const T4 p = pos[q0 + lane];
        qx = (double)p.x, qy = (double)p.y, qz = (double)p.z;
        me = order[q0 + lane];
    }
    const double q[3] = {qx, qy, qz};
    uint32_t root = me;  // an ancestor of `me` (or `me`): a hint that only saves work
    ull pairs = 0, nodes = 0, unions = 0;  // pairs, unions: this lane's; nodes: the wave's

    // the members of leaf c against the queries of the lanes that want it
    auto scan_leaf = [&](uint32_t c, bool wanted, bool is_clique) {
        const uint64_t s0 = (uint64_t)c * L;
        const int m = (int)(P - s0 < (uint64_t)L ? P - s0 : (uint64_t)L);
        __syncthreads();  // the previous leaf has been read
        if (lane < m) {
            const T4 p = pos[s0 + lane];
            sx[lane] = (double)p.x, sy[lane] = (double)p.y, sz[lane] = (double)p.z;
            const uint32_t r = order[s0 + lane];
            srow[lane] = r, spar[lane] = p_load(parent, r);
        }
        __syncthreads();
        if (wanted) {
            int j = c == leaf ? lane + 1 : 0;  // the pairs inside the own leaf once each
            for (; j < m; ++j) {
                ++pairs;
                if (!cl::link(d2(qx, qy, qz, sx[j], sy[j], sz[j]), r2)) continue;
                // a member that is the lane's root hint, or whose parent was, shares its tree already
                if (spar[j] != root && srow[j] != root) root = unite(parent, me, srow[j], unions);
                if (is_clique) break;  // k_cl_hook joined the leaf's rows: one of them is all of them
            }
        }
    };

    int sp = 0;
    stack[0] = 0, stack_level[0] = (uint32_t)(tr.levels - 1);
    sp = 1;
    while (sp > 0) {
        --sp;
        const uint32_t node = stack[sp], level = stack_level[sp];
        // the node's leaves are [node 8^level, (node + 1) 8^level): all before the wave's own, and the
        // waves of those leaves test the pairs
        if ((((uint64_t)node + 1) << (3 * level)) <= (uint64_t)leaf) continue;
        const uint64_t at = (uint64_t)tr.off[level] + node;
        const double *b = box + at * 6;
        const double nlo[3] = {b[0], b[1], b[2]}, nhi[3] = {b[3], b[4], b[5]};
        ++nodes;
        bool wanted = active && !(box_bound(nlo, nhi, q, q) > r2);
        if (__ballot(wanted) == 0) continue;  // bound > r2 in every lane
        const bool is_clique = clique[at] != 0;
        if (is_clique) {
            if (wanted && cl::far_bound(nlo, nhi, q, q) <= r2) {
                const uint32_t rep = order[first_row(node, level, L)];
                if (rep != me) root = unite(parent, me, rep, unions);
                wanted = false;
            }
            if (__ballot(wanted) == 0) continue;  // absorbed
        }
        if (level == 0) {
            scan_leaf(node, wanted, is_clique);
            continue;
        }
        // the children in descending order: the walk meets them in sorted order.  At most 8 pushed
        // for one popped: sp <= 7 * levels + 1 <= STACK
        const uint32_t cl_ = level - 1, ccnt = tr.cnt[cl_];
        const uint64_t c0 = (uint64_t)node * 8;
        const uint32_t nc = (uint32_t)(ccnt - c0 < 8 ? ccnt - c0 : 8);  // c0 < ccnt
        for (uint32_t c = nc; c-- > 0;) {
            stack[sp] = (uint32_t)c0 + c, stack_level[sp] = cl_;
            ++sp;
        }
    }
    pairs = wave_sum(pairs), unions = wave_sum(unions);
    if (lane == 0) {
        atomicAdd(&counters->pairs, pairs), atomicAdd(&counters->nodes, nodes);
        if (unions) atomicAdd(&counters->unions, unions);
    }
}

// one thread per row; a block is whole waves, and every lane of a wave runs the vote loop
__global__ __launch_bounds__(256) void k_cl_flatten(const uint32_t *__restrict__ parent, uint64_t n,
                                                    uint32_t *__restrict__ label, uint32_t *__restrict__ count,
                                                    Counters *__restrict__ counters) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t l = cl::NONE;
    if (i < n && parent[i] != cl::NONE) {
        l = (uint32_t)i;
        for (uint32_t p = parent[l]; p != l; p = parent[l]) l = p;
    }
    if (i < n) label[i] = l;
    const int lane = threadIdx.x & 63;
    uint32_t roots = 0;
    bool todo = l != cl::NONE;
    for (ull left = __ballot(todo); left; left = __ballot(todo)) {
        const uint32_t lead = __shfl(l, __ffsll((long long)left) - 1);
        const ull same = __ballot(todo && l == lead);
        if (todo && l == lead) {
            todo = false;
            if (lane == __ffsll((long long)same) - 1) {
                const uint32_t add = (uint32_t)__popcll(same);
                atomicMax(&counters->largest, atomicAdd(count + lead, add) + add);
            }
        }
    }
    roots = (uint32_t)__popcll(__ballot(l != cl::NONE && l == (uint32_t)i));
    if (lane == 0 && roots) atomicAdd(&counters->components, roots);
}

__global__ __launch_bounds__(256) void k_cl_size(const uint32_t *__restrict__ label, const uint32_t *__restrict__ count,
                                                 uint64_t n, uint32_t *__restrict__ size) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        size[i] = label[i] == cl::NONE ? 0u : count[label[i]];
}

__global__ __launch_bounds__(256) void k_cl_flags(const uint32_t *__restrict__ size, uint64_t n, int32_t mode,
                                                  double cluster_min, uint32_t largest,
                                                  uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flags[i] = cl::keep(mode, size[i], cluster_min, largest) ? 1u : 0u;
}

struct Stats {
    uint64_t rows = 0, placed = 0, components = 0, largest = 0, leaves = 0, levels = 0, pairs = 0, nodes = 0, unions = 0;
};
void publish(st_ctx *c, const Stats &s) {
    auto f = [](const char *k, uint64_t v) { return std::string("\"") + k + "\": " + std::to_string(v); };
    c->last_cluster_stats = "{" + f("rows", s.rows) + ", " + f("placed", s.placed) + ", " + f("components", s.components) +
                            ", " + f("largest", s.largest) + ", " + f("leaves", s.leaves) + ", " + f("levels", s.levels) +
                            ", " + f("pairs", s.pairs) + ", " + f("nodes", s.nodes) + ", " + f("unions", s.unions) + "}";
}

template <typename T4>
void launch_link(st_ctx *c, const Built &T, double r2, const uint8_t *clique, uint32_t *parent, Counters *d_cnt) {
    KTimer kt(c, "cl.link");
    hipLaunchKernelGGL(k_cl_link<T4>, dim3(T.tr.cnt[0]), dim3(64), 0, c->stream, (const T4 *)T.pos,
                       (const uint32_t *)T.order, T.P, T.L, r2, (const double *)T.box, clique, T.tr, parent, d_cnt);
    ST_LAUNCH_CHECK();
}

}  // namespace

void clusters_require(const st_ttable *t, double radius, const char *what) {
    (void)xyz_cols(t, what);
    ST_REQUIRE(cl::radius_ok(radius), ST_ERR_ARG, std::string(what) + ": radius must be a number >= 0");
}

void filter_clusters_require(const st_ttable *t, const st_action &act) {
    clusters_require(t, act.cluster_radius, "filterClusters");
    ST_REQUIRE(cl::mode_ok(act.cluster_mode), ST_ERR_ARG, "filterClusters: unknown cluster_mode");
    ST_REQUIRE(cl::args_ok(act.cluster_radius, act.cluster_mode, act.cluster_min), ST_ERR_ARG,
               "filterClusters: minSize must be a non-negative integer below 2^53");
}

// label and size (n each, either may be null) of every row; waits for the stream, publishes the
// statistics and returns the largest size
uint32_t clusters_tdev(st_ctx *c, const st_ttable *t, double radius, const std::string &tag, uint32_t *label,
                          uint32_t *size) {
    const NCols cs = xyz_cols(t, "clusters");
    ST_REQUIRE(cl::radius_ok(radius), ST_ERR_ARG, "clusters: radius must be a number >= 0");
    const uint64_t n = t->n;
    ST_REQUIRE(n < (1ull << 32), ST_ERR_UNSUPPORTED, "clusters: 2^32 rows or more");
    Stats S;
    S.rows = n;
    if (n == 0) {
        publish(c, S);
        return 0;
    }
    const double r2 = cl::r2_of(radius);
    auto *d_cnt = wsT<Counters>(c, tag + ".cl.counters", 1);
    ST_HIP(hipMemsetAsync(d_cnt, 0, sizeof(Counters), c->stream));
    auto *h_cnt = static_cast<Counters *>(pinned_slot(c, "cl.host", sizeof(Counters)));
    auto *parent = wsT<uint32_t>(c, tag + ".cl.parent", n);
    auto *count = wsT<uint32_t>(c, tag + ".cl.count", n);
    if (!label) label = wsT<uint32_t>(c, tag + ".cl.label", n);
    ST_HIP(hipMemsetAsync(count, 0, n * sizeof(uint32_t), c->stream));
    {
        KTimer kt(c, "cl.init");
        hipLaunchKernelGGL(k_cl_init, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, cs, n, parent);
        ST_LAUNCH_CHECK();
    }
    Built T;
    build_tree(c, cs, n, tag, T);
    S.placed = T.P;
    if (T.P) {
        auto *clique = wsT<uint8_t>(c, tag + ".cl.clique", T.nodes);
        {
            KTimer kt(c, "cl.cliques");
            hipLaunchKernelGGL(k_cl_cliques, dim3(grid_for(T.nodes, 256)), dim3(256), 0, c->stream, (const double *)T.box,
                               T.nodes, r2, clique);
            ST_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_cl_hook, dim3(grid_for(T.P, 256)), dim3(256), 0, c->stream, (const uint32_t *)T.order, T.P,
                               T.L, T.tr, (const uint8_t *)clique, parent, d_cnt);
            ST_LAUNCH_CHECK();
        }
        if (T.f32) launch_link<float4>(c, T, r2, clique, parent, d_cnt);
        else launch_link<double4>(c, T, r2, clique, parent, d_cnt);
        S.leaves = T.tr.cnt[0];
        S.levels = (uint64_t)T.tr.levels;
    }
    {
        KTimer kt(c, "cl.flatten");
        hipLaunchKernelGGL(k_cl_flatten, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const uint32_t *)parent, n, label,
                           count, d_cnt);
        ST_LAUNCH_CHECK();
    }
    if (size) {
        KTimer kt(c, "cl.size");
        hipLaunchKernelGGL(k_cl_size, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, (const uint32_t *)label,
                           (const uint32_t *)count, n, size);
        ST_LAUNCH_CHECK();
    }
    ST_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    S.pairs = h_cnt->pairs, S.nodes = h_cnt->nodes, S.unions = h_cnt->unions;
    S.components = h_cnt->components, S.largest = h_cnt->largest;
    publish(c, S);
    return h_cnt->largest;
}

uint64_t filter_clusters_tdev(st_ctx *c, const st_ttable *t, const st_action &act, const std::string &tag,
                              uint32_t *out_idx) {
    filter_clusters_require(t, act);
    const uint64_t n = t->n;
    if (n == 0) return 0;
    auto *size = wsT<uint32_t>(c, tag + ".cl.size", n);
    const uint32_t largest = clusters_tdev(c, t, act.cluster_radius, tag, nullptr, size);
    auto *flags = wsT<uint32_t>(c, tag + ".cl.flags", n);
    {
        KTimer kt(c, "cl.flags");
        hipLaunchKernelGGL(k_cl_flags, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, (const uint32_t *)size, n,
                           act.cluster_mode, act.cluster_min, largest, flags);
        ST_LAUNCH_CHECK();
    }
    return compact_flags_dev(c, flags, n, out_idx);
}

}  // namespace st

using namespace st;

extern "C" {

int st_dev_clusters(st_ctx *c, const st_ttable *t, double radius, uint32_t *dev_label, uint32_t *dev_size) {
    return guard([&] {
        ST_REQUIRE(c && t, ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(t->ncol >= 0 && (t->ncol == 0 || (t->names && t->types && t->cols)), ST_ERR_ARG, "clusters: bad table");
        ST_REQUIRE(t->n < (1ull << 32), ST_ERR_UNSUPPORTED, "clusters: 2^32 rows or more");
        for (int p = 0; p < t->ncol; ++p) {
            ST_REQUIRE(t->names[p], ST_ERR_ARG, "clusters: NULL column name");
            const int z = type_size(t->types[p]);
            ST_REQUIRE(z > 0, ST_ERR_ARG, std::string("clusters: column '") + t->names[p] + "' has a bad type");
            ST_REQUIRE(t->n == 0 || t->cols[p], ST_ERR_ARG, std::string("clusters: column '") + t->names[p] + "' is NULL");
            ST_REQUIRE(((uintptr_t)t->cols[p] & (uintptr_t)(z - 1)) == 0, ST_ERR_ARG,
                       std::string("clusters: column '") + t->names[p] + "' is not aligned to its type");
        }
        ST_REQUIRE(((uintptr_t)dev_label & 3u) == 0 && ((uintptr_t)dev_size & 3u) == 0, ST_ERR_ARG,
                   "clusters: an output is not aligned to 4 bytes");
        clusters_require(t, radius, "clusters");
        use_device(c);
        (void)clusters_tdev(c, t, radius, "clu", dev_label, dev_size);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

const char *st_ctx_last_cluster_stats(st_ctx *c) { return c ? c->last_cluster_stats.c_str() : "{}"; }

}  // extern "C"
