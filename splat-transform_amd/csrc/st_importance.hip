// st_importance.hip -- include/st_abi.h's "importance, decimation and crops" on the device.  The
// rules are the functions of st_importance.h; this file reads the columns and selects rows.
//
//   k_im_score4 / k_im_score_t   one read of scale_0..2 and opacity -> the score (f64) and / or its
//                  key (u64).  Four float32 columns on 16-byte boundaries: 4 rows per thread from
//                  four float4 loads, the last n % 4 rows scalar; any other types or alignment: one
//                  row per thread through value_at
//   decimate       the key T of rank m - 1 by radix select over the keys, 8-bit digits from the top:
//   k_im_hist      a block's LDS histogram of the digit among the keys that match the prefix so far,
//                  merged into 256 global counters with integer atomics
//   k_im_pick      one thread walks the counters from digit 255 down, extends the prefix, lowers the
//                  rank and clears the counters.  Eight rounds queued back to back: the prefix and
//                  the rank live on the device, the host reads nothing
//   k_im_split     gt[i] = key > T, eq[i] = key == T; scan_u32 over eq ranks the ties by row index
//   k_im_take      gt[i] |= eq[i] && eqpos[i] < m - count(key > T), which the select left as rank + 1
//                  then compact_flags_dev.  Integer counts and compares only: the rows do not depend
//                  on the grid, the block size or the order the atomics arrive in
//   order          radix_sort_u64 of the inverted keys (ascending = most important first, stable =
//                  ties by row index) with iota_u32 values
//   k_im_box4 / k_im_sphere4 / k_im_crop_t   the crops' flags, wide and general as for the score
// Workspace slots carry the caller's tag (the chain's), so several chains can be alive at once.
#include <cstring>

#include "st_importance.h"
#include "st_internal.h"

namespace st {
namespace {

using namespace imp;
typedef unsigned long long ull;

struct ICols {  // kernel argument: up to four columns of any type
    const void *p[4];
    int32_t type[4];
};
struct SelState {
    ull prefix, rank;
};
struct Crop {  // box: a = min, b = max; sphere: a = centre, r = radius
    double a[3], b[3], r;
    int sphere;
};

__device__ inline void put(double *scores, ull *keys, uint64_t i, double v) {
    if (scores) scores[i] = v;
    if (keys) keys[i] = key_of_score(v);
}

__global__ __launch_bounds__(256) void k_im_score_t(const ICols cs, uint64_t n, double *__restrict__ scores,
                                                    ull *__restrict__ keys) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        put(scores, keys, i,
            score(value_at(cs.p[0], cs.type[0], i), value_at(cs.p[1], cs.type[1], i),
                  value_at(cs.p[2], cs.type[2], i), value_at(cs.p[3], cs.type[3], i)));
}

__global__ __launch_bounds__(256) void k_im_score4(const ICols cs, uint64_t n, double *__restrict__ scores,
                                                   ull *__restrict__ keys) {
    const uint64_t nq = n / 4;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
        const float4 a = reinterpret_cast<const float4 *>(cs.p[0])[q], b = reinterpret_cast<const float4 *>(cs.p[1])[q],
                     d = reinterpret_cast<const float4 *>(cs.p[2])[q], o = reinterpret_cast<const float4 *>(cs.p[3])[q];
        put(scores, keys, 4 * q + 0, score((double)a.x, (double)b.x, (double)d.x, (double)o.x));
        put(scores, keys, 4 * q + 1, score((double)a.y, (double)b.y, (double)d.y, (double)o.y));
        put(scores, keys, 4 * q + 2, score((double)a.z, (double)b.z, (double)d.z, (double)o.z));
        put(scores, keys, 4 * q + 3, score((double)a.w, (double)b.w, (double)d.w, (double)o.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < n % 4) {  // the last n % 4 rows
        const uint64_t i = nq * 4 + threadIdx.x;
        put(scores, keys, i,
            score((double)((const float *)cs.p[0])[i], (double)((const float *)cs.p[1])[i],
                  (double)((const float *)cs.p[2])[i], (double)((const float *)cs.p[3])[i]));
    }
}

// pass p looks at bits [56 - 8p, 64 - 8p) of the keys whose higher bits equal the prefix
__global__ __launch_bounds__(256) void k_im_hist(const ull *__restrict__ keys, uint64_t n,
                                                 const SelState *__restrict__ st, unsigned *__restrict__ hist, int pass) {
    __shared__ unsigned h[256];
    const int shift = 56 - 8 * pass;
    const ull prefix = st->prefix;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const ull k = keys[i];
        if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&h[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// the digit that holds descending rank `rank` among the prefix's keys; the counters are cleared
__global__ __launch_bounds__(256) void k_im_pick(SelState *st, unsigned *hist) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        ull rank = st->rank, above = 0;
        int d = 255;
        for (; d > 0; --d) {
            if (rank < above + h[d]) break;
            above += h[d];
        }
        st->rank = rank - above;
        st->prefix = (st->prefix << 8) | (ull)d;
    }
}

__global__ __launch_bounds__(256) void k_im_split(const ull *__restrict__ keys, uint64_t n,
                                                  const SelState *__restrict__ st, uint32_t *__restrict__ gt,
                                                  uint32_t *__restrict__ eq) {
    const ull T = st->prefix;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const ull k = keys[i];
        gt[i] = k > T ? 1u : 0u;
        eq[i] = k == T ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_im_take(const uint32_t *__restrict__ eq, const uint32_t *__restrict__ eqpos,
                                                 uint64_t n, const SelState *__restrict__ st,
                                                 uint32_t *__restrict__ flags) {
    const ull take = st->rank + 1;  // m - count(key > T)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (eq[i] && eqpos[i] < take) flags[i] = 1u;
}

__global__ __launch_bounds__(256) void k_im_invert(ull *keys, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) keys[i] = ~keys[i];
}

__device__ inline uint32_t crop_keep(const Crop &cr, double x, double y, double z) {
    return (cr.sphere ? in_sphere(x, y, z, cr.a, cr.r) : in_box(x, y, z, cr.a, cr.b)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_im_crop_t(const ICols cs, uint64_t n, const Crop cr,
                                                   uint32_t *__restrict__ flags) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        flags[i] = crop_keep(cr, value_at(cs.p[0], cs.type[0], i), value_at(cs.p[1], cs.type[1], i),
                             value_at(cs.p[2], cs.type[2], i));
}

template <int SPHERE>
__global__ __launch_bounds__(256) void k_im_crop4(const ICols cs, uint64_t n, const Crop cr,
                                                  uint32_t *__restrict__ flags) {
    const uint64_t nq = n / 4;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    Crop c = cr;
    c.sphere = SPHERE;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += stride) {
        const float4 x = reinterpret_cast<const float4 *>(cs.p[0])[q], y = reinterpret_cast<const float4 *>(cs.p[1])[q],
                     z = reinterpret_cast<const float4 *>(cs.p[2])[q];
        reinterpret_cast<uint4 *>(flags)[q] =
            make_uint4(crop_keep(c, (double)x.x, (double)y.x, (double)z.x), crop_keep(c, (double)x.y, (double)y.y, (double)z.y),
                       crop_keep(c, (double)x.z, (double)y.z, (double)z.z), crop_keep(c, (double)x.w, (double)y.w, (double)z.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < n % 4) {
        const uint64_t i = nq * 4 + threadIdx.x;
        flags[i] = crop_keep(c, (double)((const float *)cs.p[0])[i], (double)((const float *)cs.p[1])[i],
                             (double)((const float *)cs.p[2])[i]);
    }
}

const char *const SCORE_COLS[4] = {"scale_0", "scale_1", "scale_2", "opacity"};
const char *const XYZ_COLS[3] = {"x", "y", "z"};

// the named columns of t (the first of each name); false when one is missing
bool find_cols(const st_ttable *t, const char *const *names, int count, ICols &cs, const char **missing) {
    cs = ICols{};
    for (int k = 0; k < count; ++k) {
        int col = -1;
        for (int i = 0; i < t->ncol && col < 0; ++i)
            if (std::strcmp(t->names[i], names[k]) == 0) col = i;
        if (col < 0) {
            if (missing) *missing = names[k];
            return false;
        }
        ST_REQUIRE(type_size(t->types[col]) > 0, ST_ERR_ARG, std::string("column ") + names[k] + " has a bad type");
        cs.p[k] = t->cols[col];
        cs.type[k] = t->types[col];
    }
    return true;
}

bool wide_ok(const ICols &cs, int count) {
    for (int k = 0; k < count; ++k)
        if (cs.type[k] != ST_PLY_FLOAT || ((uintptr_t)cs.p[k] & 15u)) return false;
    return true;
}

ICols score_cols(const st_ttable *t, const char *what) {
    ICols cs;
    const char *missing = nullptr;
    if (!find_cols(t, SCORE_COLS, 4, cs, &missing))
        throw Error(ST_ERR_ARG, std::string(what) + ": the table has no column " + missing);
    return cs;
}

void launch_scores(st_ctx *c, const ICols &cs, uint64_t n, double *scores, ull *keys) {
    KTimer kt(c, "im.score");
    if (wide_ok(cs, 4))
        hipLaunchKernelGGL(k_im_score4, dim3(grid_for((n + 3) / 4, 256, 8192)), dim3(256), 0, c->stream, cs, n, scores, keys);
    else
        hipLaunchKernelGGL(k_im_score_t, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, cs, n, scores, keys);
    ST_LAUNCH_CHECK();
}

uint64_t crop_tdev(st_ctx *c, const st_ttable *t, const Crop &cr, const std::string &tag, uint32_t *out_idx) {
    const uint64_t n = t->n;
    ICols cs;
    if (n == 0 || !find_cols(t, XYZ_COLS, 3, cs, nullptr)) return 0;  // a missing column reads NaN: no row passes
    auto *flags = wsT<uint32_t>(c, tag + ".im.flags", n);
    {
        KTimer kt(c, cr.sphere ? "im.sphere" : "im.box");
        if (wide_ok(cs, 3)) {
            const dim3 g(grid_for((n + 3) / 4, 256, 8192));
            if (cr.sphere) hipLaunchKernelGGL(k_im_crop4<1>, g, dim3(256), 0, c->stream, cs, n, cr, flags);
            else hipLaunchKernelGGL(k_im_crop4<0>, g, dim3(256), 0, c->stream, cs, n, cr, flags);
        } else {
            hipLaunchKernelGGL(k_im_crop_t, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, cs, n, cr, flags);
        }
        ST_LAUNCH_CHECK();
    }
    return compact_flags_dev(c, flags, n, out_idx);
}

}  // namespace

void importance_require(const st_ttable *t, const char *what) { (void)score_cols(t, what); }

void importance_scores_tdev(st_ctx *c, const st_ttable *t, double *scores) {
    const ICols cs = score_cols(t, "importance");
    if (t->n) launch_scores(c, cs, t->n, scores, nullptr);
}

void importance_order_tdev(st_ctx *c, const st_ttable *t, const std::string &tag, uint32_t *out_idx) {
    const ICols cs = score_cols(t, "orderByImportance");
    const uint64_t n = t->n;
    if (n == 0) return;
    ST_REQUIRE(n < (1ull << 32), ST_ERR_UNSUPPORTED, "importance: 2^32 rows or more");
    auto *keys = wsT<ull>(c, tag + ".im.keys", n);
    launch_scores(c, cs, n, nullptr, keys);
    hipLaunchKernelGGL(k_im_invert, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, keys, n);
    ST_LAUNCH_CHECK();
    iota_u32(c, out_idx, n);
    KTimer kt(c, "im.sort");
    radix_sort_u64(c, reinterpret_cast<uint64_t *>(keys), out_idx, n, 0, 64, tag + ".im.sort");
}

// the rows of importance rank < m, ascending, 0 < m < n; returns m
uint64_t importance_top_tdev(st_ctx *c, const st_ttable *t, uint64_t m, const std::string &tag, uint32_t *out_idx) {
    const ICols cs = score_cols(t, "decimate");
    const uint64_t n = t->n;
    ST_REQUIRE(n < (1ull << 32), ST_ERR_UNSUPPORTED, "importance: 2^32 rows or more");
    ST_REQUIRE(m > 0 && m < n, ST_ERR_INTERNAL, "importance_top: m must be in (0, n)");
    auto *keys = wsT<ull>(c, tag + ".im.keys", n);
    auto *flags = wsT<uint32_t>(c, tag + ".im.flags", n);
    auto *eq = wsT<uint32_t>(c, tag + ".im.eq", n);
    auto *eqpos = wsT<uint32_t>(c, tag + ".im.eqpos", n + 1);
    auto *hist = wsT<unsigned>(c, tag + ".im.hist", 256);
    auto *st = wsT<SelState>(c, tag + ".im.state", 1);
    launch_scores(c, cs, n, nullptr, keys);
    const SelState s0{0, m - 1};
    auto *h0 = static_cast<SelState *>(pinned_slot(c, "im.state", sizeof(SelState)));
    *h0 = s0;
    ST_HIP(hipMemcpyAsync(st, h0, sizeof(SelState), hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemsetAsync(hist, 0, 256 * sizeof(unsigned), c->stream));
    const dim3 g(grid_for(n, 256 * 8, 2048));
    for (int pass = 0; pass < 8; ++pass) {
        {
            KTimer kt(c, "im.hist");
            hipLaunchKernelGGL(k_im_hist, g, dim3(256), 0, c->stream, (const ull *)keys, n, (const SelState *)st, hist, pass);
            ST_LAUNCH_CHECK();
        }
        KTimer kt(c, "im.pick");
        hipLaunchKernelGGL(k_im_pick, dim3(1), dim3(256), 0, c->stream, st, hist);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "im.flags");
        hipLaunchKernelGGL(k_im_split, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, (const ull *)keys, n,
                           (const SelState *)st, flags, eq);
        ST_LAUNCH_CHECK();
        scan_u32(c, eq, eqpos, n, nullptr);
        hipLaunchKernelGGL(k_im_take, dim3(grid_for(n, 256, 8192)), dim3(256), 0, c->stream, (const uint32_t *)eq,
                           (const uint32_t *)eqpos, n, (const SelState *)st, flags);
        ST_LAUNCH_CHECK();
    }
    const uint64_t got = compact_flags_dev(c, flags, n, out_idx);
    ST_REQUIRE(got == m, ST_ERR_INTERNAL, "decimate: the selection kept " + std::to_string(got) + " rows, not " + std::to_string(m));
    return got;
}

uint64_t filter_box_tdev(st_ctx *c, const st_ttable *t, const double lo[3], const double hi[3], const std::string &tag,
                         uint32_t *out_idx) {
    Crop cr{};
    for (int a = 0; a < 3; ++a) cr.a[a] = lo[a], cr.b[a] = hi[a];
    return crop_tdev(c, t, cr, tag, out_idx);
}

uint64_t filter_sphere_tdev(st_ctx *c, const st_ttable *t, const double centre[3], double radius, const std::string &tag,
                            uint32_t *out_idx) {
    Crop cr{};
    for (int a = 0; a < 3; ++a) cr.a[a] = centre[a];
    cr.r = radius;
    cr.sphere = 1;
    return crop_tdev(c, t, cr, tag, out_idx);
}

uint64_t decimate_rows_checked(const st_action &act, uint64_t n) {
    uint64_t m = 0;
    ST_REQUIRE(imp::decimate_rows(act.amount_mode, act.amount, n, &m), ST_ERR_ARG,
               act.amount_mode == ST_DECIMATE_COUNT
                   ? "decimate: count must be a non-negative integer below 2^53"
                   : act.amount_mode == ST_DECIMATE_FRACTION ? "decimate: fraction must be in [0, 1]"
                                                             : "decimate: unknown amount_mode");
    return m;
}

namespace {
void check_dev_table(const st_ttable *t) {
    ST_REQUIRE(t->ncol >= 0 && (t->ncol == 0 || (t->names && t->types && t->cols)), ST_ERR_ARG, "importance: bad table");
    ST_REQUIRE(t->n < (1ull << 32), ST_ERR_UNSUPPORTED, "importance: 2^32 rows or more");
    for (int p = 0; p < t->ncol; ++p) {
        ST_REQUIRE(t->names[p], ST_ERR_ARG, "importance: NULL column name");
        const int z = type_size(t->types[p]);
        ST_REQUIRE(z > 0, ST_ERR_ARG, std::string("importance: column '") + t->names[p] + "' has a bad type");
        ST_REQUIRE(t->n == 0 || t->cols[p], ST_ERR_ARG, std::string("importance: column '") + t->names[p] + "' is NULL");
        ST_REQUIRE(((uintptr_t)t->cols[p] & (uintptr_t)(z - 1)) == 0, ST_ERR_ARG,
                   std::string("importance: column '") + t->names[p] + "' is not aligned to its type");
    }
}
}  // namespace

}  // namespace st

using namespace st;

extern "C" {

int st_dev_importance(st_ctx *c, const st_ttable *t, double *dev_scores) {
    return guard([&] {
        ST_REQUIRE(c && t && (dev_scores || t->n == 0), ST_ERR_ARG, "NULL argument");
        check_dev_table(t);
        importance_require(t, "importance");
        use_device(c);
        importance_scores_tdev(c, t, dev_scores);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

int st_dev_importance_order(st_ctx *c, const st_ttable *t, uint32_t *dev_order) {
    return guard([&] {
        ST_REQUIRE(c && t && (dev_order || t->n == 0), ST_ERR_ARG, "NULL argument");
        check_dev_table(t);
        importance_require(t, "orderByImportance");
        use_device(c);
        importance_order_tdev(c, t, "imp", dev_order);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

int st_dev_importance_top(st_ctx *c, const st_ttable *t, uint64_t m, uint32_t *dev_rows, uint64_t *out_m) {
    return guard([&] {
        ST_REQUIRE(c && t && out_m, ST_ERR_ARG, "NULL argument");
        check_dev_table(t);
        importance_require(t, "decimate");
        const uint64_t k = std::min<uint64_t>(m, t->n);
        ST_REQUIRE(dev_rows || k == 0, ST_ERR_ARG, "NULL argument");
        use_device(c);
        if (k == t->n) iota_u32(c, dev_rows, k);  // every row
        else if (k) {  // compacted into a slot of n entries: the caller's buffer holds k
            auto *rows = wsT<uint32_t>(c, "imp.rows", t->n);
            importance_top_tdev(c, t, k, "imp", rows);
            ST_HIP(hipMemcpyAsync(dev_rows, rows, k * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        }
        ST_HIP(hipStreamSynchronize(c->stream));
        *out_m = k;
    });
}

}  // extern "C"
