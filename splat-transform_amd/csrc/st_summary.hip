// st_summary.hip -- the column summary (include/st_abi.h, "column summary") on the device: typed
// columns read in place, a few reads of each, nothing but a fixed record per column in scratch.
//
// Columns go through in batches of SM_BATCH with the column on gridDim.y; a block grid-strides one
// column with 16-byte loads (scan_col: scalar head and tail around the aligned body).  Per batch:
//   k_sm_classify  NaN / infinity counts, min / max as order-preserving keys, the lowest and the
//                  highest set bit's exponent over the finite non-zero elements
//   k_sm_sum       the exact sum.  Fast path (st_summary.h: fast_ok): a lane sums its elements as
//                  integers in units of 2^e_lo in an __int128, a wave adds them up, one 128-bit
//                  atomic add (two 64-bit ones and the carry) per wave.  General path: the binned
//                  superaccumulator, 16 copies per wave in LDS (64-bit LDS atomics), normalised by carry
//                  propagation every `flush` additions, merged limb-wise into the column's limbs
//                  with 64-bit global atomics after a last normalisation (each wave then adds less
//                  than 2^32 per limb, and there are fewer than 2^31 waves).  Integer addition is
//                  associative: the merged limbs are the same bits whatever order the adds arrive in
//   k_sm_hist /    radix select of the median on the keys, 8-bit digits from the top: a histogram
//   k_sm_pick      of the finite elements that match the prefix so far -- two prefixes, for ranks
//                  (m - 1) / 2 and m / 2, one histogram while they agree -- then one thread per
//                  column picks the digits.  key_bits / 8 rounds, no host round trip between them
//   k_sm_sum       again over t_i = (v_i - mean)^2 once the host has rounded the sum and divided
// The host rounds the limbs (acc_round) and does the scalar epilogue: the same functions as the
// serial form, so the last roundings never depend on a device's division or square root.
#include <cstdlib>
#include <cstring>

#include "st_internal.h"
#include "st_summary.h"

namespace st {
namespace {

using namespace sm;
typedef unsigned long long ull;

constexpr int SM_BATCH = 128;          // columns per launch
// superaccumulators per wave: lane l adds into copy l % 16, so the 64 lanes of a column whose
// elements share a binade collide four to an address instead of sixty-four.  A copy is 140 dwords
// long: the same limb of the 16 copies lies in 16 different bank pairs
constexpr int SM_COPIES = 16;
constexpr uint64_t SM_HOST_BATCH_BYTES = 1ull << 30;  // st_summary uploads about this much at a time

struct SmCol {
    const void *ptr;
    int32_t type, pad;
};
struct SmRec {
    ull nan, inf, kmin, kmax;
    int e_lo, e_hi;
    unsigned tinf, pad;
    ull fast_lo, fast_hi;  // the fast path's int128 total, units of 2^e_lo
    ull pref[2], rank[2];  // radix select: key prefix and remaining rank of the two order statistics
    ull norms;             // normalisations inside a loop (the flush interval was crossed)
};

template <int Z>
__device__ inline uint64_t load_z(const void *p, uint64_t i) {
    if (Z == 1) return ((const uint8_t *)p)[i];
    if (Z == 2) return ((const uint16_t *)p)[i];
    if (Z == 4) return ((const uint32_t *)p)[i];
    return ((const uint64_t *)p)[i];
}

// f(bits) for every element of the column that this block's share of a grid-stride over
// gridDim.x holds; tick(count) is called by whole waves, converged, after every step in which a
// lane passed at most `count` elements to f
template <int Z, typename F, typename T>
__device__ inline void scan_col(const void *p, uint64_t n, F &&f, T &&tick) {
    constexpr int PER = 16 / Z;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, G = (uint64_t)gridDim.x * blockDim.x;
    uint64_t head = ((16 - ((uintptr_t)p & 15)) & 15) / Z;
    if (head > n) head = n;
    const uint64_t nv = (n - head) / PER, tail0 = head + nv * PER;
    if (blockIdx.x == 0) {  // fewer than 16 elements at either end
        if (tid < head) f(load_z<Z>(p, tid));
        if (tid < n - tail0) f(load_z<Z>(p, tail0 + tid));
        tick(2);
    }
    const uint4 *v = (const uint4 *)((const char *)p + head * Z);
    const uint64_t lane = threadIdx.x & 63;
    for (uint64_t base = tid - lane; base < nv; base += G) {  // wave-uniform trip count
        const uint64_t i = base + lane;
        if (i < nv) {
            const uint4 q = v[i];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            if (Z == 8) {
                f((uint64_t)w[0] | ((uint64_t)w[1] << 32));
                f((uint64_t)w[2] | ((uint64_t)w[3] << 32));
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if (Z == 4) f(w[a]);
                    if (Z == 2) f(w[a] & 0xffffu), f(w[a] >> 16);
                    if (Z == 1) f(w[a] & 0xffu), f((w[a] >> 8) & 0xffu), f((w[a] >> 16) & 0xffu), f(w[a] >> 24);
                }
            }
        }
        tick(PER);
    }
}
template <typename F, typename T>
__device__ inline void scan_typed(const SmCol &col, uint64_t n, F &&f, T &&tick) {
    switch (elem_size(col.type)) {
        case 1: scan_col<1>(col.ptr, n, f, tick); break;
        case 2: scan_col<2>(col.ptr, n, f, tick); break;
        case 4: scan_col<4>(col.ptr, n, f, tick); break;
        default: scan_col<8>(col.ptr, n, f, tick); break;
    }
}

__device__ inline ull shfl_xor64(ull v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((ull)hi << 32) | lo;
}

__global__ void k_sm_init(SmRec *rec, int ncol) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncol) return;
    SmRec r{};
    r.kmin = ~0ull;
    r.e_lo = E_NONE_LO;
    r.e_hi = E_NONE_HI;
    rec[i] = r;
}

__global__ __launch_bounds__(256) void k_sm_classify(const SmCol *__restrict__ cols, uint64_t n, SmRec *__restrict__ rec) {
    const SmCol col = cols[blockIdx.y];
    const int32_t type = col.type;
    ull nan = 0, inf = 0, kmin = ~0ull, kmax = 0;
    int lo = E_NONE_LO, hi = E_NONE_HI;
    scan_typed(
        col, n,
        [&](uint64_t b) {
            const int c = classify(type, b);
            if (c) {
                nan += c == 1;
                inf += c == 2;
                return;
            }
            const ull k = key_of(type, b);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            const double v = widen(type, b);
            if (v != 0) {
                int l, h;
                bit_span(v, &l, &h);
                lo = l < lo ? l : lo;
                hi = h > hi ? h : hi;
            }
        },
        [](int) {});
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        nan += shfl_xor64(nan, o);
        inf += shfl_xor64(inf, o);
        const ull a = shfl_xor64(kmin, o), b = shfl_xor64(kmax, o);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
        const int l = __shfl_xor(lo, o, 64), h = __shfl_xor(hi, o, 64);
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        SmRec *r = rec + blockIdx.y;
        if (nan) atomicAdd(&r->nan, nan);
        if (inf) atomicAdd(&r->inf, inf);
        if (kmin != ~0ull) atomicMin(&r->kmin, kmin);
        if (kmax) atomicMax(&r->kmax, kmax);
        if (lo != E_NONE_LO) atomicMin(&r->e_lo, lo);
        if (hi != E_NONE_HI) atomicMax(&r->e_hi, hi);
    }
}

// which 0: the sum of the finite elements (limbs[col][0], or the record's int128 on the fast path);
// which 1: the sum of t_i = (v_i - mean)^2 (limbs[col][1], always the superaccumulator)
__global__ __launch_bounds__(256) void k_sm_sum(const SmCol *__restrict__ cols, uint64_t n, SmRec *__restrict__ rec,
                                                ull *__restrict__ limbs, int which,
                                                const double *__restrict__ means, int exact, uint64_t flush) {
    __shared__ ull acc[4][SM_COPIES][NL];
    const SmCol col = cols[blockIdx.y];
    const int32_t type = col.type;
    SmRec *r = rec + blockIdx.y;
    const uint64_t m = n - r->nan - r->inf;
    if (m == 0) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (which == 0 && !exact && fast_ok(r->e_lo, r->e_hi, m)) {
        const int e_lo = r->e_lo;
        __int128 s = 0;
        scan_typed(
            col, n,
            [&](uint64_t b) {
                if (classify(type, b) == 0) s += units_of(widen(type, b), e_lo);
            },
            [](int) {});
        ull lo = (ull)(unsigned __int128)s, hi = (ull)((unsigned __int128)s >> 64);
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const unsigned __int128 a = ((unsigned __int128)hi << 64) | lo;
            const unsigned __int128 b = ((unsigned __int128)shfl_xor64(hi, o) << 64) | shfl_xor64(lo, o);
            const unsigned __int128 t = a + b;
            lo = (ull)t;
            hi = (ull)(t >> 64);
        }
        if (lane == 0 && (lo | hi)) {
            // a 128-bit add as two 64-bit ones: the carries out of the low word add up to the same
            // count in any order
            const ull old = atomicAdd(&r->fast_lo, lo);
            const ull carry = (ull)(old + lo < old);
            if (hi + carry) atomicAdd(&r->fast_hi, hi + carry);
        }
        return;
    }
    for (int j = lane; j < SM_COPIES * NL; j += 64) (&acc[w][0][0])[j] = 0;
    ull *mine = acc[w][lane & (SM_COPIES - 1)];
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    const double mean = which ? means[blockIdx.y] : 0.0;
    bool tinf = false;
    uint64_t adds = 0;
    ull norms = 0;
    scan_typed(
        col, n,
        [&](uint64_t b) {
            if (classify(type, b)) return;
            double v = widen(type, b);
            if (which) {
                const double d = v - mean;
                v = d * d;
                if (v == __builtin_inf()) {
                    tinf = true;
                    return;
                }
            }
            if (v == 0) return;
            int j;
            int64_t c[3];
            acc_chunks(v, &j, c);
            if (c[0]) atomicAdd(&mine[j], (ull)c[0]);
            if (c[1]) atomicAdd(&mine[j + 1], (ull)c[1]);
            if (c[2]) atomicAdd(&mine[j + 2], (ull)c[2]);
        },
        [&](int count) {
            adds += 64ull * count;
            if (adds >= flush) {
                __threadfence_block();
                __builtin_amdgcn_wave_barrier();
                if (lane < SM_COPIES) acc_normalise((int64_t *)acc[w][lane]);
                norms += lane == 0;
                __threadfence_block();
                __builtin_amdgcn_wave_barrier();
                adds = 0;
            }
        });
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // the copies fold limb-wise into the first (their additions together stay within the interval's
    // headroom), which is normalised and merged
    for (int j = lane; j < NL; j += 64) {
        ull s = 0;
        for (int k = 0; k < SM_COPIES; ++k) s += acc[w][k][j];
        acc[w][0][j] = s;
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) acc_normalise((int64_t *)acc[w][0]);
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    ull *g = limbs + ((uint64_t)blockIdx.y * 2 + which) * NL;
    for (int j = lane; j < NL; j += 64)
        if (acc[w][0][j]) atomicAdd(&g[j], acc[w][0][j]);
    if (tinf) atomicOr(&r->tinf, 1u);
    if (norms) atomicAdd(&r->norms, norms);
}

__global__ __launch_bounds__(256) void k_sm_hist(const SmCol *__restrict__ cols, uint64_t n,
                                                 const SmRec *__restrict__ rec, ull *__restrict__ hist, int pass) {
    __shared__ unsigned h[2][256];
    const SmCol col = cols[blockIdx.y];
    const int32_t type = col.type;
    const int W = key_bits(type);
    if (pass * 8 >= W) return;
    const int shift = W - 8 * (pass + 1);
    const ull pa = rec[blockIdx.y].pref[0], pb = rec[blockIdx.y].pref[1];
    const bool two = pa != pb;
    h[0][threadIdx.x] = 0;
    h[1][threadIdx.x] = 0;
    __syncthreads();
    scan_typed(
        col, n,
        [&](uint64_t b) {
            if (classify(type, b)) return;
            const ull k = key_of(type, b);
            const ull top = pass ? k >> (shift + 8) : 0;
            const unsigned d = (unsigned)(k >> shift) & 255u;
            if (top == pa) atomicAdd(&h[0][d], 1u);
            if (two && top == pb) atomicAdd(&h[1][d], 1u);
        },
        [](int) {});
    __syncthreads();
    ull *g = hist + (uint64_t)blockIdx.y * 512;
    if (h[0][threadIdx.x]) atomicAdd(&g[threadIdx.x], (ull)h[0][threadIdx.x]);
    if (h[1][threadIdx.x]) atomicAdd(&g[256 + threadIdx.x], (ull)h[1][threadIdx.x]);
}

// one block per column: the next digit of both order statistics, then the histograms are cleared
__global__ __launch_bounds__(64) void k_sm_pick(const SmCol *__restrict__ cols, uint64_t n, SmRec *__restrict__ rec,
                                                ull *__restrict__ hist, int pass) {
    SmRec *r = rec + blockIdx.x;
    ull *g = hist + (uint64_t)blockIdx.x * 512;
    const uint64_t m = n - r->nan - r->inf;
    if (pass * 8 >= key_bits(cols[blockIdx.x].type) || m == 0) return;
    if (threadIdx.x == 0) {
        ull pref[2] = {r->pref[0], r->pref[1]}, rank[2] = {r->rank[0], r->rank[1]};
        if (pass == 0) rank[0] = (m - 1) / 2, rank[1] = m / 2;
        const bool two = pref[0] != pref[1];
        for (int q = 0; q < 2; ++q) {
            const ull *h = g + (q && two ? 256 : 0);
            ull cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                if (rank[q] < cum + h[d]) break;
                cum += h[d];
            }
            rank[q] -= cum;
            pref[q] = (pref[q] << 8) | (ull)d;
        }
        r->pref[0] = pref[0], r->pref[1] = pref[1];
        r->rank[0] = rank[0], r->rank[1] = rank[1];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 64) g[i] = 0;
}

struct Paths {
    uint64_t columns = 0, fast = 0, general = 0, norms = 0, flush = 0;
    bool exact = false;
};

void read_switches(Paths &P) {  // read per call (tests set them around one call)
    const char *e = getenv("ST_SUM_EXACT");
    P.exact = e && *e && std::strcmp(e, "0") != 0;
    P.flush = FLUSH_DEFAULT;
    if (const char *f = getenv("ST_SUM_FLUSH")) {
        const uint64_t v = std::strtoull(f, nullptr, 10);
        ST_REQUIRE(v >= 1 && v <= FLUSH_MAX, ST_ERR_ARG, "ST_SUM_FLUSH must be 1 .. 2^30");
        P.flush = v;
    }
}

void publish(st_ctx *c, const Paths &P) {
    c->last_summary_stats = "{\"columns\": " + std::to_string(P.columns) + ", \"fast\": " + std::to_string(P.fast) +
                            ", \"general\": " + std::to_string(P.general) + ", \"normalisations\": " +
                            std::to_string(P.norms) + ", \"flush\": " + std::to_string(P.flush) + "}";
}

// up to SM_BATCH device columns of n rows
void summarize_batch(st_ctx *c, const std::vector<SmCol> &cs, uint64_t n, st_col_summary *out, Paths &P) {
    const int nc = (int)cs.size();
    auto *d_cols = wsT<SmCol>(c, "sm.cols", SM_BATCH);
    auto *d_rec = wsT<SmRec>(c, "sm.rec", SM_BATCH);
    auto *d_limbs = wsT<ull>(c, "sm.limbs", (size_t)SM_BATCH * 2 * NL);
    auto *d_hist = wsT<ull>(c, "sm.hist", (size_t)SM_BATCH * 512);
    auto *d_mean = wsT<double>(c, "sm.mean", SM_BATCH);
    const size_t host_bytes = SM_BATCH * (sizeof(SmRec) + 2 * NL * 8 + 8);
    char *hp = static_cast<char *>(pinned_slot(c, "sm.host", host_bytes));
    auto *h_rec = reinterpret_cast<SmRec *>(hp);
    auto *h_limbs = reinterpret_cast<int64_t *>(hp + SM_BATCH * sizeof(SmRec));
    auto *h_mean = reinterpret_cast<double *>(hp + SM_BATCH * (sizeof(SmRec) + 2 * NL * 8));
    ST_HIP(hipMemcpyAsync(d_cols, cs.data(), sizeof(SmCol) * nc, hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemsetAsync(d_limbs, 0, (size_t)nc * 2 * NL * 8, c->stream));
    ST_HIP(hipMemsetAsync(d_hist, 0, (size_t)nc * 512 * 8, c->stream));
    hipLaunchKernelGGL(k_sm_init, dim3(1), dim3(SM_BATCH), 0, c->stream, d_rec, nc);
    ST_LAUNCH_CHECK();
    // about 2,048 rows a block, 4,096 blocks a launch at the most
    const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 2047) / 2048, std::max(8, 4096 / nc)));
    const dim3 grid(gx, (unsigned)nc);
    int passes = 0;
    for (const SmCol &s : cs) passes = std::max(passes, key_bits(s.type) / 8);
    if (n) {
        {
            KTimer kt(c, "sm.classify");
            hipLaunchKernelGGL(k_sm_classify, grid, dim3(256), 0, c->stream, (const SmCol *)d_cols, n, d_rec);
            ST_LAUNCH_CHECK();
        }
        {
            KTimer kt(c, "sm.sum");
            hipLaunchKernelGGL(k_sm_sum, grid, dim3(256), 0, c->stream, (const SmCol *)d_cols, n, d_rec, d_limbs, 0,
                               (const double *)d_mean, P.exact ? 1 : 0, P.flush);
            ST_LAUNCH_CHECK();
        }
        for (int pass = 0; pass < passes; ++pass) {
            {
                KTimer kt(c, "sm.hist");
                hipLaunchKernelGGL(k_sm_hist, grid, dim3(256), 0, c->stream, (const SmCol *)d_cols, n,
                                   (const SmRec *)d_rec, d_hist, pass);
                ST_LAUNCH_CHECK();
            }
            KTimer kt(c, "sm.pick");
            hipLaunchKernelGGL(k_sm_pick, dim3((unsigned)nc), dim3(64), 0, c->stream, (const SmCol *)d_cols, n, d_rec,
                               d_hist, pass);
            ST_LAUNCH_CHECK();
        }
    }
    ST_HIP(hipMemcpyAsync(h_rec, d_rec, sizeof(SmRec) * nc, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipMemcpyAsync(h_limbs, d_limbs, (size_t)nc * 2 * NL * 8, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    std::vector<uint64_t> ms(nc), norms0(nc);
    bool any = false;
    for (int p = 0; p < nc; ++p) {
        const SmRec &r = h_rec[p];
        const Gathered g{n, r.nan, r.inf, r.kmin, r.kmax, {r.pref[0], r.pref[1]}};
        finish_counts(cs[p].type, g, &out[p]);
        const uint64_t m = ms[p] = n - r.nan - r.inf;
        h_mean[p] = 0;
        const bool fast = !P.exact && fast_ok(r.e_lo, r.e_hi, m);
        ++P.columns;
        ++(fast ? P.fast : P.general);
        P.norms += norms0[p] = r.norms;
        if (!m) continue;
        any = true;
        int64_t *limbs = h_limbs + (size_t)p * 2 * NL;
        if (fast) {
            const __int128 V = (__int128)(((unsigned __int128)r.fast_hi << 64) | r.fast_lo);
            acc_add_i128(limbs, V, r.e_lo);
        }
        out[p].sum = acc_round(limbs);
        out[p].mean = h_mean[p] = mean_of(out[p].sum, m);
    }
    if (!any) return;
    ST_HIP(hipMemcpyAsync(d_mean, h_mean, sizeof(double) * nc, hipMemcpyHostToDevice, c->stream));
    {
        KTimer kt(c, "sm.dev");
        hipLaunchKernelGGL(k_sm_sum, grid, dim3(256), 0, c->stream, (const SmCol *)d_cols, n, d_rec, d_limbs, 1,
                           (const double *)d_mean, 1, P.flush);
        ST_LAUNCH_CHECK();
    }
    ST_HIP(hipMemcpyAsync(h_rec, d_rec, sizeof(SmRec) * nc, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipMemcpyAsync(h_limbs, d_limbs, (size_t)nc * 2 * NL * 8, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    for (int p = 0; p < nc; ++p) {
        if (!ms[p]) continue;
        P.norms += h_rec[p].norms - norms0[p];
        const double ssd = h_rec[p].tinf ? f64_of_bits(0x7ff0000000000000ull) : acc_round(h_limbs + ((size_t)p * 2 + 1) * NL);
        finish_ssd(ssd, ms[p], &out[p]);
    }
}

void check_table(const st_ttable *t) {
    ST_REQUIRE(t->ncol > 0 && t->names && t->types && t->cols, ST_ERR_ARG, "summary: a table needs at least one column");
    ST_REQUIRE(t->n < (1ull << 53), ST_ERR_UNSUPPORTED, "summary: 2^53 rows or more");
    for (int p = 0; p < t->ncol; ++p) {
        ST_REQUIRE(t->names[p], ST_ERR_ARG, "summary: NULL column name");
        const std::string name = t->names[p];
        const int z = elem_size(t->types[p]);
        ST_REQUIRE(z > 0, ST_ERR_ARG, "summary: column '" + name + "' has a bad type");
        ST_REQUIRE(t->n == 0 || t->cols[p], ST_ERR_ARG, "summary: column '" + name + "' is NULL");
        ST_REQUIRE(((uintptr_t)t->cols[p] & (uintptr_t)(z - 1)) == 0, ST_ERR_ARG,
                   "summary: column '" + name + "' is not aligned to its type");
    }
}

}  // namespace

void summary_dev(st_ctx *c, const st_ttable *t, st_col_summary *out) {
    check_table(t);
    Paths P;
    read_switches(P);
    for (int p0 = 0; p0 < t->ncol; p0 += SM_BATCH) {
        std::vector<SmCol> cs;
        for (int p = p0; p < std::min(t->ncol, p0 + SM_BATCH); ++p) cs.push_back(SmCol{t->cols[p], t->types[p], 0});
        summarize_batch(c, cs, t->n, out + p0, P);
    }
    publish(c, P);
}

void summary_f64_dev(st_ctx *c, const double *col, uint64_t n, st_col_summary *out) {
    ST_REQUIRE(((uintptr_t)col & 7u) == 0, ST_ERR_INTERNAL, "summary_f64_dev: misaligned column");
    Paths P;
    read_switches(P);
    summarize_batch(c, {SmCol{col, ST_PLY_DOUBLE, 0}}, n, out, P);
}

void summary_host(st_ctx *c, const st_ttable *t, st_col_summary *out) {
    check_table(t);
    Paths P;
    read_switches(P);
    int p0 = 0;
    while (p0 < t->ncol) {
        std::vector<SmCol> cs;
        std::vector<HostXfer> up;
        uint64_t bytes = 0;
        int p = p0;
        for (; p < t->ncol && p - p0 < SM_BATCH && (p == p0 || bytes < SM_HOST_BATCH_BYTES); ++p) {
            const uint64_t b = t->n * (uint64_t)elem_size(t->types[p]);
            void *d = ws_upload(c, "sm.in." + std::to_string(p - p0), t->cols[p], b, up);
            cs.push_back(SmCol{d, t->types[p], 0});
            bytes += b;
        }
        if (t->n) staged_h2d(c, up);
        summarize_batch(c, cs, t->n, out + p0, P);
        p0 = p;
    }
    publish(c, P);
}

}  // namespace st

using namespace st;

extern "C" {

int st_dev_summary(st_ctx *c, const st_ttable *t, st_col_summary *out) {
    return guard([&] {
        ST_REQUIRE(c && t && out, ST_ERR_ARG, "NULL argument");
        use_device(c);
        summary_dev(c, t, out);
    });
}

int st_summary(st_ctx *c, const st_ttable *t, st_col_summary *out) {
    return guard([&] {
        ST_REQUIRE(c && t && out, ST_ERR_ARG, "NULL argument");
        use_device(c);
        summary_host(c, t, out);
    });
}

int st_summary_text(const st_ttable *t, const st_col_summary *s, char **out, uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(t && s && out && size, ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(t->ncol > 0 && t->names, ST_ERR_ARG, "summary: a table needs at least one column");
        for (int p = 0; p < t->ncol; ++p) ST_REQUIRE(t->names[p], ST_ERR_ARG, "summary: NULL column name");
        const std::string text = sm::summary_text(t, s, numfmt_host_table());
        char *p = static_cast<char *>(std::malloc(text.size() + 1));
        ST_REQUIRE(p, ST_ERR_NOMEM, "summary text: allocation failed");
        std::memcpy(p, text.c_str(), text.size() + 1);
        *out = p;
        *size = text.size();
    });
}

const char *st_ctx_last_summary_stats(st_ctx *c) { return c ? c->last_summary_stats.c_str() : "{}"; }

}  // extern "C"
