// st_ksplat_write.hip -- the .ksplat writer on the device: typed columns in, the bucketed file image
// out.  The reference has no writer for the format; the rules are this project's own
// (include/st_abi.h, "the .ksplat writer"), anchored on readers/read-ksplat.ts: each field gets the
// code the reader decodes to the nearest value.
//
//   plan     k_ks_min (finite minimum per axis) -> k_ks_keys (cell key per row, the largest cell
//            per axis, the clamp count) -> stable LSD radix sort of (key, row) over only the key bits
//            the largest cells make non-constant (three ranges: x, y, z) -> k_ks_heads + scan (the
//            cell of each sorted row) -> k_ks_cells + three scans over the cells (full buckets,
//            partial buckets, partial rows before each cell) -> k_ks_assign: every sorted row gets
//            its record index and bucket, and the first row of a bucket writes the bucket's centre
//            (and a partial bucket's size).  F, P and the clamp count are all that comes back.
//   records  k_ksplat_records: a 256-lane workgroup takes 256 consecutive OUTPUT records; a lane
//            gathers its row's 14 + 3C values through the order, encodes them and stores the record
//            into the tile's slice in LDS, laid out at the slice's global address modulo 4; after
//            one barrier the slice leaves as coalesced 4-byte stores with single bytes at its
//            unaligned ends (slice_out, k_spz_planes' rule), so the output may lie at any byte.
#include <cstring>

#include "st_ksplat_encode.h"

namespace st {
namespace {

constexpr uint32_t KSW_TILE = 256, KS_CAP = 256;

// order-preserving u64 image of a double, for atomicMin
__host__ __device__ inline unsigned long long dkey(double v) {
    const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
    return (w >> 63) ? ~w : (w | 0x8000000000000000ull);
}
__host__ __device__ inline double dkey_inv(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
// lo_a of the rules from the reduced key: 0 where the axis has no finite value
__host__ __device__ inline double ks_lo(unsigned long long k) {
    const double v = dkey_inv(k);
    return v < __builtin_inf() ? v : 0.0;
}

struct KsStats {
    unsigned long long lo[3];   // dkey of the least finite value per axis (dkey(+Inf): none)
    unsigned long long clamped;
    uint32_t maxcell[3];
    uint32_t pad;
};

struct KsPos {
    WrCol c[3];
};

__global__ void k_ks_init(KsStats *s) {
    for (int a = 0; a < 3; ++a) s->lo[a] = dkey(__builtin_inf()), s->maxcell[a] = 0;
    s->clamped = 0;
}

__global__ __launch_bounds__(256) void k_ks_min(KsPos P, uint64_t n, KsStats *s) {
    __shared__ double sm[4];
    const WrCol col = P.c[blockIdx.y];
    double m = __builtin_inf();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const double v = ta_load(col.p, col.t, i);
        if (__builtin_fabs(v) < __builtin_inf() && v < m) m = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(m, o, 64);
        m = t < m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) m = sm[w] < m ? sm[w] : m;
        if (m < __builtin_inf()) atomicMin(&s->lo[blockIdx.y], dkey(m));
    }
}

__global__ __launch_bounds__(256) void k_ks_keys(KsPos P, uint64_t n, double B, KsStats *s, uint64_t *__restrict__ keys,
                                                 uint32_t *__restrict__ rows) {
    __shared__ uint32_t s_max[3], s_cl;
    if (threadIdx.x < 3) s_max[threadIdx.x] = 0;
    if (threadIdx.x == 3) s_cl = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        uint32_t cell[3], cl = 0;
        for (int a = 0; a < 3; ++a) {
            bool clamped;
            cell[a] = ks_cell(ta_load(P.c[a].p, P.c[a].t, i), ks_lo(s->lo[a]), B, &clamped);
            cl += clamped;
            atomicMax(&s_max[a], cell[a]);
        }
        if (cl) atomicAdd(&s_cl, cl);
        keys[i] = ((uint64_t)cell[2] << 42) | ((uint64_t)cell[1] << 21) | cell[0];
        rows[i] = (uint32_t)i;
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_max[threadIdx.x]) atomicMax(&s->maxcell[threadIdx.x], s_max[threadIdx.x]);
    if (threadIdx.x == 3 && s_cl) atomicAdd(&s->clamped, (unsigned long long)s_cl);
}

// head[i] = 1 where sorted row i opens a cell
__global__ __launch_bounds__(256) void k_ks_heads(const uint64_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// cid: the exclusive scan of the heads (so a head's cell is cid[i], a later row's cid[i] - 1);
// cstart[cell] = its first sorted row, cstart[ncell] = n
__global__ __launch_bounds__(256) void k_ks_cellstart(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ cid,
                                                      uint64_t n, const uint32_t *__restrict__ ncell,
                                                      uint32_t *__restrict__ cstart) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || keys[i] != keys[i - 1]) cstart[cid[i]] = (uint32_t)i;
    if (i == 0) cstart[*ncell] = (uint32_t)n;
}

// per cell: full buckets, whether a partial bucket follows, and its rows (0 past the last cell)
__global__ __launch_bounds__(256) void k_ks_cells(const uint32_t *__restrict__ cstart, const uint32_t *__restrict__ ncell,
                                                  uint64_t n, uint32_t *__restrict__ fullc, uint32_t *__restrict__ partc,
                                                  uint32_t *__restrict__ prem) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    uint32_t m = 0;
    if (j < *ncell) m = cstart[j + 1] - cstart[j];
    fullc[j] = m / KS_CAP;
    partc[j] = (m % KS_CAP) ? 1u : 0u;
    prem[j] = m % KS_CAP;
}

struct KsAssign {
    const uint64_t *keys;      // sorted
    const uint32_t *rows;      // the sort's permutation
    const uint32_t *cid, *cstart, *fulloff, *partoff, *prow;
    const KsStats *stats;
    uint64_t n;
    uint32_t F;
    double B;
    uint32_t *order, *bucket;  // per record
    float *centres;            // 3 per bucket, 4-byte aligned (nullable)
    uint32_t *psize;           // per partial bucket, 4-byte aligned (nullable)
    uint8_t *img_centres, *img_psize;  // the same tables at any byte address (nullable)
};

__global__ __launch_bounds__(256) void k_ks_assign(KsAssign A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    const uint64_t key = A.keys[i];
    const bool head = i == 0 || key != A.keys[i - 1];
    const uint32_t j = head ? A.cid[i] : A.cid[i] - 1;
    const uint32_t start = A.cstart[j], m = A.cstart[j + 1] - start, r = (uint32_t)i - start;
    const uint32_t nfull = m / KS_CAP, rem = m % KS_CAP;
    uint64_t rec;
    uint32_t b;
    bool first;
    if (r < nfull * KS_CAP) {
        b = A.fulloff[j] + r / KS_CAP;
        rec = (uint64_t)A.fulloff[j] * KS_CAP + r;
        first = r % KS_CAP == 0;
    } else {
        b = A.F + A.partoff[j];
        rec = (uint64_t)A.F * KS_CAP + A.prow[j] + (r - nfull * KS_CAP);
        first = r == nfull * KS_CAP;
        if (first) {
            if (A.psize) A.psize[A.partoff[j]] = rem;
            if (A.img_psize) ks_put32(A.img_psize + 4ull * A.partoff[j], rem);
        }
    }
    A.order[rec] = A.rows[i];
    A.bucket[rec] = b;
    if (first) {
        for (int a = 0; a < 3; ++a) {
            const float c = ks_centre(ks_lo(A.stats->lo[a]), (uint32_t)(key >> (21 * a)) & (KS_CELLS - 1), A.B);
            if (A.centres) A.centres[3ull * b + a] = c;
            if (A.img_centres) ks_put32(A.img_centres + 12ull * b + 4 * a, __builtin_bit_cast(uint32_t, c));
        }
    }
}

struct KsRecs {
    const uint32_t *order, *bucket;  // per record: source row (null: the record index), bucket (null in mode 0)
    const float *centres;
    uint64_t n, nbuckets, rec0, nrec;
    uint8_t *out;
    uint32_t stride;
};

template <bool F32>
__global__ __launch_bounds__(KSW_TILE) void k_ksplat_records(WrCols C, KsRecArgs A, KsRecs R) {
    extern __shared__ uint32_t lds32[];
    __shared__ double s_by255[256];
    const uint64_t r0 = (uint64_t)blockIdx.x * KSW_TILE;
    const uint32_t nr = R.nrec - r0 < KSW_TILE ? (uint32_t)(R.nrec - r0) : KSW_TILE;
    const uint32_t t = threadIdx.x;
    uint8_t *g = R.out + r0 * R.stride;
    const uint32_t shift = (uint32_t)((uintptr_t)g & 3);
    if (A.mode == 2) {  // b / 255 once per workgroup instead of three divisions per harmonic
        s_by255[t] = (double)t / 255.0;
        A.by255 = s_by255;
        __syncthreads();
    }
    if (t < nr) {
        const uint64_t rec = R.rec0 + r0 + t;
        // an order or bucket entry outside its table is the caller's error: it reads the last one
        uint64_t row = R.order ? R.order[rec] : rec;
        if (row >= R.n) row = R.n - 1;
        const float *centre = nullptr;
        if (A.mode != 0) {
            uint64_t b = R.bucket[rec];
            if (b >= R.nbuckets) b = R.nbuckets - 1;
            centre = R.centres + 3 * b;
        }
        ksplat_encode<F32>(C, A, row, centre, reinterpret_cast<uint8_t *>(lds32) + shift + t * R.stride);
    }
    __syncthreads();
    slice_out(lds32, shift, nr * R.stride, g);
}

int degree_of(int C) { return C == 3 ? 1 : C == 8 ? 2 : C == 15 ? 3 : 0; }
constexpr int COEFFS[4] = {0, 3, 8, 15};

}  // namespace

uint64_t ksplat_image_size(uint64_t n, int C, int mode, uint64_t full, uint64_t partial) {
    if (!(C == 0 || C == 3 || C == 8 || C == 15) || mode < 0 || mode > 2 || n == 0 || n >= (1ull << 32)) return 0;
    if (full > n || partial > n) return 0;
    return 5120 + 4 * partial + 12 * (full + partial) + n * ksplat_stride(mode, C);
}

float ksplat_block(double block_size) {
    const float B = (float)block_size;
    ST_REQUIRE(B > 0.0f && B < __builtin_inff(), ST_ERR_ARG, "ksplat: block_size must be finite and > 0 as a float32");
    return B;
}

KswParams ksplat_params(const WrTable &W, int mode, int degree, double block_size, float sh_min, float sh_max) {
    ST_REQUIRE(mode >= 0 && mode <= 2, ST_ERR_ARG, "ksplat: mode must be 0, 1 or 2");
    ST_REQUIRE(degree >= -1 && degree <= 3, ST_ERR_ARG, "ksplat: degree must be -1..3");
    ST_REQUIRE(degree <= degree_of(W.C), ST_ERR_ARG, "ksplat: degree is above the table's");
    KswParams P{};
    P.B = ksplat_block(block_size);
    ST_REQUIRE(mode != 2 || (sh_min == sh_min && sh_max == sh_max && __builtin_fabsf(sh_min) < __builtin_inff() &&
                   __builtin_fabsf(sh_max) < __builtin_inff() && sh_min != 0.0f && sh_max != 0.0f && sh_min < sh_max),
               ST_ERR_ARG, "ksplat: sh_min and sh_max must be finite and non-zero with sh_min < sh_max");
    ST_REQUIRE(W.n != 0, ST_ERR_ARG, "ksplat: a .ksplat file of no rows is one the reader refuses");
    ST_REQUIRE(W.n < (1ull << 32), ST_ERR_UNSUPPORTED, "ksplat: the header holds fewer than 2^32 splats");
    P.mode = mode;
    P.c_out = degree < 0 ? W.C : COEFFS[degree];
    P.sh_min = mode == 2 ? sh_min : -1.5f;
    P.sh_max = mode == 2 ? sh_max : 1.5f;
    return P;
}

void ksplat_headers(uint64_t n, const KswParams &P, uint64_t F, uint64_t Pn, uint8_t head[5120]) {
    std::memset(head, 0, 5120);
    auto u32 = [&](size_t o, uint32_t v) {
        for (int k = 0; k < 4; ++k) head[o + k] = (uint8_t)(v >> (8 * k));
    };
    auto u16 = [&](size_t o, uint32_t v) { head[o] = (uint8_t)v, head[o + 1] = (uint8_t)(v >> 8); };
    head[1] = 1;
    u32(4, 1), u32(8, 1), u32(12, (uint32_t)n), u32(16, (uint32_t)n);
    u16(20, (uint32_t)P.mode);
    u32(36, __builtin_bit_cast(uint32_t, P.sh_min)), u32(40, __builtin_bit_cast(uint32_t, P.sh_max));
    const size_t s = 4096;
    u32(s, (uint32_t)n), u32(s + 4, (uint32_t)n), u32(s + 8, KS_CAP), u32(s + 12, (uint32_t)(F + Pn));
    u32(s + 16, __builtin_bit_cast(uint32_t, P.B));
    u16(s + 20, 12);
    u32(s + 24, 32767);
    u32(s + 32, (uint32_t)F), u32(s + 36, (uint32_t)Pn);
    u16(s + 40, (uint32_t)degree_of(P.c_out));
}

// keys, sort and the scans over the cells; F, P and the clamp count read back (waits for the stream)
KswPlan ksplat_plan_begin(st_ctx *c, const WrTable &W, float B) {
    const uint64_t n = W.n;
    ST_REQUIRE(n != 0, ST_ERR_ARG, "ksplat: a .ksplat file of no rows is one the reader refuses");
    ST_REQUIRE(n < (1ull << 32), ST_ERR_UNSUPPORTED, "ksplat: the header holds fewer than 2^32 splats");
    KswPlan K{};
    K.n = n;
    K.B = B;
    KsPos P{{W.cols.c[0], W.cols.c[1], W.cols.c[2]}};
    auto *stats = wsT<KsStats>(c, "ksw.stats", 1);
    K.keys = wsT<uint64_t>(c, "ksw.keys", n);
    K.rows = wsT<uint32_t>(c, "ksw.rows", n);
    K.cid = wsT<uint32_t>(c, "ksw.cid", n);
    K.cstart = wsT<uint32_t>(c, "ksw.cstart", n + 1);
    K.fulloff = wsT<uint32_t>(c, "ksw.fulloff", n);
    K.partoff = wsT<uint32_t>(c, "ksw.partoff", n);
    K.prow = wsT<uint32_t>(c, "ksw.prow", n);
    auto *totals = wsT<uint32_t>(c, "ksw.totals", 4);  // cells, F, P
    K.stats = stats;
    const unsigned nb = grid_for(n, 256);
    {
        KTimer kt(c, "ksw.keys");
        hipLaunchKernelGGL(k_ks_init, dim3(1), dim3(1), 0, c->stream, stats);
        hipLaunchKernelGGL(k_ks_min, dim3(grid_for(n, 4096, 1024), 3), dim3(256), 0, c->stream, P, n, stats);
        hipLaunchKernelGGL(k_ks_keys, dim3(nb), dim3(256), 0, c->stream, P, n, (double)B, stats, K.keys, K.rows);
        ST_LAUNCH_CHECK();
    }
    auto *h = static_cast<KsStats *>(pinned_slot(c, "ksw.stats", sizeof(KsStats) + 16));
    ST_HIP(hipMemcpyAsync(h, stats, sizeof(KsStats), hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    K.clamped = h->clamped;
    {
        // only the bits the largest cell of each axis makes non-constant, least significant axis first
        KTimer kt(c, "ksw.sort");
        for (int a = 0; a < 3; ++a) {
            int bits = 0;
            while (bits < 21 && (h->maxcell[a] >> bits)) ++bits;
            K.sort_bits += bits;
            if (bits) radix_sort_u64(c, K.keys, K.rows, n, 21 * a, 21 * a + bits, "ksw.sort");
        }
    }
    {
        KTimer kt(c, "ksw.buckets");
        uint32_t *head = K.fulloff;  // free until the cells' scans
        hipLaunchKernelGGL(k_ks_heads, dim3(nb), dim3(256), 0, c->stream, K.keys, n, head);
        ST_LAUNCH_CHECK();
        scan_u32(c, head, K.cid, n, totals);
        hipLaunchKernelGGL(k_ks_cellstart, dim3(nb), dim3(256), 0, c->stream, K.keys, K.cid, n, totals, K.cstart);
        hipLaunchKernelGGL(k_ks_cells, dim3(nb), dim3(256), 0, c->stream, K.cstart, totals, n, K.fulloff, K.partoff, K.prow);
        ST_LAUNCH_CHECK();
        scan_u32(c, K.fulloff, K.fulloff, n, totals + 1);
        scan_u32(c, K.partoff, K.partoff, n, totals + 2);
        scan_u32(c, K.prow, K.prow, n, nullptr);
    }
    auto *ht = static_cast<uint32_t *>(pinned_slot(c, "ksw.totals", 32));
    ST_HIP(hipMemcpyAsync(ht, totals, 12, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    K.F = ht[1];
    K.P = ht[2];
    return K;
}

// the per-record tables of a begun plan, queued on the stream: order and bucket (n each), the centres
// (3 (F + P) float32) and partial sizes (P) at 4-byte aligned addresses and / or at any byte address
void ksplat_plan_tables(st_ctx *c, const KswPlan &K, uint32_t *order, uint32_t *bucket, float *centres, uint32_t *psize,
                        uint8_t *img_centres, uint8_t *img_psize) {
    KsAssign A{};
    A.keys = K.keys, A.rows = K.rows, A.cid = K.cid, A.cstart = K.cstart, A.fulloff = K.fulloff, A.partoff = K.partoff;
    A.prow = K.prow, A.stats = static_cast<const KsStats *>(K.stats), A.n = K.n, A.F = (uint32_t)K.F, A.B = (double)K.B;
    A.order = order, A.bucket = bucket, A.centres = centres, A.psize = psize;
    A.img_centres = img_centres, A.img_psize = img_psize;
    KTimer kt(c, "ksw.assign");
    hipLaunchKernelGGL(k_ks_assign, dim3(grid_for(K.n, 256)), dim3(256), 0, c->stream, A);
    ST_LAUNCH_CHECK();
}

void ksplat_records_dev(st_ctx *c, const WrTable &W, const KswParams &P, double block, double range,
                        const uint32_t *order, const uint32_t *bucket, const float *centres, uint64_t nbuckets,
                        uint64_t rec0, uint64_t nrec, uint8_t *out) {
    ST_REQUIRE(rec0 <= W.n && nrec <= W.n - rec0, ST_ERR_ARG, "ksplat records: records outside the table");
    if (!nrec) return;
    ST_REQUIRE(out, ST_ERR_ARG, "NULL argument");
    if (P.mode != 0) {
        ST_REQUIRE(bucket && centres && nbuckets, ST_ERR_ARG, "ksplat records: modes 1 and 2 need the bucket tables");
        ST_REQUIRE((((uintptr_t)bucket | (uintptr_t)centres) & 3) == 0, ST_ERR_ARG,
                   "ksplat records: the bucket tables must be 4-byte aligned");
    }
    ST_REQUIRE(((uintptr_t)order & 3) == 0, ST_ERR_ARG, "ksplat records: the order must be 4-byte aligned");
    KsRecArgs A{};
    A.ps = block / 2.0 / range;
    A.range = range;
    A.sh_lo = (double)P.sh_min;
    A.sh_span = (double)P.sh_max - (double)P.sh_min;
    A.sh_fast = ks_sh8_fast((double)P.sh_min, (double)P.sh_max);
    A.mode = P.mode, A.c_src = W.C, A.c_out = P.c_out;
    KsRecs R{order, bucket, centres, W.n, nbuckets, rec0, nrec, out, ksplat_stride(P.mode, P.c_out)};
    KTimer kt(c, "wr.ksplat");
    const dim3 grid(grid_for(nrec, KSW_TILE));
    const size_t lds = slice_words(KSW_TILE * R.stride) * 4;
    if (W.f32)
        hipLaunchKernelGGL(k_ksplat_records<true>, grid, dim3(KSW_TILE), lds, c->stream, W.cols, A, R);
    else
        hipLaunchKernelGGL(k_ksplat_records<false>, grid, dim3(KSW_TILE), lds, c->stream, W.cols, A, R);
    ST_LAUNCH_CHECK();
}

uint64_t ksplat_plan_image_size(const KswPlan &K, const KswParams &P) {
    return ksplat_image_size(K.n, P.c_out, P.mode, K.F, K.P);
}

void ksplat_image_from_plan(st_ctx *c, const WrTable &W, const KswParams &P, const KswPlan &K, uint8_t *out) {
    ST_REQUIRE(out, ST_ERR_ARG, "NULL argument");
    auto *order = wsT<uint32_t>(c, "ksw.order", W.n);
    auto *bucket = wsT<uint32_t>(c, "ksw.bucket", W.n);
    auto *centres = wsT<float>(c, "ksw.centres", 3 * (K.F + K.P));
    auto *head = static_cast<uint8_t *>(pinned_slot(c, "ksw.head", 5120));
    ksplat_headers(W.n, P, K.F, K.P, head);
    ST_HIP(hipMemcpyAsync(out, head, 5120, hipMemcpyHostToDevice, c->stream));
    ksplat_plan_tables(c, K, order, bucket, centres, nullptr, out + 5120 + 4 * K.P, out + 5120);
    ksplat_records_dev(c, W, P, (double)P.B, 32767.0, order, bucket, centres, K.F + K.P, 0, W.n,
                       out + 5120 + 4 * K.P + 12 * (K.F + K.P));
    ST_HIP(hipStreamSynchronize(c->stream));  // the pinned header may be reused
}

}  // namespace st

using namespace st;

extern "C" {

uint64_t st_ksplat_image_size(uint64_t n, int32_t sh_coeffs, int32_t mode, uint64_t full, uint64_t partial) {
    return ksplat_image_size(n, sh_coeffs, mode, full, partial);
}

int st_dev_ksplat_plan(st_ctx *c, const st_ttable *t, float block_size, uint64_t bucket_cap, uint32_t *dev_order,
                       uint32_t *dev_bucket, float *dev_centres, uint32_t *dev_partial_sizes, uint64_t *full,
                       uint64_t *partial, uint64_t *out_clamped) {
    return guard([&] {
        ST_REQUIRE(c && t && full && partial, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, false, "ksplat plan");
        const float B = ksplat_block(block_size);
        ST_REQUIRE(W.n != 0, ST_ERR_ARG, "ksplat: a .ksplat file of no rows is one the reader refuses");
        ST_REQUIRE(W.n < (1ull << 32), ST_ERR_UNSUPPORTED, "ksplat: the header holds fewer than 2^32 splats");
        ST_REQUIRE(dev_order && dev_bucket && dev_centres && dev_partial_sizes, ST_ERR_ARG, "NULL argument");
        ST_REQUIRE((((uintptr_t)dev_order | (uintptr_t)dev_bucket | (uintptr_t)dev_centres | (uintptr_t)dev_partial_sizes) & 3) == 0,
                   ST_ERR_ARG, "ksplat plan: the outputs must be 4-byte aligned");
        use_device(c);
        const KswPlan K = ksplat_plan_begin(c, W, B);
        *full = K.F;
        *partial = K.P;
        if (out_clamped) *out_clamped = K.clamped;
        ST_REQUIRE(K.F + K.P <= bucket_cap, ST_ERR_ARG, "ksplat plan: the bucket tables are too small");
        ksplat_plan_tables(c, K, dev_order, dev_bucket, dev_centres, dev_partial_sizes, nullptr, nullptr);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

int st_dev_ksplat_records(st_ctx *c, const st_ttable *t, int32_t mode, int32_t degree, float sh_min, float sh_max,
                          float block_size, uint32_t quant_range, const uint32_t *dev_order, const uint32_t *dev_bucket,
                          const float *dev_centres, uint64_t nbuckets, uint64_t rec0, uint64_t nrec, uint8_t *dev_out) {
    return guard([&] {
        ST_REQUIRE(c && t, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, true, "ksplat records");
        // the grid is the caller's here: any float32 block size and any range (a fixture file's own)
        KswParams P = ksplat_params(W, mode, degree, 5.0, mode == 2 ? sh_min : -1.5f, mode == 2 ? sh_max : 1.5f);
        ST_REQUIRE(quant_range != 0, ST_ERR_ARG, "ksplat records: quant_range must not be 0");
        use_device(c);
        ksplat_records_dev(c, W, P, (double)block_size, (double)quant_range, dev_order, dev_bucket, dev_centres, nbuckets,
                           rec0, nrec, dev_out);
    });
}

int st_dev_ksplat_image(st_ctx *c, const st_ttable *t, int32_t mode, int32_t degree, float block_size, float sh_min,
                        float sh_max, uint8_t *dev_out, uint64_t cap, uint64_t *size, uint64_t *out_clamped) {
    return guard([&] {
        ST_REQUIRE(c && t && size, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, true, "ksplat image");
        const KswParams P = ksplat_params(W, mode, degree, block_size, sh_min, sh_max);
        use_device(c);
        const KswPlan K = ksplat_plan_begin(c, W, P.B);
        *size = ksplat_plan_image_size(K, P);
        if (out_clamped) *out_clamped = K.clamped;
        ST_REQUIRE(*size <= cap, ST_ERR_ARG, "ksplat image: the output buffer is too small");
        ksplat_image_from_plan(c, W, P, K, dev_out);
    });
}

}  // extern "C"
