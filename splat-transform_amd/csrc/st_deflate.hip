// st_deflate.hip -- DEFLATE on the device: the stream of include/st_abi.h, "the gzip member around
// a .spz image", made of distance-1 runs and one prefix code per 64 KiB segment.  Every rule is a
// __host__ __device__ function of st_deflate.h, which a host program runs serially
// (tests/native/deflate_cpu_check.cpp); the kernels below give its bytes.
//
//   k_defl_hist   one 1,024-lane workgroup per segment.  The segment comes into LDS by aligned
//                 4-byte loads (the input has any alignment: the LDS image keeps its skew), one pad
//                 word after every 16 so that lane t walks bytes [64t, 64t + 64) free of bank
//                 conflicts.  A lane marks the run starts of its 64 bytes in one 64-bit mask; a
//                 prefix maximum and a suffix minimum over the lanes' last and first run starts
//                 give every lane the start of the run it begins in and the end of the run it ends
//                 in, so token_at's closed form (run offset, run length) needs no sequential
//                 parse.  Tokens go into a 286-bin LDS histogram, which is the kernel's output.
//   k_defl_plan   one wave per segment: the lanes rank the used symbols by (count, symbol), lane 0
//                 merges the tree, describes the code and sizes the three codings (plan_segment).
//                 The merge is a chain of dependent LDS reads on one lane, some 0.4 ms a segment;
//                 in a kernel of its own it needs 7 KiB of LDS, not the segment's 68, so some
//                 twenty segments share a CU and their chains overlap.  Out: the segment's bytes,
//                 its choice, and for a dynamic block the code table and header bits (1.5 KiB).
//   k_defl_scan   byte offsets of the segments (64-bit), the stream's size, whether it fits.
//   k_defl_emit   one workgroup per segment again: the same tokens, a scan of the lanes' bit
//                 counts, then every lane ORs its tokens' bits into the segment's output image in
//                 LDS.  The image leaves at the segment's byte offset with the skew of its
//                 destination: whole words between, single bytes at the two ends, so no word that
//                 two segments or the caller's surrounding bytes share is written as a word, and
//                 the output needs no memset.  A stream that does not fit writes nothing.
//
// LDS: the histogram pass holds the padded segment (68 KiB) and 9 KiB of scan arrays and histogram,
// 77 KiB, so two workgroups (32 waves, the CU's limit) share a CU's 160 KiB; the emit pass
// adds the output image (64 KiB + 16 B, the stored form being the largest), 141 KiB, one workgroup
// of 16 waves per CU.
#include <cstring>

#include "st_deflate.h"
#include "st_internal.h"
#include "st_webp.h"

namespace st {
namespace {

using namespace defl;

constexpr uint32_t DT = 1024;           // lanes per workgroup
constexpr uint32_t CH = SEG / DT;       // bytes per lane
constexpr uint32_t CHW = CH / 4;        // words per lane; one pad word follows them in LDS
static_assert(CH <= 64 && CH % 4 == 0 && CH >= 16, "a lane's run starts are one 64-bit mask");
#ifndef ST_DEFL_SEG_TRIAL
static_assert(SEG == ST_DEFLATE_SEG, "the header states the segment size");
#endif
constexpr uint32_t IN_WORDS = (SEG / 4 + 1) + (SEG / 4 + 1) / CHW + 1;  // aligned words of a skewed segment, padded
constexpr uint32_t OUT_WORDS = (3 + SEG + 10 + 3) / 4 + 1;              // a stored segment at any skew
constexpr uint32_t MISC_WORDS = 2 * DT;

struct SegMeta {
    uint32_t btype, bytes, hdr_bits, dist_bits;
};

// the segment g[0..n) into lin: aligned word j at lin[j + j / CHW]; returns the skew g & 3.  (The
// first and last word are read whole: they lie in the 4-byte words that hold g[0] and g[n - 1].)
__device__ inline uint32_t load_segment(const uint8_t *g, uint32_t n, uint32_t *lin) {
    const uint32_t a = (uint32_t)((uintptr_t)g & 3);
    const uint32_t *gb = reinterpret_cast<const uint32_t *>(g - a);
    const uint32_t nw = (a + n + 3) >> 2;
    for (uint32_t j = threadIdx.x; j < nw; j += DT) lin[j + j / CHW] = gb[j];
    return a;
}
// byte p of the segment
__device__ inline uint32_t seg_byte(const uint32_t *lin, uint32_t a, uint32_t p) {
    const uint32_t r = a + p, j = r >> 2;
    return (lin[j + j / CHW] >> (8 * (r & 3))) & 0xffu;
}
// f(i, byte) for the lane's bytes i = 0..cnt-1 (positions 64t + i), in order
template <class F>
__device__ inline void walk_chunk(const uint32_t *lin, uint32_t a, uint32_t cnt, F f) {
    const uint32_t base = threadIdx.x * (CHW + 1);
    uint32_t lo = lin[base];
    for (uint32_t k = 0; k < CHW && 4 * k < cnt; ++k) {
        const uint32_t hi = lin[base + (k + 1 == CHW ? CHW + 1 : k + 1)];
        const uint32_t v = a ? (lo >> (8 * a)) | (hi << (32 - 8 * a)) : lo;
        lo = hi;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
            if (4 * k + b < cnt) f(4 * k + b, (v >> (8 * b)) & 0xffu);
    }
}

// inclusive scans over the workgroup's lanes in lane order / in reverse lane order; part: 16 words
template <class Op>
__device__ inline uint32_t scan_up(uint32_t v, Op op, uint32_t ident, uint32_t *part) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v = op(u, v);
    }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    uint32_t pre = ident;
    for (uint32_t k = 0; k < wave; ++k) pre = op(pre, part[k]);
    __syncthreads();
    return op(pre, v);
}
template <class Op>
__device__ inline uint32_t scan_down(uint32_t v, Op op, uint32_t ident, uint32_t *part) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_down(v, d, 64);
        if (lane + d < 64) v = op(v, u);
    }
    if (lane == 0) part[wave] = v;
    __syncthreads();
    uint32_t post = ident;
    for (uint32_t k = DT / 64 - 1; k > wave; --k) post = op(part[k], post);
    __syncthreads();
    return op(v, post);
}

// the lane's view of the segment's runs
struct Runs {
    uint64_t mask;   // bit i: position 64t + i starts a run
    uint32_t start;  // the start of the run that position 64t lies in
    uint32_t next;   // the first run start after the lane's bytes, or n
    uint32_t cnt;    // the lane's bytes: min(64, n - 64t), 0 past the end
};

// sc: 2 * DT words, part: 16 words.  Ends on a barrier.
__device__ inline Runs find_runs(const uint32_t *lin, uint32_t a, uint32_t n, uint32_t *sc, uint32_t *part) {
    const uint32_t t = threadIdx.x, p0 = t * CH;
    Runs R{0, 0, n, p0 < n ? (n - p0 < CH ? n - p0 : CH) : 0};
    if (R.cnt) {
        uint32_t prev = p0 ? seg_byte(lin, a, p0 - 1) : 0x100u;
        uint64_t m = 0;
        walk_chunk(lin, a, R.cnt, [&](uint32_t i, uint32_t b) {
            if (b != prev) m |= 1ull << i;
            prev = b;
        });
        R.mask = m;
    }
    // last run start + 1 at or before each lane's end; first run start at or after each lane's begin
    const uint32_t last = R.mask ? p0 + (63u - (uint32_t)__builtin_clzll(R.mask)) + 1u : 0u;
    const uint32_t first = R.mask ? p0 + (uint32_t)__builtin_ctzll(R.mask) : n;
    sc[t] = scan_up(last, [](uint32_t x, uint32_t y) { return x > y ? x : y; }, 0u, part);
    sc[DT + t] = scan_down(first, [](uint32_t x, uint32_t y) { return x < y ? x : y; }, n, part);
    __syncthreads();
    R.start = t ? sc[t - 1] - 1u : 0u;  // (position 0 starts a run, so sc[t - 1] >= 1; unused when bit 0 is set)
    R.next = t + 1 < DT ? sc[DT + t + 1] : n;
    __syncthreads();
    return R;
}

// f(token, byte) for every token that starts in the lane's bytes, in order (token_at's values)
template <class F>
__device__ inline void walk_tokens(const uint32_t *lin, uint32_t a, const Runs &R, F f) {
    const uint32_t p0 = threadIdx.x * CH;
    uint32_t s = R.start, e = R.mask ? p0 + (uint32_t)__builtin_ctzll(R.mask) : R.next;
    walk_chunk(lin, a, R.cnt, [&](uint32_t i, uint32_t b) {
        const uint32_t p = p0 + i;
        if ((R.mask >> i) & 1) {
            const uint64_t rest = i + 1 < 64 ? R.mask >> (i + 1) : 0;
            s = p;
            e = rest ? p + 1 + (uint32_t)__builtin_ctzll(rest) : R.next;
        }
        const uint32_t tok = token_at(p - s, e - s);
        if (tok) f(tok, b);
    });
}

__global__ __launch_bounds__(DT) void k_defl_hist(const uint8_t *__restrict__ in, uint64_t n, uint32_t *__restrict__ hist) {
    __shared__ uint32_t lin[IN_WORDS];
    __shared__ uint32_t misc[MISC_WORDS];  // the scans' arrays
    __shared__ uint32_t cnt[NLIT];
    __shared__ uint32_t part[DT / 64];
    const uint32_t t = threadIdx.x;
    const uint64_t seg = blockIdx.x, b0 = seg * SEG;
    const uint32_t len = n - b0 < SEG ? (uint32_t)(n - b0) : SEG;
    const uint32_t a = load_segment(in + b0, len, lin);
    if (t < NLIT) cnt[t] = t == EOB ? 1u : 0u;
    __syncthreads();
    const Runs R = find_runs(lin, a, len, misc, part);
    walk_tokens(lin, a, R, [&](uint32_t tok, uint32_t b) {
        uint32_t eb, ev;
        atomicAdd(&cnt[tok == 1 ? b : len_symbol(tok, &eb, &ev)], 1u);
    });
    __syncthreads();
    if (t < NLIT) hist[seg * NLIT + t] = cnt[t];
}

// one wave per segment: the lanes rank the used symbols, lane 0 builds the code and sizes the codings.
// 7 KiB of LDS, so a CU holds some twenty segments at once and the serial merges overlap.
constexpr uint32_t PT = 64;
__global__ __launch_bounds__(PT) void k_defl_plan(const uint32_t *__restrict__ hist, uint64_t n,
                                                  uint32_t *__restrict__ sizes, SegMeta *__restrict__ meta,
                                                  uint32_t *__restrict__ tabs, uint32_t *__restrict__ hdrs) {
    __shared__ uint32_t cnt[NLIT], tab[NLIT], hdr[HDR_WORDS];
    __shared__ Work W;
    __shared__ uint32_t s_m;
    __shared__ SegMeta s_meta;
    const uint32_t t = threadIdx.x;
    const uint64_t seg = blockIdx.x, b0 = seg * SEG;
    const uint32_t len = n - b0 < SEG ? (uint32_t)(n - b0) : SEG;
    const bool final = b0 + len == n;
    for (uint32_t s = t; s < NLIT; s += PT) cnt[s] = hist[seg * NLIT + s];
    if (t == 0) s_m = 0;
    __syncthreads();
    for (uint32_t s = t; s < NLIT; s += PT)
        if (cnt[s]) {
            const uint32_t r = rank_of(cnt, NLIT, (int)s);
            W.order[r] = (uint16_t)s;
            W.lw[r] = cnt[s];
            atomicAdd(&s_m, 1u);
        }
    __syncthreads();
    if (t == 0) {
        Plan P;
        plan_segment(cnt, len, final, (int)s_m, W, tab, hdr, P);
        s_meta = SegMeta{P.btype, P.bytes, P.hdr_bits, P.dist_bits};
        sizes[seg] = P.bytes;
        meta[seg] = s_meta;
    }
    __syncthreads();
    if (s_meta.btype == 2) {
        for (uint32_t s = t; s < NLIT; s += PT) tabs[seg * NLIT + s] = tab[s];
        for (uint32_t s = t; s < HDR_WORDS; s += PT) hdrs[seg * HDR_WORDS + s] = hdr[s];
    }
}

// off[i] = the bytes before segment i, off[nseg] = res[0] = the stream's size; res[1] = it fits cap
__global__ __launch_bounds__(1024) void k_defl_scan(const uint32_t *__restrict__ sizes, uint32_t nseg, uint64_t cap,
                                                    uint64_t *__restrict__ off, uint64_t *__restrict__ res) {
    __shared__ uint64_t s[2][1024];
    const uint32_t t = threadIdx.x, per = (nseg + 1023) / 1024;
    const uint32_t i0 = t * per < nseg ? t * per : nseg, i1 = i0 + per < nseg ? i0 + per : nseg;
    uint64_t sum = 0;
    for (uint32_t i = i0; i < i1; ++i) sum += sizes[i];
    int cur = 0;
    s[0][t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= d ? s[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    uint64_t o = s[cur][t] - sum;
    for (uint32_t i = i0; i < i1; ++i) {
        off[i] = o;
        o += sizes[i];
    }
    if (t == 1023) {
        off[nseg] = s[cur][t];
        res[0] = s[cur][t];
        res[1] = s[cur][t] <= cap;
    }
}

// bits [shift, shift + bytes) of the image l32 -> g[0, bytes) where shift = g & 3: whole words
// between, single bytes at the two ends
__device__ inline void image_out(const uint32_t *l32, uint32_t shift, uint32_t bytes, uint8_t *g) {
    const uint8_t *l8 = reinterpret_cast<const uint8_t *>(l32);
    uint8_t *base = g - shift;  // 4-byte aligned
    const uint32_t end = shift + bytes;
    const uint32_t w0 = (shift + 3) >> 2, w1 = end >> 2;
    for (uint32_t i = w0 + threadIdx.x; i < w1; i += DT) reinterpret_cast<uint32_t *>(base)[i] = l32[i];
    const uint32_t head_end = w0 * 4 < end ? w0 * 4 : end;
    const uint32_t tail = w1 * 4 > head_end ? w1 * 4 : head_end;
    if (shift + threadIdx.x < head_end) base[shift + threadIdx.x] = l8[shift + threadIdx.x];
    if (tail + threadIdx.x < end) base[tail + threadIdx.x] = l8[tail + threadIdx.x];
}

// v's low nb bits (nb <= 32) into the zeroed image at bit position pos
__device__ inline void or_bits(uint32_t *lout, uint32_t pos, uint32_t v, uint32_t nb) {
    if (!nb) return;
    const uint32_t i = pos >> 5, sh = pos & 31u;
    atomicOr(&lout[i], v << sh);
    if (sh + nb > 32) atomicOr(&lout[i + 1], v >> (32 - sh));
}

__global__ __launch_bounds__(DT) void k_defl_emit(const uint8_t *__restrict__ in, uint64_t n,
                                                  const SegMeta *__restrict__ meta, const uint32_t *__restrict__ tabs,
                                                  const uint32_t *__restrict__ hdrs, const uint64_t *__restrict__ off,
                                                  const uint64_t *__restrict__ res, uint8_t *__restrict__ out) {
    __shared__ uint32_t lin[IN_WORDS];
    __shared__ uint32_t lout[OUT_WORDS];
    __shared__ uint32_t misc[MISC_WORDS];
    __shared__ uint32_t tab[NLIT];
    __shared__ uint32_t part[DT / 64];
    if (!res[1]) return;  // the stream does not fit: nothing is written
    const uint32_t t = threadIdx.x;
    const uint64_t seg = blockIdx.x, b0 = seg * SEG;
    const uint32_t len = n - b0 < SEG ? (uint32_t)(n - b0) : SEG;
    const bool final = b0 + len == n;
    const SegMeta M = meta[seg];
    uint8_t *dst = out + off[seg];
    const uint32_t sk = (uint32_t)((uintptr_t)dst & 3);
    const uint32_t a = load_segment(in + b0, len, lin);
    const uint32_t ow = (sk + M.bytes + 3) / 4 + 1;
    for (uint32_t i = t; i < ow && i < OUT_WORDS; i += DT) lout[i] = 0;
    if (t < NLIT) tab[t] = M.btype == 2 ? tabs[seg * NLIT + t] : fixed_entry(t);
    __syncthreads();
    uint8_t *lout8 = reinterpret_cast<uint8_t *>(lout);
    if (M.btype == 0) {
        // stored blocks of at most 65,535 bytes: 5 header bytes each
        for (uint32_t i = t; i < len; i += DT) lout8[sk + i + 5 * (i / STORED_MAX + 1)] = (uint8_t)seg_byte(lin, a, i);
        const uint32_t nblk = (len + STORED_MAX - 1) / STORED_MAX;
        if (t < nblk) {
            const uint32_t b = t * STORED_MAX, bl = len - b < STORED_MAX ? len - b : STORED_MAX;
            uint8_t *h = lout8 + sk + b + 5 * t;
            h[0] = final && t + 1 == nblk ? 1 : 0;
            h[1] = (uint8_t)bl, h[2] = (uint8_t)(bl >> 8), h[3] = (uint8_t)~bl, h[4] = (uint8_t)(~bl >> 8);
        }
    } else {
        const Runs R = find_runs(lin, a, len, misc, part);
        uint32_t bits = 0;
        walk_tokens(lin, a, R, [&](uint32_t tok, uint32_t b) {
            uint32_t eb = 0, ev = 0;
            const uint32_t e = tab[tok == 1 ? b : len_symbol(tok, &eb, &ev)];
            bits += (e >> 16) + (tok == 1 ? 0u : eb + M.dist_bits);
        });
        const uint32_t endbit = scan_up(bits, [](uint32_t x, uint32_t y) { return x + y; }, 0u, part);
        // block header: fixed = BFINAL, BTYPE 01; dynamic = the saved bits
        const uint32_t origin = 8 * sk;
        if (M.btype == 1) {
            if (t == 0) or_bits(lout, origin, (final ? 1u : 0u) | 2u, 3);
        } else if (32 * t < M.hdr_bits) {
            const uint32_t left = M.hdr_bits - 32 * t;
            or_bits(lout, origin + 32 * t, hdrs[seg * HDR_WORDS + t], left < 32 ? left : 32);
        }
        // the lane's tokens: bits gather in a 64-bit accumulator and leave a word at a time
        uint32_t pos = origin + M.hdr_bits + (endbit - bits);
        uint32_t wi = pos >> 5, nacc = pos & 31u;
        uint64_t acc = 0;
        walk_tokens(lin, a, R, [&](uint32_t tok, uint32_t b) {
            uint32_t eb = 0, ev = 0;
            const uint32_t e = tab[tok == 1 ? b : len_symbol(tok, &eb, &ev)];
            const uint32_t cl = e >> 16;
            const uint32_t v = tok == 1 ? e & 0xffffu : (e & 0xffffu) | ev << cl;
            acc |= (uint64_t)v << nacc;
            nacc += cl + (tok == 1 ? 0u : eb + M.dist_bits);
            if (nacc >= 32) {
                atomicOr(&lout[wi++], (uint32_t)acc);
                acc >>= 32;
                nacc -= 32;
            }
        });
        if (nacc && (uint32_t)acc) atomicOr(&lout[wi], (uint32_t)acc);
        if (t == DT - 1) or_bits(lout, origin + M.hdr_bits + endbit, tab[EOB] & 0xffffu, tab[EOB] >> 16);
        __syncthreads();
        // not the last segment: an empty stored block follows (000, zeros to the byte, 00 00 FF FF)
        if (!final && t < 2) lout8[sk + M.bytes - 2 + t] = 0xff;
    }
    __syncthreads();
    image_out(lout, sk, M.bytes, dst);
}

}  // namespace

// the stream of dev_in[0..n) at dev_out; above cap: ST_ERR_ARG and nothing is written.  Waits for
// the kernels (the size).
uint64_t deflate_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap) {
    if (n == 0) {
        ST_REQUIRE(cap >= 2, ST_ERR_ARG, "deflate: the output buffer is too small");
        auto *h = static_cast<uint8_t *>(pinned_slot(c, "defl.empty", 16));
        h[0] = 3, h[1] = 0;
        ST_HIP(hipMemcpyAsync(dev_out, h, 2, hipMemcpyHostToDevice, c->stream));
        ST_HIP(hipStreamSynchronize(c->stream));
        return 2;
    }
    const uint64_t nseg64 = (n + SEG - 1) / SEG;
    ST_REQUIRE(nseg64 < (1ull << 31), ST_ERR_UNSUPPORTED, "deflate: too many segments for one launch");
    const uint32_t nseg = (uint32_t)nseg64;
    auto *hist = wsT<uint32_t>(c, "defl.hist", (size_t)nseg * NLIT);
    auto *sizes = wsT<uint32_t>(c, "defl.sizes", nseg);
    auto *meta = wsT<SegMeta>(c, "defl.meta", nseg);
    auto *tabs = wsT<uint32_t>(c, "defl.tabs", (size_t)nseg * NLIT);
    auto *hdrs = wsT<uint32_t>(c, "defl.hdrs", (size_t)nseg * HDR_WORDS);
    auto *off = wsT<uint64_t>(c, "defl.off", (size_t)nseg + 1);
    auto *res = wsT<uint64_t>(c, "defl.res", 2);
    {
        KTimer kt(c, "defl.hist");
        hipLaunchKernelGGL(k_defl_hist, dim3(nseg), dim3(DT), 0, c->stream, dev_in, n, hist);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "defl.plan");
        hipLaunchKernelGGL(k_defl_plan, dim3(nseg), dim3(PT), 0, c->stream, hist, n, sizes, meta, tabs, hdrs);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "defl.scan");
        hipLaunchKernelGGL(k_defl_scan, dim3(1), dim3(1024), 0, c->stream, sizes, nseg, cap, off, res);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "defl.emit");
        hipLaunchKernelGGL(k_defl_emit, dim3(nseg), dim3(DT), 0, c->stream, dev_in, n, meta, tabs, hdrs, off, res, dev_out);
        ST_LAUNCH_CHECK();
    }
    auto *h = static_cast<uint64_t *>(pinned_slot(c, "defl.res", 16));
    ST_HIP(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    ST_REQUIRE(h[1] != 0, ST_ERR_ARG, "deflate: the output buffer is too small");
    return h[0];
}

// the gzip member of dev_in[0..n) at dev_out: header, stream, CRC-32, n mod 2^32
uint64_t gzip_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap) {
    ST_REQUIRE(cap >= 18 + 2, ST_ERR_ARG, "gzip: the output buffer is too small");
    const uint64_t size = deflate_dev(c, dev_in, n, dev_out + 10, cap - 18);
    const uint32_t zero = 0;
    uint32_t crc = 0;
    crc32_dev(c, &dev_in, &n, &zero, 1, &crc);
    auto *h = static_cast<uint8_t *>(pinned_slot(c, "defl.gz", 32));
    const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    std::memcpy(h, head, 10);
    const uint32_t tail[2] = {crc, (uint32_t)n};
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 4; ++k) h[10 + 4 * i + k] = (uint8_t)(tail[i] >> (8 * k));
    ST_HIP(hipMemcpyAsync(dev_out, h, 10, hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemcpyAsync(dev_out + 10 + size, h + 10, 8, hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    return size + 18;
}

}  // namespace st

using namespace st;

extern "C" {

uint64_t st_deflate_bound(uint64_t n) { return defl::deflate_bound(n); }
uint64_t st_gzip_bound(uint64_t n) { return defl::gzip_bound(n); }

int st_dev_deflate(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap, uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(c && size && (dev_in || n == 0) && dev_out, ST_ERR_ARG, "NULL argument");
        use_device(c);
        *size = deflate_dev(c, dev_in, n, dev_out, cap);
    });
}

int st_dev_gzip(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap, uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(c && size && (dev_in || n == 0) && dev_out, ST_ERR_ARG, "NULL argument");
        use_device(c);
        *size = gzip_dev(c, dev_in, n, dev_out, cap);
    });
}

}  // extern "C"
