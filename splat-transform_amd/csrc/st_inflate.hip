// st_inflate.hip -- INFLATE on the device: the chunked method of include/st_abi.h, "inflating a
// gzip member on the device".  Every rule is a __host__ __device__ function of st_inflate.h, which a
// host program runs serially in the same steps (tests/native/inflate_cpu_check.cpp); the kernels
// below give its bytes and its statistics.
//
//   k_infl_find     one 256-lane workgroup per chunk: round r tests bit positions
//                   lo + 256 r + lane with candidate_at, the workgroup takes the lowest hit and
//                   leaves.  Nine positions in ten fall at the first three bytes; a lane that goes
//                   on parses the header with its length array in scratch.
//   k_infl_size     one LANE per decoder, 16 decoders per workgroup: size_decoder.  A decoder's
//                   tables (lengths, counts, symbols in code order: 1,024 bytes) are in LDS, 1,028
//                   bytes apart, so the lanes' reads of one table slot fall in different banks.
//   (host)          chain_walk over the decoders' records; offsets by a running sum
//   k_infl_write    one lane per KEPT decoder: write_decoder, 16-bit symbols at its offset
//   k_infl_tails    one workgroup, the only sequential step: kept chunk after kept chunk, the
//                   last 32 KiB of the chunk's symbols become bytes of the output.  The window of
//                   the next chunk is the 32 KiB of OUTPUT before its first byte: those bytes are
//                   final by then, also where a short chunk's window reaches into earlier chunks
//                   (their tails were written in earlier turns), so no window is stored twice.
//   k_infl_resolve  every other symbol becomes a byte; a tile of 16 KiB per workgroup turn, the
//                   tile's first chunk found by bisection, the lanes step on from there.
// No kernel waits on what another workgroup writes; the host waits twice (records, write status).
#include <cstring>
#include <string>
#include <vector>

#include "st_inflate.h"
#include "st_internal.h"
#include "st_webp.h"

namespace st {
namespace {

using namespace infl;

static_assert(CHUNK_DEFAULT == ST_INFLATE_CHUNK && BUDGET_MULT == ST_INFLATE_BUDGET, "the header states both");
static_assert(sizeof(Stats) == sizeof(st_inflate_stats), "st_inflate_stats");

constexpr uint32_t FT = 256;                   // the finder's lanes
constexpr uint32_t DL = 16;                    // decoders (lanes) per workgroup: a quarter of one wave
constexpr uint32_t TSTRIDE = TABLE_BYTES + 4;  // an odd number of words between two decoders' tables
constexpr uint32_t TT = 1024;                  // the tails' lanes
constexpr uint32_t RT = 256, RTILE = 16384;    // resolve: lanes, bytes per turn

__global__ __launch_bounds__(FT) void k_infl_find(const uint8_t *__restrict__ in, uint64_t n, uint32_t chunk_bytes,
                                                  uint64_t *__restrict__ cand) {
    __shared__ uint32_t found;
    const uint32_t t = threadIdx.x, c = blockIdx.x;
    if (c == 0) {
        if (t == 0) cand[0] = 0;
        return;
    }
    uint64_t lo, hi;
    chunk_bits(n, chunk_bytes, c, lo, hi);
    const uint32_t rounds = (8u * chunk_bytes + FT - 1) / FT;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t base = lo + (uint64_t)r * FT;
        if (base >= hi) break;
        if (t == 0) found = ~0u;
        __syncthreads();
        if (base + t < hi && candidate_at(in, n, base + t)) atomicMin(&found, t);
        __syncthreads();
        const uint32_t f = found;
        __syncthreads();
        if (f != ~0u) {
            if (t == 0) cand[c] = base + f;
            return;
        }
    }
    if (t == 0) cand[c] = NONE;
}

__global__ __launch_bounds__(DL) void k_infl_size(const uint8_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ cand,
                                                  uint32_t nchunks, uint64_t expect, uint32_t chunk_bytes,
                                                  DecRec *__restrict__ rec) {
    __shared__ __attribute__((aligned(4))) uint8_t tabs[DL * TSTRIDE];
    const uint32_t c = blockIdx.x * DL + threadIdx.x;
    if (c >= nchunks) return;
    Tables T = tables_at(tabs + threadIdx.x * TSTRIDE);
    DecRec R;
    size_decoder(in, n, cand, nchunks, c, expect, chunk_bytes, T, R);
    rec[c] = R;
}

__global__ __launch_bounds__(DL) void k_infl_write(const uint8_t *__restrict__ in, uint64_t n, const uint32_t *__restrict__ kept,
                                                   const uint64_t *__restrict__ off, uint32_t nkept, uint32_t chunk_bytes,
                                                   DecRec *__restrict__ rec, uint16_t *__restrict__ sym) {
    __shared__ __attribute__((aligned(4))) uint8_t tabs[DL * TSTRIDE];
    const uint32_t i = blockIdx.x * DL + threadIdx.x;
    if (i >= nkept) return;
    Tables T = tables_at(tabs + threadIdx.x * TSTRIDE);
    DecRec R = rec[kept[i]];
    write_decoder(in, n, sym + off[i], off[i], chunk_bytes, T, R);
    rec[kept[i]].markers = R.markers;
    rec[kept[i]].wrote = R.wrote;
}

// the byte of symbol s of the chunk that starts at output byte base; a symbol no write pass makes
// (the host has checked every decoder before this runs) is flagged, not followed
__device__ inline uint8_t checked_byte(uint16_t s, const uint8_t *out, uint64_t base, uint32_t *bad) {
    if (s >= 256u && (s >= 256u + WIN || base + (s - 256u) < WIN)) {
        *bad = 1;
        return 0;
    }
    return resolve_sym(s, out, base);
}

__global__ __launch_bounds__(TT) void k_infl_tails(const uint16_t *__restrict__ sym, const uint64_t *__restrict__ off,
                                                   uint32_t nkept, uint8_t *out, uint32_t *__restrict__ bad) {
    for (uint32_t i = 0; i < nkept; ++i) {
        const uint64_t base = off[i], end = off[i + 1];
        const uint64_t from = end - base > WIN ? end - WIN : base;
        // at most WIN / TT turns; sources lie before `base`, written in earlier turns of i
        for (uint64_t q = from + threadIdx.x; q < end; q += TT) out[q] = checked_byte(sym[q], out, base, bad);
        __syncthreads();
    }
}

__global__ __launch_bounds__(RT) void k_infl_resolve(const uint16_t *__restrict__ sym, const uint64_t *__restrict__ off,
                                                     uint32_t nkept, uint64_t expect, uint64_t tiles, uint8_t *out,
                                                     uint32_t *__restrict__ bad) {
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t q0 = tile * RTILE;
        // the last kept chunk that starts at or before q0
        uint32_t lo = 0, hi = nkept;
        for (uint32_t step = 0; step < 32 && hi - lo > 1; ++step) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= q0) lo = mid;
            else hi = mid;
        }
        uint32_t i = lo;
        for (uint32_t k = 0; k < RTILE / RT; ++k) {
            const uint64_t q = q0 + (uint64_t)k * RT + threadIdx.x;
            if (q >= expect) break;
            while (i + 1 < nkept && off[i + 1] <= q) ++i;
            if (q + WIN < off[i + 1]) out[q] = checked_byte(sym[q], out, off[i], bad);  // the rest is a tail
        }
    }
}

}  // namespace

// The raw deflate stream dev_in[0..n) into dev_out[0..expect).  true = inflated, false = declined.
bool inflate_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_arg,
                 st_inflate_stats *stats) {
    using namespace infl;
    Stats st{};
    if (stats) std::memset(stats, 0, sizeof *stats);
    ST_REQUIRE(chunk_arg == 0 || chunk_arg >= CHUNK_MIN, ST_ERR_ARG, "inflate: chunk_bytes below 256");
    const uint32_t chunk = chunk_arg == 0 ? CHUNK_DEFAULT : chunk_arg > (1u << 30) ? (1u << 30) : (uint32_t)chunk_arg;
    if (n == 0 || n >= (1ull << 40) || (n + chunk - 1) / chunk >= (1ull << 31)) return false;
    const uint32_t nchunks = chunk_count(n, chunk);
    auto *cand = wsT<uint64_t>(c, "infl.cand", nchunks);
    auto *rec = wsT<DecRec>(c, "infl.rec", nchunks);
    {
        KTimer kt(c, "infl.find");
        hipLaunchKernelGGL(k_infl_find, dim3(nchunks), dim3(FT), 0, c->stream, dev_in, n, chunk, cand);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "infl.size");
        hipLaunchKernelGGL(k_infl_size, dim3(grid_for(nchunks, DL)), dim3(DL), 0, c->stream, dev_in, n, cand, nchunks, expect,
                           chunk, rec);
        ST_LAUNCH_CHECK();
    }
    auto *hrec = static_cast<DecRec *>(pinned_slot(c, "infl.rec", sizeof(DecRec) * (size_t)nchunks));
    ST_HIP(hipMemcpyAsync(hrec, rec, sizeof(DecRec) * (size_t)nchunks, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> kept;
    std::vector<uint64_t> off;
    const bool chained = chain_walk(hrec, nchunks, n, expect, kept, off, st);
    if (stats) std::memcpy(stats, &st, sizeof st);
    if (!chained) return false;
    const uint32_t nkept = (uint32_t)kept.size();
    auto *dkept = wsT<uint32_t>(c, "infl.kept", nkept);
    auto *doff = wsT<uint64_t>(c, "infl.off", (size_t)nkept + 1);
    auto *sym = wsT<uint16_t>(c, "infl.sym", expect);
    auto *bad = wsT<uint32_t>(c, "infl.bad", 1);
    auto *hk = static_cast<uint8_t *>(pinned_slot(c, "infl.kept", 12 * (size_t)nkept + 16));
    std::memcpy(hk, off.data(), 8 * ((size_t)nkept + 1));
    std::memcpy(hk + 8 * ((size_t)nkept + 1), kept.data(), 4 * (size_t)nkept);
    ST_HIP(hipMemcpyAsync(doff, hk, 8 * ((size_t)nkept + 1), hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemcpyAsync(dkept, hk + 8 * ((size_t)nkept + 1), 4 * (size_t)nkept, hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemsetAsync(bad, 0, 4, c->stream));
    {
        KTimer kt(c, "infl.write");
        hipLaunchKernelGGL(k_infl_write, dim3(grid_for(nkept, DL)), dim3(DL), 0, c->stream, dev_in, n, dkept, doff, nkept, chunk,
                           rec, sym);
        ST_LAUNCH_CHECK();
    }
    ST_HIP(hipMemcpyAsync(hrec, rec, sizeof(DecRec) * (size_t)nchunks, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < nkept; ++i) {
        if (!hrec[kept[i]].wrote) return false;
        st.markers += hrec[kept[i]].markers;
    }
    if (stats) std::memcpy(stats, &st, sizeof st);
    if (expect == 0) return true;
    {
        KTimer kt(c, "infl.tails");
        hipLaunchKernelGGL(k_infl_tails, dim3(1), dim3(TT), 0, c->stream, sym, doff, nkept, dev_out, bad);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "infl.resolve");
        const uint64_t tiles = (expect + RTILE - 1) / RTILE;
        hipLaunchKernelGGL(k_infl_resolve, dim3(grid_for(tiles, 1, 8192)), dim3(RT), 0, c->stream, sym, doff, nkept, expect,
                           tiles, dev_out, bad);
        ST_LAUNCH_CHECK();
    }
    auto *hb = static_cast<uint32_t *>(pinned_slot(c, "infl.bad", 16));
    ST_HIP(hipMemcpyAsync(hb, bad, 4, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    return hb[0] == 0;
}

// The gzip member dev_in[0..n): its header fields are stepped over on the host (the first 4 KiB
// come down), the stream is inflated, CRC-32 and ISIZE are checked.
bool gunzip_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_arg,
                st_inflate_stats *stats) {
    using namespace infl;
    if (stats) std::memset(stats, 0, sizeof *stats);
    ST_REQUIRE(chunk_arg == 0 || chunk_arg >= CHUNK_MIN, ST_ERR_ARG, "inflate: chunk_bytes below 256");
    if (n < 18) return false;
    const uint64_t nh = n < 4096 ? n : 4096;
    auto *h = static_cast<uint8_t *>(pinned_slot(c, "infl.head", 4096 + 8));
    ST_HIP(hipMemcpyAsync(h, dev_in, nh, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipMemcpyAsync(h + 4096, dev_in + n - 8, 8, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    uint64_t hdr = 0;
    Member M{};
    if (!member_header(h, nh, &hdr) || !member_of(hdr, h + 4096, n, M)) return false;
    if (M.isize != (uint32_t)expect) return false;
    if (!inflate_dev(c, dev_in + M.stream_off, M.stream_len, dev_out, expect, chunk_arg, stats)) return false;
    const uint32_t zero = 0;
    uint32_t crc = 0;
    const uint8_t *p = dev_out;
    crc32_dev(c, &p, &expect, &zero, 1, &crc);
    return crc == M.crc;
}

}  // namespace st

using namespace st;

extern "C" {

int st_gzip_member_layout(const uint8_t *host, uint64_t n, uint64_t *stream_off, uint64_t *stream_len, uint32_t *crc,
                          uint32_t *isize) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE((host || !n) && stream_off && stream_len && crc && isize, ST_ERR_ARG, "NULL argument");
        infl::Member M{};
        if (!infl::member_layout(host, n, M)) return;
        *stream_off = M.stream_off, *stream_len = M.stream_len, *crc = M.crc, *isize = M.isize;
        rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

int st_inflate_head(const uint8_t *host_stream, uint64_t n, uint8_t *out, uint64_t want, uint64_t *got) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE((host_stream || !n) && (out || !want) && got, ST_ERR_ARG, "NULL argument");
        if (infl::inflate_head(host_stream, n, out, want, got)) rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

int st_dev_inflate(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_bytes,
                   st_inflate_stats *stats) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE(c && (dev_in || !n) && (dev_out || !expect), ST_ERR_ARG, "NULL argument");
        use_device(c);
        if (inflate_dev(c, dev_in, n, dev_out, expect, chunk_bytes, stats)) rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

int st_dev_gunzip(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_bytes,
                  st_inflate_stats *stats) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE(c && (dev_in || !n) && (dev_out || !expect), ST_ERR_ARG, "NULL argument");
        use_device(c);
        if (gunzip_dev(c, dev_in, n, dev_out, expect, chunk_bytes, stats)) rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}


// ---- the gzipped .spz FILE, inflated on the device --------------------------------------------------
// (here and not beside st_spz_read: the readers' source is also built alone, into a host program
// without this file; the image's checks and the decode kernel are reached through st_spz_layout and
// st_dev_spz_decode)
}  // extern "C"

namespace {

struct SpzGz {
    infl::Member M;
    uint64_t n;
    int32_t nsh;
};
// member layout, the image's first 16 bytes, st_spz_layout's checks on them against the trailer's
// ISIZE; false = declined (also what st_spz_layout refuses: the caller's host path words that)
bool spz_gz_plan(const uint8_t *file, uint64_t len, SpzGz &G) {
    if (!infl::member_layout(file, len, G.M)) return false;
    uint8_t head[16] = {0};
    uint64_t got = 0;
    if (!infl::inflate_head(file + G.M.stream_off, G.M.stream_len, head, 16, &got)) return false;
    if (got < 16 || G.M.isize < 16) return false;
    return st_spz_layout(head, G.M.isize, &G.n, &G.nsh) == ST_OK;
}
// the member in HBM ("rd.gz"), its image inflated into "rd.file" (4-byte aligned); nullptr = declined
const uint8_t *spz_gz_image(st_ctx *c, const uint8_t *file, uint64_t len, const SpzGz &G, uint64_t chunk_bytes,
                            st_inflate_stats *stats) {
    uint8_t *gz = wsT<uint8_t>(c, "rd.gz", len);
    staged_h2d(c, {HostXfer{const_cast<uint8_t *>(file), gz, len}});
    uint8_t *image = wsT<uint8_t>(c, "rd.file", G.M.isize);
    return gunzip_dev(c, gz, len, image, G.M.isize, chunk_bytes, stats) ? image : nullptr;
}
void decode_image(st_ctx *c, const uint8_t *image, uint64_t len, float *const *cols) {
    const int rc = st_dev_spz_decode(c, image, len, cols);
    if (rc != ST_OK) throw Error(rc, st_last_error());
}

}  // namespace

extern "C" {

int st_spz_gz_layout(const uint8_t *file, uint64_t len, uint64_t *n, int32_t *nsh, uint64_t *image_bytes) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE((file || !len) && n && nsh && image_bytes, ST_ERR_ARG, "NULL argument");
        SpzGz G;
        if (!spz_gz_plan(file, len, G)) return;
        *n = G.n, *nsh = G.nsh, *image_bytes = G.M.isize;
        rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

int st_dev_spz_gz_read(st_ctx *c, const uint8_t *file, uint64_t len, float *const *cols, uint64_t chunk_bytes,
                       st_inflate_stats *stats) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE(c && (file || !len) && cols, ST_ERR_ARG, "NULL argument");
        SpzGz G;
        if (!spz_gz_plan(file, len, G)) return;
        use_device(c);
        const uint8_t *image = spz_gz_image(c, file, len, G, chunk_bytes, stats);
        if (!image) return;
        decode_image(c, image, G.M.isize, cols);
        ST_HIP(hipStreamSynchronize(c->stream));
        rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

int st_spz_gz_read(st_ctx *c, const uint8_t *file, uint64_t len, float *const *host_cols, uint64_t chunk_bytes,
                   st_inflate_stats *stats) {
    int rc = ST_DECLINED;
    const int g = guard([&] {
        ST_REQUIRE(c && (file || !len) && host_cols, ST_ERR_ARG, "NULL argument");
        SpzGz G;
        if (!spz_gz_plan(file, len, G)) return;
        use_device(c);
        const uint8_t *image = spz_gz_image(c, file, len, G, chunk_bytes, stats);
        if (!image) return;
        const int ncol = 14 + G.nsh;
        std::vector<float *> d(ncol);
        for (int k = 0; k < ncol; ++k) d[k] = wsT<float>(c, "rd.col" + std::to_string(k), G.n);
        decode_image(c, image, G.M.isize, d.data());
        if (G.n) {
            std::vector<HostXfer> down;
            for (int k = 0; k < ncol; ++k) {
                ST_REQUIRE(host_cols[k], ST_ERR_ARG, "NULL host column");
                down.push_back(HostXfer{host_cols[k], d[k], G.n * 4});
            }
            staged_d2h(c, down);
        }
        rc = ST_OK;
    });
    return g != ST_OK ? g : rc;
}

}  // extern "C"
