// st_readers.hip -- the .splat, .ksplat and .spz readers on the device.
//
//   .splat    readers/read-splat.ts:14-148: headerless 32-byte rows.  One thread per row, two
//             16-byte loads, 14 coalesced column stores.           read 32 B, write 56 B per splat
//   .ksplat   readers/read-ksplat.ts:103-384: a 4096-byte main header, 1024 bytes per section
//             header, then per section the partial bucket sizes, the bucket centres and records
//             of 24..224 bytes (three compression modes, SH degree per section).  The section
//             walk and the partial-bucket walk stay on the host (ks_plan, ks_bucket_ends); one
//             launch per section decodes 128 records per block out of LDS.
//   .spz      readers/read-spz.ts:49-241 (after the caller's gunzip): a 16-byte header and six
//             planes (positions 9 B, alphas 1 B, colours 3 B, scales 3 B, rotations 3 B, SH D
//             bytes per splat).  A block decodes its 256-splat slice of every plane out of LDS.
//
// Records and plane slices are not lane-friendly (strides of 9, 33, 45 ... bytes): a block's
// contiguous byte range is staged into LDS with coalesced 4-byte loads (stage_bytes, as
// k_ply_cols does) and each lane reads its record's bytes there; every column store has
// consecutive lanes on consecutive rows.  Arithmetic is the reference's: f64 in source order,
// one f32 store per value, V8's Math.log (js::log), NaNs as V8 on x86-64 makes them
// (st_jsmath.h: an invalid operation gives the sign-set default NaN, a NaN operand propagates,
// the first one when both are).
//
// The *_layout functions are the only gate before a launch: they check every view the reference
// constructs (and every read it makes past one) against the file size, so no kernel reads a byte
// outside [0, len) of the uploaded buffer whatever the headers say.
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <string>
#include <vector>

#include "st_internal.h"
#include "st_jsmath.h"

namespace st {
namespace {

constexpr int RD_SH_MAX = 45;
constexpr int RD_COLS_MAX = 14 + RD_SH_MAX;
struct RdCols {
    float *c[RD_COLS_MAX];  // x y z scale_0..2 f_dc_0..2 opacity rot_0..3 f_rest_0..
};

__host__ __device__ inline int sh_count(uint32_t degree) { return degree == 0 ? 0 : degree == 1 ? 9 : degree == 2 ? 24 : 45; }

// ---- JS number semantics shared by the three decoders ----------------------------------------
__host__ __device__ inline float fbits(uint32_t b) { return __builtin_bit_cast(float, b); }
__host__ __device__ inline double quiet(double a) {
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, a) | 0x0008000000000000ull);
}
// a float32 read as a JS number and stored to a Float32Array: the two conversions quiet a
// signalling NaN and change nothing else
__host__ __device__ inline float f32_through_f64(uint32_t b) {
    if ((b & 0x7f800000u) == 0x7f800000u && (b & 0x007fffffu)) b |= 0x00400000u;
    return fbits(b);
}
__host__ __device__ inline double f64_of_f32_bits(uint32_t b) { return (double)f32_through_f64(b); }
// a * b and a + b as the x86-64 SSE unit gives them (see the file comment)
__host__ __device__ inline double mul_js(double a, double b) {
    if (js::isnan_(a)) return quiet(a);
    if (js::isnan_(b)) return quiet(b);
    const double r = a * b;
    return js::isnan_(r) ? js::nan_() : r;
}
__host__ __device__ inline double add_js(double a, double b) {
    if (js::isnan_(a)) return quiet(a);
    if (js::isnan_(b)) return quiet(b);
    const double r = a + b;
    return js::isnan_(r) ? js::nan_() : r;
}
// Math.log(x) stored to a Float32Array.  V8's ieee754::log returns a signalling-NaN constant for
// any x with the sign bit set other than -0 (a negative NaN included), which the store turns
// into 0x7fe00000; js::log covers the rest
__host__ __device__ inline float log_f32(double x) {
    if (js::signbit_(x) && !(x == 0)) return fbits(0x7fe00000u);
    return (float)js::log(x);
}
// (b / 255 - 0.5) / SH_C0                                  read-splat.ts:108-111, read-ksplat.ts:326-329
__host__ __device__ inline float colour_f32(uint32_t b) { return (float)(((double)b / 255.0 - 0.5) / 0.28209479177387814); }
// the inverse sigmoid of an opacity byte                   read-splat.ts:114-116 (the same in all three)
__host__ __device__ inline float opacity_f32(uint32_t b) {
    const double epsilon = 1e-6;
    double p = (double)b / 255.0;
    p = p < 1.0 - epsilon ? p : 1.0 - epsilon;  // Math.min / Math.max of finite numbers
    p = p > epsilon ? p : epsilon;
    return (float)js::log(p / (1.0 - p));
}
// decodeFloat16 (read-ksplat.ts:29-60) as float32 bits: exact, subnormals normalised, NaN = JS NaN
__host__ __device__ inline uint32_t half_bits(uint32_t h) {
    const uint32_t s = (h >> 15) & 1u, e = (h >> 10) & 0x1fu;
    uint32_t m = h & 0x3ffu;
    if (e == 0) {
        if (m == 0) return s << 31;
        int32_t ex = -14;
        while (!(m & 0x400u)) {
            m <<= 1;
            --ex;
        }
        m &= 0x3ffu;
        return (s << 31) | ((uint32_t)(ex + 127) << 23) | (m << 13);
    }
    if (e == 0x1f) return m == 0 ? ((s << 31) | 0x7f800000u) : 0x7fc00000u;
    return (s << 31) | ((e + 112u) << 23) | (m << 13);
}

// little-endian reads of a record's bytes (LDS on the device; any alignment)
__host__ __device__ inline uint32_t rd8(const uint8_t *p, uint32_t o) { return p[o]; }
__host__ __device__ inline uint32_t rd16(const uint8_t *p, uint32_t o) { return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8); }
__host__ __device__ inline uint32_t rd32(const uint8_t *p, uint32_t o) {
    if ((((uintptr_t)p + o) & 3u) == 0) return *(const uint32_t *)(p + o);
    return (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8) | ((uint32_t)p[o + 2] << 16) | ((uint32_t)p[o + 3] << 24);
}

// ---- .splat ----------------------------------------------------------------------------------
// w: the row's eight little-endian words
__host__ __device__ inline void splat_decode(const uint32_t w[8], uint64_t row, const RdCols &C) {
    for (int k = 0; k < 3; ++k) C.c[k][row] = f32_through_f64(w[k]);
    for (int k = 0; k < 3; ++k) C.c[3 + k][row] = log_f32(f64_of_f32_bits(w[3 + k]));
    for (int k = 0; k < 3; ++k) C.c[6 + k][row] = colour_f32((w[6] >> (8 * k)) & 0xffu);
    C.c[9][row] = opacity_f32(w[6] >> 24);
    double q[4];
    for (int k = 0; k < 4; ++k) q[k] = ((double)((w[7] >> (8 * k)) & 0xffu) / 255.0) * 2.0 - 1.0;
    const double length = __builtin_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (length > 0) {
        for (int k = 0; k < 4; ++k) C.c[10 + k][row] = (float)(q[k] / length);
    } else {
        for (int k = 0; k < 4; ++k) C.c[10 + k][row] = k == 3 ? 1.0f : 0.0f;
    }
}

// rows (16-byte aligned) [0, nrows) -> columns at rows [row0, row0 + nrows)
__global__ __launch_bounds__(256) void k_splat_decode(const uint4 *__restrict__ rows, uint64_t nrows, RdCols C,
                                                      uint64_t row0) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const uint4 a = rows[2 * i], b = rows[2 * i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    splat_decode(w, row0 + i, C);
}

void splat_launch(st_ctx *c, const uint8_t *rows, uint64_t nrows, const RdCols &C, uint64_t row0) {
    if (!nrows) return;
    KTimer kt(c, "rd.splat");
    hipLaunchKernelGGL(k_splat_decode, dim3(grid_for(nrows, 256)), dim3(256), 0, c->stream, (const uint4 *)rows,
                       nrows, C, row0);
    ST_LAUNCH_CHECK();
}

void splat_layout(uint64_t size, uint64_t *n) {
    ST_REQUIRE(size % 32 == 0, ST_ERR_ARG, "Invalid .splat file: file size is not a multiple of 32 bytes");
    ST_REQUIRE(size != 0, ST_ERR_ARG, "Invalid .splat file: file is empty");
    *n = size / 32;
}

// ---- staging -----------------------------------------------------------------------------------
// bytes [a, a + len) of buf (4-byte aligned, `total` bytes long, a + len <= total) into lds32 by
// the block's nt threads, whole words where they lie inside the buffer and single bytes at its
// end; the bytes then start at ((uint8_t *)lds32) + the returned skew (a & 3).  lds32 holds
// (len + 6) / 4 + 1 words at most.
__device__ inline uint32_t stage_bytes(uint32_t *lds32, const uint8_t *__restrict__ buf, uint64_t a, uint32_t len,
                                       uint64_t total, uint32_t nt) {
    const uint64_t w0 = a >> 2;
    const uint32_t nw = len ? (uint32_t)(((a + len + 3) >> 2) - w0) : 0;
    const uint32_t *src = (const uint32_t *)buf + w0;
    for (uint32_t i = threadIdx.x; i < nw; i += nt) {
        const uint64_t b = (w0 + i) * 4;
        uint32_t v = 0;
        if (b + 4 <= total) {
            v = src[i];
        } else {
            for (uint32_t k = 0; k < 4; ++k)
                if (b + k < total) v |= (uint32_t)buf[b + k] << (8 * k);
        }
        lds32[i] = v;
    }
    return (uint32_t)(a & 3);
}
constexpr uint32_t stage_words(uint32_t len) { return (len + 6) / 4 + 1; }

// ---- .ksplat ---------------------------------------------------------------------------------
struct KsMode {
    uint32_t base, scale, rot, colour, sh, sh_bytes;
    uint32_t quant;
};
const KsMode KS_MODES[3] = {{44, 12, 24, 40, 44, 4, 1}, {24, 6, 12, 20, 24, 2, 32767}, {24, 6, 12, 20, 24, 1, 32767}};

struct KsSection {
    uint64_t data_off;     // file offset of record 0
    uint64_t centres_off;  // file offset of the bucket centres (4-byte aligned)
    uint64_t row0;         // output row of record 0
    uint64_t full_splats;  // fullBuckets * bucketCapacity
    uint64_t full_buckets;
    uint32_t count, stride, mode, nsh, nsh_max;
    uint32_t bucket_count, capacity;
    uint32_t nends;        // entries of `ends`
    uint32_t ends_at;      // first entry in the shared ends array
    double quant, pos_scale, min_h, range_h;
};

// the bucket of splat s of a section: the full buckets by division, the partial ones by the
// ranges of ks_bucket_ends (how many of them end at or before s)
__host__ __device__ inline uint64_t ks_bucket(const KsSection &S, const uint32_t *ends, uint32_t s) {
    if (s < S.full_splats) return s / S.capacity;
    uint32_t lo = 0, hi = S.nends;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (ends[mid] <= s)
            lo = mid + 1;
        else
            hi = mid;
    }
    return S.full_buckets + lo;
}

// p: the record's bytes; s: its index in the section; centres: the section's bucket centres
__host__ __device__ inline void ks_decode(const uint8_t *p, uint32_t s, const KsSection &S, const uint32_t *centres,
                                          const uint32_t *ends, const RdCols &C) {
    const uint64_t row = S.row0 + s;
    const uint32_t so = S.mode == 0 ? 12 : 6, ro = S.mode == 0 ? 24 : 12, co = S.mode == 0 ? 40 : 20,
                   ho = S.mode == 0 ? 44 : 24;
    if (S.mode == 0) {
        for (uint32_t k = 0; k < 3; ++k) C.c[k][row] = f32_through_f64(rd32(p, 4 * k));
        for (uint32_t k = 0; k < 3; ++k) {
            const double v = f64_of_f32_bits(rd32(p, so + 4 * k));
            C.c[3 + k][row] = v > 0 ? (float)js::log(v) : -10.0f;
        }
        for (uint32_t k = 0; k < 4; ++k) C.c[10 + k][row] = f32_through_f64(rd32(p, ro + 4 * k));
    } else {
        const uint64_t b = ks_bucket(S, ends + S.ends_at, s);
        const bool have = b < S.bucket_count;  // past the last bucket the centre is `undefined`: NaN
        for (uint32_t k = 0; k < 3; ++k) {
            const double centre = have ? f64_of_f32_bits(centres[b * 3 + k]) : (double)fbits(0x7fc00000u);
            const double t = mul_js((double)rd16(p, 2 * k) - S.quant, S.pos_scale);
            C.c[k][row] = (float)add_js(t, centre);
        }
        for (uint32_t k = 0; k < 3; ++k) {
            const double v = (double)fbits(half_bits(rd16(p, so + 2 * k)));
            C.c[3 + k][row] = v > 0 ? (float)js::log(v) : -10.0f;
        }
        for (uint32_t k = 0; k < 4; ++k) C.c[10 + k][row] = fbits(half_bits(rd16(p, ro + 2 * k)));
    }
    for (uint32_t k = 0; k < 3; ++k) C.c[6 + k][row] = colour_f32(rd8(p, co + k));
    C.c[9][row] = opacity_f32(rd8(p, co + 3));
    // band 1's nine values, then band 2's fifteen, then band 3's: channel-major inside each
    const uint32_t per = S.nsh / 3;
    for (uint32_t i = 0; i < S.nsh; ++i) {
        uint32_t channel, coeff;
        if (i < 9) {
            channel = i / 3;
            coeff = i % 3;
        } else if (i < 24) {
            channel = (i - 9) / 5;
            coeff = (i - 9) % 5 + 3;
        } else {
            channel = (i - 24) / 7;
            coeff = (i - 24) % 7 + 8;
        }
        float v;
        if (S.mode == 0)
            v = f32_through_f64(rd32(p, ho + 4 * i));
        else if (S.mode == 1)
            v = fbits(half_bits(rd16(p, ho + 2 * i)));
        else
            v = (float)add_js(S.min_h, mul_js((double)rd8(p, ho + i) / 255.0, S.range_h));
        C.c[14 + channel * per + coeff][row] = v;
    }
    // a section below the file's degree leaves the other columns as allocated: +0
    for (uint32_t i = S.nsh; i < S.nsh_max; ++i) C.c[14 + i][row] = 0.0f;
}

constexpr uint32_t KS_TILE = 128;

__global__ __launch_bounds__(KS_TILE) void k_ksplat_decode(const uint8_t *__restrict__ buf, uint64_t total, KsSection S,
                                                           const uint32_t *__restrict__ ends, RdCols C) {
    extern __shared__ uint32_t lds32[];
    const uint32_t r0 = blockIdx.x * KS_TILE;
    const uint32_t nr = S.count - r0 < KS_TILE ? S.count - r0 : KS_TILE;
    const uint32_t skew = stage_bytes(lds32, buf, S.data_off + (uint64_t)r0 * S.stride, nr * S.stride, total, KS_TILE);
    __syncthreads();
    if (threadIdx.x < nr)
        ks_decode((const uint8_t *)lds32 + skew + threadIdx.x * S.stride, r0 + threadIdx.x, S,
                  (const uint32_t *)(buf + S.centres_off), ends, C);
}

struct KsPlan {
    uint64_t n = 0;
    int nsh = 0;
    uint64_t headers = 0;  // bytes of the main header and the section headers
    std::vector<KsSection> sections;       // the non-empty ones
    std::vector<uint64_t> partial_off;     // per entry of `sections`: file offset and count of its
    std::vector<uint32_t> partial_count;   // partial bucket sizes
};

uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// new DataView(buffer, off, len) over a buffer of `total` bytes (V8's messages)
void need_view(uint64_t off, uint64_t len, uint64_t total) {
    if (off > total)
        throw Error(ST_ERR_ARG, "Start offset " + std::to_string(off) + " is outside the bounds of the buffer");
    ST_REQUIRE(len <= total - off, ST_ERR_ARG, "Invalid DataView length undefined");
}
// new Float32Array / Uint32Array(buffer, off, count)
void need_array4(const char *type, uint64_t off, uint64_t count, uint64_t total) {
    if (off % 4) throw Error(ST_ERR_ARG, std::string("start offset of ") + type + " should be a multiple of 4");
    if (off > total || count > (total - off) / 4)
        throw Error(ST_ERR_ARG, "Invalid typed array length: " + std::to_string(count));
}

// read-ksplat.ts:111-232, :371: the headers of a file of `total` bytes checked as the reader
// checks them, in its order, and every non-empty section's launch parameters.  head: the first
// head_len bytes of the file (at least the main header and the section headers).
void ks_plan(const uint8_t *head, uint64_t head_len, uint64_t total, KsPlan &P) {
    ST_REQUIRE(total >= 4096, ST_ERR_ARG, "File too small to be valid .ksplat format");
    ST_REQUIRE(head_len >= 4096, ST_ERR_ARG, "ksplat: the host headers are shorter than the main header");
    const uint32_t major = head[0], minor = head[1];
    if (major != 0 || minor < 1)
        throw Error(ST_ERR_UNSUPPORTED, "Unsupported version " + std::to_string(major) + "." + std::to_string(minor));
    const uint64_t max_sections = le32(head + 4);
    const uint64_t num_splats = le32(head + 16);
    const uint32_t mode = le16(head + 20);
    if (mode > 2) throw Error(ST_ERR_UNSUPPORTED, "Invalid compression mode: " + std::to_string(mode));
    // getFloat32(36) || -1.5, getFloat32(40) || 1.5: 0, -0 and NaN take the default
    float fmin = fbits(le32(head + 36)), fmax = fbits(le32(head + 40));
    const double min_h = (fmin == 0 || fmin != fmin) ? -1.5 : f64_of_f32_bits(le32(head + 36));
    const double max_h = (fmax == 0 || fmax != fmax) ? 1.5 : f64_of_f32_bits(le32(head + 40));
    ST_REQUIRE(num_splats != 0, ST_ERR_ARG, "Invalid .ksplat file: file is empty");
    for (uint64_t si = 0; si < max_sections; ++si) need_view(4096 + si * 1024, 1024, total);
    P.headers = 4096 + max_sections * 1024;
    ST_REQUIRE(head_len >= P.headers, ST_ERR_ARG, "ksplat: the host headers are shorter than the section headers");
    uint32_t max_degree = 0;
    for (uint64_t si = 0; si < max_sections; ++si) {
        const uint8_t *h = head + 4096 + si * 1024;
        const uint32_t degree = le16(h + 40);
        // (the reference indexes a four-entry table with it: a non-empty section fails on its first
        // read; an empty one derails the offsets of the sections after it, which is not reproduced)
        if (degree > 3) throw Error(ST_ERR_ARG, "ksplat: harmonics degree " + std::to_string(degree) + " of a section");
        if (le32(h) != 0 && degree > max_degree) max_degree = degree;
    }
    P.n = num_splats;
    P.nsh = sh_count(max_degree);
    const KsMode &M = KS_MODES[mode];
    uint64_t cur = P.headers, processed = 0;
    for (uint64_t si = 0; si < max_sections; ++si) {
        const uint8_t *h = head + 4096 + si * 1024;
        const uint64_t count = le32(h), max_splats = le32(h + 4), capacity = le32(h + 8), bucket_count = le32(h + 12);
        const double block = f64_of_f32_bits(le32(h + 16));
        const uint64_t storage = le16(h + 20);
        const uint32_t quant = le32(h + 24) ? le32(h + 24) : M.quant;
        const uint64_t full = le32(h + 32), partial = le32(h + 36);
        const uint32_t nsh = (uint32_t)sh_count(le16(h + 40));
        const uint64_t partial_meta = partial * 4, bucket_storage = storage * bucket_count + partial_meta;
        const uint64_t stride = M.base + (uint64_t)nsh * M.sh_bytes, data_size = stride * max_splats;
        need_array4("Float32Array", cur + partial_meta, bucket_count * 3, total);
        need_array4("Uint32Array", cur, partial, total);
        need_view(cur + bucket_storage, data_size, total);
        ST_REQUIRE(count <= max_splats, ST_ERR_ARG, "Offset is outside the bounds of the DataView");
        if (count) {
            KsSection S{};
            S.data_off = cur + bucket_storage;
            S.centres_off = cur + partial_meta;
            S.row0 = processed;
            S.full_splats = full * capacity;
            S.full_buckets = full;
            S.count = (uint32_t)count;
            S.stride = (uint32_t)stride;
            S.mode = mode;
            S.nsh = nsh;
            S.nsh_max = (uint32_t)P.nsh;
            S.bucket_count = (uint32_t)bucket_count;
            S.capacity = (uint32_t)capacity;
            S.quant = (double)quant;
            S.pos_scale = block / 2.0 / (double)quant;
            S.min_h = min_h;
            S.range_h = max_h - min_h;  // on the host: Inf - Inf is the x86 NaN already
            P.sections.push_back(S);
            P.partial_off.push_back(cur);
            P.partial_count.push_back((uint32_t)partial);
        }
        processed += count;
        cur += data_size + bucket_storage;
    }
    if (processed != num_splats)
        throw Error(ST_ERR_ARG, "Splat count mismatch: expected " + std::to_string(num_splats) + ", processed " +
                                    std::to_string(processed));
}

// read-ksplat.ts:251-269: the reader steps to the next partial bucket at most once per splat, so
// an empty partial bucket still takes the splat that steps onto it.  ends[j]: the first splat
// past partial bucket j's run (clamped to the section); a splat past every entry stays in the
// bucket after the last one
void ks_bucket_ends(const KsSection &S, const uint32_t *sizes, uint32_t npartial, std::vector<uint32_t> &ends) {
    uint64_t start = S.full_splats, base = S.full_splats;
    for (uint32_t j = 0; j < npartial && start < S.count; ++j) {
        uint64_t end = base + sizes[j];
        if (j > 0 && end < start + 1) end = start + 1;
        if (end > S.count) end = S.count;
        ends.push_back((uint32_t)end);
        start = end;
        base += sizes[j];
    }
}

// host: the first host_len bytes of the file; dev: all `total` bytes of it in HBM
void ksplat_decode_dev(st_ctx *c, const uint8_t *host, uint64_t host_len, const uint8_t *dev, uint64_t total,
                       float *const *cols) {
    ST_REQUIRE(((uintptr_t)dev & 3) == 0, ST_ERR_ARG, "ksplat: the device bytes must be 4-byte aligned");
    KsPlan P;
    ks_plan(host, host_len, total, P);
    RdCols C{};
    for (int k = 0; k < 14 + P.nsh; ++k) {
        ST_REQUIRE(cols[k], ST_ERR_ARG, "ksplat: NULL column");
        C.c[k] = cols[k];
    }
    std::vector<uint32_t> ends, sizes;
    for (size_t i = 0; i < P.sections.size(); ++i) {
        KsSection &S = P.sections[i];
        S.ends_at = (uint32_t)ends.size();
        const uint32_t np = P.partial_count[i];
        if (S.mode != 0 && S.count > S.full_splats && np) {
            const uint32_t *src;
            if (P.partial_off[i] + 4ull * np <= host_len) {
                sizes.resize(np);
                std::memcpy(sizes.data(), host + P.partial_off[i], 4ull * np);
            } else {  // the caller kept the headers only: the sizes come down from HBM
                sizes.resize(np);
                ST_HIP(hipMemcpyAsync(sizes.data(), dev + P.partial_off[i], 4ull * np, hipMemcpyDeviceToHost, c->stream));
                ST_HIP(hipStreamSynchronize(c->stream));
            }
            src = sizes.data();
            ks_bucket_ends(S, src, np, ends);
        }
        S.nends = (uint32_t)ends.size() - S.ends_at;
    }
    uint32_t *d_ends = wsT<uint32_t>(c, "rd.ks.ends", ends.size() + 1);
    if (!ends.empty())
        ST_HIP(hipMemcpyAsync(d_ends, ends.data(), 4 * ends.size(), hipMemcpyHostToDevice, c->stream));
    for (const KsSection &S : P.sections) {
        KTimer kt(c, "rd.ksplat");
        hipLaunchKernelGGL(k_ksplat_decode, dim3(grid_for(S.count, KS_TILE)), dim3(KS_TILE),
                           stage_words(KS_TILE * S.stride) * 4, c->stream, dev, total, S, (const uint32_t *)d_ends, C);
        ST_LAUNCH_CHECK();
    }
    // the pageable `ends` was staged by the copy call; nothing else of this frame is read later
}

// ---- .spz ------------------------------------------------------------------------------------
struct SpzPlan {
    uint64_t n;
    uint32_t version, nsh;
    double pos_scale;
    uint64_t pos, alpha, colour, scale, rot, sh;  // plane offsets in the file
};

// read-spz.ts:62-107 over the inflated stream: head = its first min(total, 16) bytes
void spz_plan(const uint8_t *head, uint64_t total, SpzPlan &P) {
    ST_REQUIRE(total >= 4, ST_ERR_ARG, "Invalid DataView length undefined");
    ST_REQUIRE(le32(head) == 0x5053474eu, ST_ERR_ARG, "invalid file header");
    ST_REQUIRE(total >= 16, ST_ERR_ARG, "File too small to be valid .spz format");
    const uint32_t version = le32(head + 4);
    if (!(version == 2 || version == 3)) throw Error(ST_ERR_UNSUPPORTED, "Unsupported version " + std::to_string(version));
    const uint64_t n = le32(head + 8);
    const uint32_t degree = head[12], fractional = head[13];
    // a degree past 3 has no entry in the reader's component table: its SH view gets length NaN
    // (= 0), no f_rest column is made and none is read
    const uint32_t nsh = degree <= 3 ? (uint32_t)sh_count(degree) : 0;
    P.n = n;
    P.version = version;
    P.nsh = nsh;
    P.pos_scale = 1.0 / (double)(int32_t)(1u << (fractional & 31));  // 1 << bits is an int32 shift
    P.pos = 16;
    P.alpha = P.pos + n * 9;
    P.colour = P.alpha + n;
    P.scale = P.colour + n * 3;
    P.rot = P.scale + n * 3;
    P.sh = P.rot + n * 3;
    need_view(P.pos, n * 9, total);
    need_view(P.alpha, n, total);
    need_view(P.colour, n * 3, total);
    need_view(P.scale, n * 3, total);
    need_view(P.rot, n * 3, total);
    need_view(P.sh, n * nsh, total);
    // version 3 reads four bytes at offset splatIndex of the 3n-byte rotation plane
    ST_REQUIRE(!(version == 3 && n == 1), ST_ERR_ARG, "Offset is outside the bounds of the DataView");
}

// v / 127.5 - 1 (a NaN from the version-3 square root propagates as it is)
__host__ __device__ inline double spz_rot_norm(double v) { return js::isnan_(v) ? v : v / 127.5 - 1.0; }

// the splat's slice pointers: 9 position bytes, 1 alpha, 3 colour, 3 scale, the rotation bytes (3 for
// version 2; for version 3 the four bytes at plane offset splatIndex) and nsh SH bytes
__host__ __device__ inline void spz_decode(const uint8_t *pos, uint32_t alpha, const uint8_t *colour, const uint8_t *scale,
                                           const uint8_t *rot, const uint8_t *sh, const SpzPlan &P, uint64_t row,
                                           const RdCols &C) {
    for (uint32_t k = 0; k < 3; ++k) {
        uint32_t v = (uint32_t)pos[3 * k] | ((uint32_t)pos[3 * k + 1] << 8) | ((uint32_t)pos[3 * k + 2] << 16);
        if (v & 0x800000u) v |= 0xff000000u;
        C.c[k][row] = (float)((double)(int32_t)v * P.pos_scale);
    }
    for (uint32_t k = 0; k < 3; ++k) C.c[3 + k][row] = (float)((double)scale[k] / 16.0 - 10.0);
    for (uint32_t k = 0; k < 3; ++k) C.c[6 + k][row] = (float)(((double)colour[k] / 255.0 - 0.5) / 0.15);
    C.c[9][row] = opacity_f32(alpha);
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    if (P.version == 2) {
        for (uint32_t k = 0; k < 3; ++k) r[1 + k] = (double)rot[k];
    } else {
        // getUint32 is big-endian; every later operator works on its ToInt32
        int32_t packed = (int32_t)(((uint32_t)rot[0] << 24) | ((uint32_t)rot[1] << 16) | ((uint32_t)rot[2] << 8) | rot[3]);
        const int32_t largest = packed >> 30;  // -2 .. 1: a negative one matches no component
        double sum_squares = 0;
        for (int32_t i = 3; i >= 0; --i) {
            if (i != largest) {
                const int32_t mag = packed & 511, negbit = (packed >> 9) & 1;
                packed >>= 10;
                double v = 0.7071067811865476 * (double)mag / 511.0;
                if (negbit == 1) v = -v;
                r[i] = v;
                sum_squares += v * v;
            }
        }
        if (largest >= 0) {
            const double s = 1.0 - sum_squares;
            r[largest] = s < 0 ? js::nan_() : __builtin_sqrt(s);  // Math.sqrt of a negative: the x86 NaN
        }
    }
    // (version 3 too: the unpacked components still go through the byte mapping, read-spz.ts:209-217)
    const double r1 = spz_rot_norm(r[1]), r2 = spz_rot_norm(r[2]), r3 = spz_rot_norm(r[3]);
    double r0;
    if (P.version == 2) {
        const double dot = r1 * r1 + r2 * r2 + r3 * r3, s = 1.0 - dot;
        r0 = __builtin_sqrt(s > 0.0 ? s : 0.0);
    } else {
        r0 = spz_rot_norm(r[0]);
    }
    C.c[10][row] = (float)r0;
    C.c[11][row] = (float)r1;
    C.c[12][row] = (float)r2;
    C.c[13][row] = (float)r3;
    const uint32_t per = P.nsh / 3;
    for (uint32_t i = 0; i < P.nsh; ++i)
        C.c[14 + (i % 3) * per + i / 3][row] = (float)(((double)sh[i] - 128.0) / 128.0);
}

constexpr uint32_t SPZ_TILE = 256;
// LDS words of each plane's slice
constexpr uint32_t SPZ_W_POS = stage_words(SPZ_TILE * 9), SPZ_W_ALPHA = stage_words(SPZ_TILE),
                   SPZ_W_3 = stage_words(SPZ_TILE * 3);
constexpr uint32_t spz_lds_words(uint32_t nsh) { return SPZ_W_POS + SPZ_W_ALPHA + 3 * SPZ_W_3 + stage_words(SPZ_TILE * nsh); }

__global__ __launch_bounds__(SPZ_TILE) void k_spz_decode(const uint8_t *__restrict__ buf, uint64_t total, SpzPlan P,
                                                         RdCols C) {
    extern __shared__ uint32_t lds32[];
    uint32_t *l_pos = lds32, *l_alpha = l_pos + SPZ_W_POS, *l_colour = l_alpha + SPZ_W_ALPHA,
             *l_scale = l_colour + SPZ_W_3, *l_rot = l_scale + SPZ_W_3, *l_sh = l_rot + SPZ_W_3;
    const uint64_t r0 = (uint64_t)blockIdx.x * SPZ_TILE;
    const uint32_t nr = P.n - r0 < SPZ_TILE ? (uint32_t)(P.n - r0) : SPZ_TILE;
    const uint32_t k_pos = stage_bytes(l_pos, buf, P.pos + r0 * 9, nr * 9, total, SPZ_TILE);
    const uint32_t k_alpha = stage_bytes(l_alpha, buf, P.alpha + r0, nr, total, SPZ_TILE);
    const uint32_t k_colour = stage_bytes(l_colour, buf, P.colour + r0 * 3, nr * 3, total, SPZ_TILE);
    const uint32_t k_scale = stage_bytes(l_scale, buf, P.scale + r0 * 3, nr * 3, total, SPZ_TILE);
    // version 3: splat s reads plane bytes [s, s + 4); the layout call has checked s + 4 <= 3n
    const uint32_t k_rot = P.version == 2 ? stage_bytes(l_rot, buf, P.rot + r0 * 3, nr * 3, total, SPZ_TILE)
                                          : stage_bytes(l_rot, buf, P.rot + r0, nr + 3, total, SPZ_TILE);
    const uint32_t k_sh = stage_bytes(l_sh, buf, P.sh + r0 * P.nsh, nr * P.nsh, total, SPZ_TILE);
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t >= nr) return;
    spz_decode((const uint8_t *)l_pos + k_pos + 9 * t, ((const uint8_t *)l_alpha)[k_alpha + t],
               (const uint8_t *)l_colour + k_colour + 3 * t, (const uint8_t *)l_scale + k_scale + 3 * t,
               (const uint8_t *)l_rot + k_rot + (P.version == 2 ? 3 * t : t), (const uint8_t *)l_sh + k_sh + P.nsh * t, P,
               r0 + t, C);
}

void spz_decode_dev(st_ctx *c, const uint8_t *head, const uint8_t *dev, uint64_t total, float *const *cols) {
    ST_REQUIRE(((uintptr_t)dev & 3) == 0, ST_ERR_ARG, "spz: the device bytes must be 4-byte aligned");
    SpzPlan P;
    spz_plan(head, total, P);
    if (!P.n) return;
    RdCols C{};
    for (uint32_t k = 0; k < 14 + P.nsh; ++k) {
        ST_REQUIRE(cols[k], ST_ERR_ARG, "spz: NULL column");
        C.c[k] = cols[k];
    }
    KTimer kt(c, "rd.spz");
    hipLaunchKernelGGL(k_spz_decode, dim3(grid_for(P.n, SPZ_TILE)), dim3(SPZ_TILE), spz_lds_words(P.nsh) * 4, c->stream,
                       dev, total, P, C);
    ST_LAUNCH_CHECK();
}

// ---- host forms ----------------------------------------------------------------------------------
// device columns in workspace slots for a host-column call
std::vector<float *> ws_cols(st_ctx *c, int ncol, uint64_t n) {
    std::vector<float *> d(ncol);
    for (int k = 0; k < ncol; ++k) d[k] = wsT<float>(c, "rd.col" + std::to_string(k), n);
    return d;
}
void cols_down(st_ctx *c, const std::vector<float *> &d, float *const *host, uint64_t n) {
    if (!n) return;
    std::vector<HostXfer> down;
    for (size_t k = 0; k < d.size(); ++k) {
        ST_REQUIRE(host[k], ST_ERR_ARG, "NULL host column");
        down.push_back(HostXfer{host[k], d[k], n * 4});
    }
    staged_d2h(c, down);
}
const uint8_t *upload_file(st_ctx *c, const uint8_t *data, uint64_t len) {
    uint8_t *d = wsT<uint8_t>(c, "rd.file", len);
    if (len) staged_h2d(c, {HostXfer{const_cast<uint8_t *>(data), d, len}});
    return d;
}

void splat_read_dev(st_ctx *c, int fd, float *const *cols) {
    struct stat sb;
    ST_REQUIRE(fstat(fd, &sb) == 0, ST_ERR_ARG, "splat: fstat failed");
    uint64_t n = 0;
    splat_layout((uint64_t)sb.st_size, &n);
    RdCols C{};
    for (int k = 0; k < 14; ++k) {
        ST_REQUIRE(cols[k], ST_ERR_ARG, "splat: NULL column");
        C.c[k] = cols[k];
    }
    stream_rows_dev(
        c, fd, 0, n, 32, 256, [&](const uint8_t *rows, uint64_t nr, uint64_t row) { splat_launch(c, rows, nr, C, row); },
        nullptr, "Failed to read expected amount of data from .splat file");
}

}  // namespace
}  // namespace st

using namespace st;

extern "C" {

int st_splat_layout(uint64_t file_size, uint64_t *n, int32_t *nsh) {
    return guard([&] {
        ST_REQUIRE(n && nsh, ST_ERR_ARG, "NULL argument");
        splat_layout(file_size, n);
        *nsh = 0;
    });
}

int st_ksplat_layout(const uint8_t *data, uint64_t len, uint64_t *n, int32_t *nsh) {
    return guard([&] {
        ST_REQUIRE((data || !len) && n && nsh, ST_ERR_ARG, "NULL argument");
        KsPlan P;
        ks_plan(data, len, len, P);
        *n = P.n;
        *nsh = P.nsh;
    });
}

int st_spz_layout(const uint8_t *data, uint64_t len, uint64_t *n, int32_t *nsh) {
    return guard([&] {
        ST_REQUIRE((data || !len) && n && nsh, ST_ERR_ARG, "NULL argument");
        SpzPlan P;
        spz_plan(data, len, P);
        *n = P.n;
        *nsh = (int32_t)P.nsh;
    });
}

int st_dev_splat_decode(st_ctx *c, const uint8_t *rows, uint64_t nrows, float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && cols && (rows || !nrows), ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(((uintptr_t)rows & 15) == 0, ST_ERR_ARG, "splat: rows must be 16-byte aligned");
        ST_REQUIRE(nrows < (1ull << 38), ST_ERR_UNSUPPORTED, "splat: too many rows for one launch");
        use_device(c);
        RdCols C{};
        for (int k = 0; k < 14; ++k) {
            ST_REQUIRE(cols[k] || !nrows, ST_ERR_ARG, "splat: NULL column");
            C.c[k] = cols[k];
        }
        splat_launch(c, rows, nrows, C, 0);
    });
}

int st_dev_ksplat_decode(st_ctx *c, const uint8_t *headers, uint64_t headers_len, const uint8_t *file, uint64_t len,
                         float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && headers && file && cols, ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(headers_len <= len, ST_ERR_ARG, "ksplat: more header bytes than file bytes");
        use_device(c);
        ksplat_decode_dev(c, headers, headers_len, file, len, cols);
    });
}

int st_dev_spz_decode(st_ctx *c, const uint8_t *file, uint64_t len, float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && (file || !len) && cols, ST_ERR_ARG, "NULL argument");
        use_device(c);
        uint8_t head[16] = {0};
        if (len) {
            ST_HIP(hipMemcpyAsync(head, file, len < 16 ? len : 16, hipMemcpyDeviceToHost, c->stream));
            ST_HIP(hipStreamSynchronize(c->stream));
        }
        spz_decode_dev(c, head, file, len, cols);
    });
}

int st_dev_splat_read(st_ctx *c, int32_t fd, float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && cols && fd >= 0, ST_ERR_ARG, "bad argument");
        use_device(c);
        splat_read_dev(c, fd, cols);
    });
}

int st_splat_read(st_ctx *c, int32_t fd, float *const *host_cols) {
    return guard([&] {
        ST_REQUIRE(c && host_cols && fd >= 0, ST_ERR_ARG, "bad argument");
        use_device(c);
        struct stat sb;
        ST_REQUIRE(fstat(fd, &sb) == 0, ST_ERR_ARG, "splat: fstat failed");
        uint64_t n = 0;
        splat_layout((uint64_t)sb.st_size, &n);
        const std::vector<float *> d = ws_cols(c, 14, n);
        splat_read_dev(c, fd, d.data());
        cols_down(c, d, host_cols, n);
    });
}

int st_dev_ksplat_read(st_ctx *c, const uint8_t *data, uint64_t len, float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && (data || !len) && cols, ST_ERR_ARG, "NULL argument");
        KsPlan P;
        ks_plan(data, len, len, P);  // before the upload: a rejected file costs no copy
        use_device(c);
        ksplat_decode_dev(c, data, len, upload_file(c, data, len), len, cols);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

int st_ksplat_read(st_ctx *c, const uint8_t *data, uint64_t len, float *const *host_cols) {
    return guard([&] {
        ST_REQUIRE(c && (data || !len) && host_cols, ST_ERR_ARG, "NULL argument");
        KsPlan P;
        ks_plan(data, len, len, P);
        use_device(c);
        const std::vector<float *> d = ws_cols(c, 14 + P.nsh, P.n);
        ksplat_decode_dev(c, data, len, upload_file(c, data, len), len, d.data());
        cols_down(c, d, host_cols, P.n);
    });
}

int st_dev_spz_read(st_ctx *c, const uint8_t *data, uint64_t len, float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && (data || !len) && cols, ST_ERR_ARG, "NULL argument");
        SpzPlan P;
        spz_plan(data, len, P);
        use_device(c);
        spz_decode_dev(c, data, upload_file(c, data, len), len, cols);
        ST_HIP(hipStreamSynchronize(c->stream));
    });
}

int st_spz_read(st_ctx *c, const uint8_t *data, uint64_t len, float *const *host_cols) {
    return guard([&] {
        ST_REQUIRE(c && (data || !len) && host_cols, ST_ERR_ARG, "NULL argument");
        SpzPlan P;
        spz_plan(data, len, P);
        use_device(c);
        const std::vector<float *> d = ws_cols(c, 14 + (int)P.nsh, P.n);
        spz_decode_dev(c, data, upload_file(c, data, len), len, d.data());
        cols_down(c, d, host_cols, P.n);
    });
}

}  // extern "C"
