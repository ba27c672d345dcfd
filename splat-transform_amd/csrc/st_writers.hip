// st_writers.hip -- the .splat and .spz writers on the device: typed columns in, the packed bytes
// out.  The reference has no writer for either format; the encode rules are this project's own
// (include/st_abi.h, "the .splat and .spz writers"): each field gets the code the reference's own
// reader (readers/read-splat.ts, readers/read-spz.ts) decodes to the nearest value.
//
//   .splat   k_splat_rows: one thread per row, 14 coalesced column loads of any type, the 32-byte
//            row as two 16-byte stores (eight 4-byte stores where the output is only 4-byte
//            aligned).                                       read 56 B, write 32 B per splat
//   .spz     k_spz_planes, the mirror of k_spz_decode: a workgroup takes a 256-splat tile; lanes
//            sit on consecutive rows for every column load (the 3C harmonics streams included)
//            and put their splat's bytes into the tile's slice of each plane in LDS (9 + 1 + 3 +
//            3 + 3 + 3C bytes per splat, 16 KiB at degree 3); each slice then leaves as coalesced
//            4-byte stores.  A plane starts at any byte (16 + 9n, + n, + 3n ... in a file): its
//            slice is laid out in LDS at the same offset modulo 4, only the words that lie wholly
//            inside the slice are stored as words, and the up-to-3 bytes at either end go out one
//            by one -- no word that two tiles, two planes or a plane and the caller's surrounding
//            bytes share is ever written as a word.  A full tile's slice is a multiple of 4 bytes
//            in every plane, so each plane has one skew for all its tiles.
//
// Arithmetic: JS numbers (f64) in the order the rules are written, one rounding per operation
// (the library is built with contraction off), V8's Math.exp (st_jsmath.h).  The per-splat encode
// functions are __host__ __device__, as the readers' decode functions are
// (tests/native/writers_cpu_check.cpp runs them on the CPU).
#include <cstring>

#include "st_wr_encode.h"

namespace st {
namespace {

// ---- .splat ----------------------------------------------------------------------------------
// w: the row's eight little-endian words
template <bool F32>
__host__ __device__ inline void splat_encode(const WrCols &C, uint64_t row, uint32_t w[8]) {
    for (int k = 0; k < 3; ++k) {
        const WrCol &col = C.c[k];
        // a float32 column's bits go out unchanged (NaN payloads included); else Math.fround(v)
        w[k] = col.t == ST_PLY_FLOAT ? static_cast<const uint32_t *>(col.p)[row]
                                     : __builtin_bit_cast(uint32_t, js::f32_store(ta_load(col.p, col.t, row)));
    }
    for (int k = 0; k < 3; ++k)
        w[3 + k] = __builtin_bit_cast(uint32_t, js::f32_store(js::exp(wr_load<F32>(C.c[3 + k], row))));
    uint32_t b = 0;
    for (int k = 0; k < 3; ++k) b |= q8((wr_load<F32>(C.c[6 + k], row) * SH_C0 + 0.5) * 255.0) << (8 * k);
    w[6] = b | (q8(js::sigmoid(wr_load<F32>(C.c[9], row)) * 255.0) << 24);
    double u[4];
    unit_quat<F32>(C, row, u);
    b = 0;
    for (int k = 0; k < 4; ++k) b |= q8((u[k] + 1.0) * 127.5) << (8 * k);
    w[7] = b;
}

// rows [row0, row0 + nrows) -> out (4-byte aligned; wide: 16-byte aligned)
template <bool F32>
__global__ __launch_bounds__(256) void k_splat_rows(WrCols C, uint64_t row0, uint64_t nrows, uint8_t *__restrict__ out,
                                                    int wide) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    uint32_t w[8];
    splat_encode<F32>(C, row0 + i, w);
    if (wide) {
        uint4 *o = reinterpret_cast<uint4 *>(out) + 2 * i;
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + 8 * i;
        for (int k = 0; k < 8; ++k) o[k] = w[k];
    }
}

// ---- .spz ------------------------------------------------------------------------------------
// one splat's bytes of the six planes (a null pointer skips that plane's bytes); returns how many
// of its three position values were NaN or fell outside [-2^23, 2^23 - 1] before the clamp.
// pos_scale = 2^fractional_bits, nsh = 3C
template <bool F32>
__host__ __device__ inline uint32_t spz_encode(const WrCols &C, uint32_t nsh, double pos_scale, uint64_t row,
                                               uint8_t *pos, uint8_t *alpha, uint8_t *colour, uint8_t *scale,
                                               uint8_t *rot, uint8_t *sh) {
    uint32_t clamped = 0;
    for (int k = 0; k < 3; ++k) {
        const double v = wr_load<F32>(C.c[k], row);
        int32_t q = 0;
        if (v != v) {
            ++clamped;
        } else {
            const double f = __builtin_floor(v * pos_scale + 0.5);
            if (f < -8388608.0) q = -8388608, ++clamped;
            else if (f > 8388607.0) q = 8388607, ++clamped;
            else q = (int32_t)f;
        }
        if (pos) {
            pos[3 * k] = (uint8_t)q;
            pos[3 * k + 1] = (uint8_t)((uint32_t)q >> 8);
            pos[3 * k + 2] = (uint8_t)((uint32_t)q >> 16);
        }
    }
    if (alpha) *alpha = (uint8_t)q8(js::sigmoid(wr_load<F32>(C.c[9], row)) * 255.0);
    if (colour)
        for (int k = 0; k < 3; ++k) colour[k] = (uint8_t)q8((wr_load<F32>(C.c[6 + k], row) * 0.15 + 0.5) * 255.0);
    if (scale)
        for (int k = 0; k < 3; ++k) scale[k] = (uint8_t)q8((wr_load<F32>(C.c[3 + k], row) + 10.0) * 16.0);
    if (rot) {
        double u[4];
        unit_quat<F32>(C, row, u);
        if (u[0] < 0.0)
            for (int k = 0; k < 4; ++k) u[k] = -u[k];
        for (int k = 1; k < 4; ++k) rot[k - 1] = (uint8_t)q8((u[k] + 1.0) * 127.5);
    }
    if (sh) {
        // byte i = 3 * coefficient + channel comes from f_rest_{channel * C + coefficient}
        const uint32_t per = nsh / 3;
        for (uint32_t j = 0; j < per; ++j)
            for (uint32_t ch = 0; ch < 3; ++ch)
                sh[3 * j + ch] = (uint8_t)q8(wr_load<F32>(C.c[14 + ch * per + j], row) * 128.0 + 128.0);
    }
    return clamped;
}

constexpr uint32_t SPZW_TILE = 256;
constexpr uint32_t SPZW_W_POS = slice_words(SPZW_TILE * 9), SPZW_W_1 = slice_words(SPZW_TILE),
                   SPZW_W_3 = slice_words(SPZW_TILE * 3);
constexpr uint32_t spzw_lds_words(uint32_t nsh) {
    return SPZW_W_POS + SPZW_W_1 + 3 * SPZW_W_3 + slice_words(SPZW_TILE * nsh);
}

struct SpzwArgs {
    uint8_t *plane[6];  // where row0's bytes of positions, alphas, colours, scales, rotations, harmonics go
    double pos_scale;
    uint64_t row0, nrows;
    uint32_t nsh;
};

template <bool F32>
__global__ __launch_bounds__(SPZW_TILE) void k_spz_planes(WrCols C, SpzwArgs A, unsigned long long *clamped) {
    extern __shared__ uint32_t lds32[];
    __shared__ uint32_t s_clamped;
    const uint32_t stride[6] = {9, 1, 3, 3, 3, A.nsh};
    uint32_t *l[6];
    l[0] = lds32, l[1] = l[0] + SPZW_W_POS, l[2] = l[1] + SPZW_W_1, l[3] = l[2] + SPZW_W_3, l[4] = l[3] + SPZW_W_3,
    l[5] = l[4] + SPZW_W_3;
    const uint64_t r0 = (uint64_t)blockIdx.x * SPZW_TILE;
    const uint32_t nr = A.nrows - r0 < SPZW_TILE ? (uint32_t)(A.nrows - r0) : SPZW_TILE;
    const uint32_t t = threadIdx.x;
    uint8_t *g[6], *mine[6];
    uint32_t shift[6];
    for (int p = 0; p < 6; ++p) {
        g[p] = A.plane[p] && stride[p] ? A.plane[p] + r0 * stride[p] : nullptr;
        shift[p] = (uint32_t)((uintptr_t)g[p] & 3);
        mine[p] = g[p] ? reinterpret_cast<uint8_t *>(l[p]) + shift[p] + t * stride[p] : nullptr;
    }
    if (t == 0) s_clamped = 0;
    __syncthreads();
    if (t < nr) {
        const uint32_t cl = spz_encode<F32>(C, A.nsh, A.pos_scale, A.row0 + r0 + t, mine[0], mine[1], mine[2], mine[3],
                                            mine[4], mine[5]);
        if (cl) atomicAdd(&s_clamped, cl);
    }
    __syncthreads();
    for (int p = 0; p < 6; ++p)
        if (g[p]) slice_out(l[p], shift[p], nr * stride[p], g[p]);
    if (t == 0 && s_clamped) atomicAdd(clamped, (unsigned long long)s_clamped);  // one per workgroup
}

const char *const WR_NAMES[14] = {"x", "y", "z", "scale_0", "scale_1", "scale_2", "f_dc_0",
                                  "f_dc_1", "f_dc_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3"};

}  // namespace

WrTable wr_table(const st_ttable *t, bool with_sh, const char *what) {
    ST_REQUIRE(t->ncol >= 0 && (t->ncol == 0 || (t->names && t->types && t->cols)), ST_ERR_ARG,
               std::string(what) + ": bad table");
    WrTable W{};
    W.n = t->n;
    W.f32 = true;
    // the first column of a name wins
    auto find = [&](const std::string &name) {
        for (int i = 0; i < t->ncol; ++i)
            if (t->names[i] && name == t->names[i]) return i;
        return -1;
    };
    auto take = [&](int slot, const std::string &name) {
        const int i = find(name);
        ST_REQUIRE(i >= 0, ST_ERR_ARG, std::string(what) + ": missing column " + name);
        const int z = type_size(t->types[i]);
        ST_REQUIRE(z > 0, ST_ERR_ARG, std::string(what) + ": bad column type");
        ST_REQUIRE(t->n == 0 || t->cols[i], ST_ERR_ARG, std::string(what) + ": NULL column");
        ST_REQUIRE(((uintptr_t)t->cols[i] & (uintptr_t)(z - 1)) == 0, ST_ERR_ARG, std::string(what) + ": misaligned column");
        W.cols.c[slot] = WrCol{t->cols[i], t->types[i], 0};
        W.f32 = W.f32 && t->types[i] == ST_PLY_FLOAT;
    };
    for (int k = 0; k < 14; ++k) take(k, WR_NAMES[k]);
    if (with_sh) {
        W.C = band_coeffs([&](const char *nm) { return find(nm) >= 0; });
        for (int i = 0; i < 3 * W.C; ++i) take(14 + i, "f_rest_" + std::to_string(i));
    }
    return W;
}

uint64_t spz_image_size(uint64_t n, int C) {
    if (!(C == 0 || C == 3 || C == 8 || C == 15) || n >= (1ull << 32)) return 0;
    return 16 + n * (19 + 3 * (uint64_t)C);
}

static void spz_header(uint64_t n, int C, int fractional_bits, uint8_t head[16]) {
    const uint32_t words[3] = {0x5053474eu, 2u, (uint32_t)n};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 4; ++k) head[4 * i + k] = (uint8_t)(words[i] >> (8 * k));
    head[12] = (uint8_t)(C == 3 ? 1 : C == 8 ? 2 : C == 15 ? 3 : 0);
    head[13] = (uint8_t)fractional_bits;
    head[14] = head[15] = 0;
}

void splat_rows_dev(st_ctx *c, const WrTable &W, uint64_t row0, uint64_t nrows, uint8_t *out) {
    ST_REQUIRE(row0 <= W.n && nrows <= W.n - row0, ST_ERR_ARG, "splat rows: rows outside the table");
    ST_REQUIRE(((uintptr_t)out & 3) == 0, ST_ERR_ARG, "splat rows: output must be 4-byte aligned");
    ST_REQUIRE(nrows < (1ull << 38), ST_ERR_UNSUPPORTED, "splat rows: too many rows for one launch");
    if (!nrows) return;
    ST_REQUIRE(out, ST_ERR_ARG, "NULL argument");
    KTimer kt(c, "wr.splat");
    const int wide = ((uintptr_t)out & 15) == 0;
    if (W.f32)
        hipLaunchKernelGGL(k_splat_rows<true>, dim3(grid_for(nrows, 256)), dim3(256), 0, c->stream, W.cols, row0, nrows,
                           out, wide);
    else
        hipLaunchKernelGGL(k_splat_rows<false>, dim3(grid_for(nrows, 256)), dim3(256), 0, c->stream, W.cols, row0, nrows,
                           out, wide);
    ST_LAUNCH_CHECK();
}

void spz_check(const WrTable &W, int fractional_bits) {
    ST_REQUIRE(fractional_bits >= 0 && fractional_bits <= 23, ST_ERR_ARG, "spz: fractional_bits must be 0..23");
    ST_REQUIRE(W.n < (1ull << 32), ST_ERR_UNSUPPORTED, "spz: the header holds fewer than 2^32 splats");
}

// rows [row0, row0 + nrows) into the planes, queued on the stream; adds to *d_clamped (device)
static void spz_planes_dev(st_ctx *c, const WrTable &W, int fractional_bits, uint64_t row0, uint64_t nrows,
                    uint8_t *const planes[6], unsigned long long *d_clamped) {
    spz_check(W, fractional_bits);
    ST_REQUIRE(row0 <= W.n && nrows <= W.n - row0, ST_ERR_ARG, "spz planes: rows outside the table");
    if (!nrows) return;
    SpzwArgs A{};
    for (int p = 0; p < 6; ++p) A.plane[p] = planes[p];
    A.pos_scale = (double)(1u << fractional_bits);
    A.row0 = row0;
    A.nrows = nrows;
    A.nsh = 3 * (uint32_t)W.C;
    KTimer kt(c, "wr.spz");
    const dim3 grid(grid_for(nrows, SPZW_TILE));
    const size_t lds = spzw_lds_words(A.nsh) * 4;
    if (W.f32)
        hipLaunchKernelGGL(k_spz_planes<true>, grid, dim3(SPZW_TILE), lds, c->stream, W.cols, A, d_clamped);
    else
        hipLaunchKernelGGL(k_spz_planes<false>, grid, dim3(SPZW_TILE), lds, c->stream, W.cols, A, d_clamped);
    ST_LAUNCH_CHECK();
}

// the clamp counter: a device word zeroed on the stream before the launches that add to it
static unsigned long long *clamp_counter(st_ctx *c) {
    auto *d = wsT<unsigned long long>(c, "wr.clamped", 1);
    ST_HIP(hipMemsetAsync(d, 0, 8, c->stream));
    return d;
}
static uint64_t clamp_read(st_ctx *c, const unsigned long long *d) {
    auto *h = static_cast<unsigned long long *>(pinned_slot(c, "wr.clamped", 16));
    ST_HIP(hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    return *h;
}

// the same with the count read back (waits for the stream)
static uint64_t spz_planes_count_dev(st_ctx *c, const WrTable &W, int fractional_bits, uint64_t row0, uint64_t nrows,
                              uint8_t *const planes[6]) {
    unsigned long long *d = clamp_counter(c);
    spz_planes_dev(c, W, fractional_bits, row0, nrows, planes, d);
    return clamp_read(c, d);
}

uint64_t spz_image_dev(st_ctx *c, const WrTable &W, int fractional_bits, uint8_t *out, uint64_t *clamped) {
    spz_check(W, fractional_bits);
    const uint64_t n = W.n, size = spz_image_size(n, W.C);
    uint8_t head[16];
    spz_header(n, W.C, fractional_bits, head);
    ST_HIP(hipMemcpyAsync(out, head, 16, hipMemcpyHostToDevice, c->stream));
    uint8_t *planes[6];
    uint64_t off = 16;
    const uint64_t per[6] = {9, 1, 3, 3, 3, 3 * (uint64_t)W.C};
    for (int p = 0; p < 6; ++p) {
        planes[p] = out + off;
        off += n * per[p];
    }
    const uint64_t cl = spz_planes_count_dev(c, W, fractional_bits, 0, n, planes);  // (waits: head is on the stack)
    if (clamped) *clamped = cl;
    return size;
}

}  // namespace st

using namespace st;

extern "C" {

uint64_t st_spz_image_size(uint64_t n, int32_t sh_coeffs) { return spz_image_size(n, sh_coeffs); }

int st_dev_splat_rows(st_ctx *c, const st_ttable *t, uint64_t row0, uint64_t nrows, uint8_t *dev_rows) {
    return guard([&] {
        ST_REQUIRE(c && t, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, false, "splat rows");
        use_device(c);
        splat_rows_dev(c, W, row0, nrows, dev_rows);
    });
}

int st_dev_spz_planes(st_ctx *c, const st_ttable *t, int32_t fractional_bits, uint64_t row0, uint64_t nrows,
                      uint8_t *const planes[6], uint64_t *out_clamped) {
    return guard([&] {
        ST_REQUIRE(c && t && planes, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, true, "spz planes");
        spz_check(W, fractional_bits);
        ST_REQUIRE(row0 <= W.n && nrows <= W.n - row0, ST_ERR_ARG, "spz planes: rows outside the table");
        use_device(c);
        const uint64_t cl = spz_planes_count_dev(c, W, fractional_bits, row0, nrows, planes);
        if (out_clamped) *out_clamped = cl;
    });
}

int st_dev_spz_image(st_ctx *c, const st_ttable *t, int32_t fractional_bits, uint8_t *dev_out, uint64_t cap,
                     uint64_t *size, uint64_t *out_clamped) {
    return guard([&] {
        ST_REQUIRE(c && t && size, ST_ERR_ARG, "NULL argument");
        const WrTable W = wr_table(t, true, "spz image");
        spz_check(W, fractional_bits);
        *size = spz_image_size(W.n, W.C);
        ST_REQUIRE(*size <= cap, ST_ERR_ARG, "spz image: the output buffer is too small");
        ST_REQUIRE(dev_out, ST_ERR_ARG, "NULL argument");
        use_device(c);
        spz_image_dev(c, W, fractional_bits, dev_out, out_clamped);
    });
}

}  // extern "C"
