// st_sog_read.hip -- the .sog reader: textures -> float32 columns on the device.
//
// The reference writes SOG (write-sog.ts:110-370) and cannot read it back; the decode rules
// here are this project's own, the exact inverses of the writer's quantisers in JS-number
// arithmetic (include/st_abi.h spells them out; tests/sog_read_ref.py restates them in numpy).
//
//   k_sog_decode   one thread per splat i < count; texel i of each per-splat texture is one
//                  coalesced 4-byte load, every column store has consecutive lanes on consecutive
//                  rows.  The three 256-entry codebooks sit in LDS.  The SH palette row of a splat
//                  is C contiguous texels of shN_centroids (texel label * C + j: row label >> 6,
//                  column (label & 63) * C + j of a 64 * C wide texture), gathered per thread; a
//                  label >= palette_size reads the last palette row instead (the index is bounded
//                  before the load), writes zeros and bumps one counter.
//                  read 20 (28 + 4 C with SH) B, write 56 + 12 C B per splat: 276 B at SH-3
//
// The host part: the archive's index (st_zip_index.h), the seven names, st_webp_info,
// sog_read_layout -- the only gate before the launch: after it no texel index leaves its texture
// -- then the textures decoded on one host thread each (at most seven, never sized by the
// machine), each uploaded from its pinned slot as it finishes, and the kernel.
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "st_internal.h"
#include "st_jsmath.h"
#include "st_zip_index.h"

namespace st {
namespace {

constexpr int SR_SH_MAX = 45;
constexpr int SR_TILE = 256;
struct SrCols {
    float *c[14 + SR_SH_MAX];  // x y z scale_0..2 f_dc_0..2 opacity rot_0..3 f_rest_0..
};
struct SrPlan {
    const uint32_t *means_l, *means_u, *quats, *scales, *sh0, *labels, *centroids;
    const float *codebooks;  // scales, sh0, shN: 3 x 256 float32
    double mins[3], span[3];  // span = maxs - mins (a JS subtraction done on the host)
    uint64_t count;
    uint32_t C;        // SH coefficients per channel: 0, 3, 8, 15
    uint32_t palette;  // shN.count
};

__host__ __device__ inline int coeffs_of_bands(int bands) { return bands == 1 ? 3 : bands == 2 ? 8 : bands == 3 ? 15 : 0; }

// x, y or z from its 16-bit code
__host__ __device__ inline float sr_mean(uint32_t q, double mn, double span) {
    const double t = (double)q / 65535.0;
    const double m = js::x86_nan(span * t, js::isnan_(span));
    const double v = js::x86_nan(mn + m, js::isnan_(mn) || js::isnan_(m));
    if (js::isnan_(v)) return js::f32_store(v);  // Math.sign(NaN) * NaN: the NaN as it is
    return js::f32_store(js::sign_(v) * (js::exp(__builtin_fabs(v)) - 1.0));
}

__host__ __device__ inline void sr_quat(uint32_t texel, float out[4]) {
    const uint32_t tag = (texel >> 24) & 3u;
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = ((double)((texel >> (8 * k)) & 0xffu) / 255.0 - 0.5) * 1.4142135623730951;
    const double m = __builtin_sqrt(js::max_(0.0, 1.0 - (c[0] * c[0] + c[1] * c[1] + c[2] * c[2])));
    int k = 0;
    for (uint32_t j = 0; j < 4; ++j) out[j] = js::f32_store(j == tag ? m : c[k++]);
}

__host__ __device__ inline float sr_opacity(uint32_t byte) {
    const double p = (double)byte / 255.0;
    const double e = js::min_(1.0 - 1e-6, js::max_(1e-6, p));
    return js::f32_store(js::log(e / (1.0 - e)));
}

__global__ __launch_bounds__(SR_TILE) void k_sog_decode(SrPlan P, SrCols O, uint32_t *__restrict__ bad) {
    __shared__ float cb[3 * 256];
    for (uint32_t k = threadIdx.x; k < 3 * 256; k += SR_TILE) cb[k] = P.codebooks[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * SR_TILE + threadIdx.x;
    if (i >= P.count) return;
    const uint32_t ml = P.means_l[i], mu = P.means_u[i];
    for (int a = 0; a < 3; ++a) {
        const uint32_t q = ((ml >> (8 * a)) & 0xffu) | (((mu >> (8 * a)) & 0xffu) << 8);
        O.c[a][i] = sr_mean(q, P.mins[a], P.span[a]);
    }
    const uint32_t sc = P.scales[i], s0 = P.sh0[i];
    for (int k = 0; k < 3; ++k) O.c[3 + k][i] = cb[(sc >> (8 * k)) & 0xffu];
    for (int k = 0; k < 3; ++k) O.c[6 + k][i] = cb[256 + ((s0 >> (8 * k)) & 0xffu)];
    O.c[9][i] = sr_opacity(s0 >> 24);
    float r[4];
    sr_quat(P.quats[i], r);
    for (int k = 0; k < 4; ++k) O.c[10 + k][i] = r[k];
    if (P.C) {
        const uint32_t label = P.labels[i] & 0xffffu;  // R | G << 8
        const bool ok = label < P.palette;
        const uint32_t row = label < P.palette - 1 ? label : P.palette - 1;  // bounded before the load
        const uint32_t *t = P.centroids + (uint64_t)row * P.C;
        for (uint32_t j = 0; j < P.C; ++j) {
            const uint32_t texel = t[j];
            for (uint32_t ch = 0; ch < 3; ++ch)
                O.c[14 + j + ch * P.C][i] = ok ? cb[512 + ((texel >> (8 * ch)) & 0xffu)] : 0.0f;
        }
        if (!ok) atomicAdd(bad, 1u);
    }
}

// the checks of st_sog_read_layout; returns C
int sog_read_layout(const st_sog_meta &m, uint64_t count, const int32_t wh[7][2]) {
    ST_REQUIRE(count >= 1, ST_ERR_ARG, "sog: count must be at least 1");
    const int64_t w = wh[0][0], h = wh[0][1];
    ST_REQUIRE(w >= 1 && h >= 1 && w <= 16384 && h <= 16384, ST_ERR_ARG, "sog: texture size out of range");
    ST_REQUIRE(m.sh_bands >= 0 && m.sh_bands <= 3, ST_ERR_ARG, "sog: shN.bands must be 0..3");
    static const char *names[7] = {"means_l", "means_u", "quats", "scales", "sh0", "shN_centroids", "shN_labels"};
    for (int k = 0; k < 7; ++k) {
        if (k == 5 || (k == 6 && m.sh_bands == 0)) continue;
        if (wh[k][0] != w || wh[k][1] != h)
            throw Error(ST_ERR_ARG, std::string("sog: texture ") + names[k] + " is " + std::to_string(wh[k][0]) + " x " +
                                        std::to_string(wh[k][1]) + ", means_l is " + std::to_string(w) + " x " +
                                        std::to_string(h));
    }
    ST_REQUIRE(m.width == w && m.height == h, ST_ERR_ARG, "sog: meta width / height differ from the textures");
    ST_REQUIRE((uint64_t)(w * h) >= count, ST_ERR_ARG, "sog: the textures hold fewer texels than count");
    const int C = coeffs_of_bands(m.sh_bands);
    if (C) {
        ST_REQUIRE(m.palette_size >= 1 && m.palette_size <= 65536, ST_ERR_ARG, "sog: shN.count must be 1..65536");
        const int64_t cw = wh[5][0], chh = wh[5][1];
        ST_REQUIRE(cw == 64 * C, ST_ERR_ARG, "sog: shN_centroids must be 64 * coefficients texels wide");
        ST_REQUIRE(chh >= 1 && chh <= 16384 && 64 * chh >= m.palette_size, ST_ERR_ARG,
                   "sog: shN_centroids has fewer rows than shN.count needs");
        ST_REQUIRE(m.shn_width == cw && m.shn_height == chh, ST_ERR_ARG,
                   "sog: meta shn_width / shn_height differ from the texture");
    }
    return C;
}

void wh_of_meta(const st_sog_meta &m, int32_t wh[7][2]) {
    for (int k = 0; k < 7; ++k) wh[k][0] = m.width, wh[k][1] = m.height;
    wh[5][0] = m.shn_width, wh[5][1] = m.shn_height;
}

// queues the kernel; returns the device counter of labels outside the palette
uint32_t *sog_decode_launch(st_ctx *c, const st_sog_meta &m, uint64_t count, int C, const st_sog_textures &t,
                            float *const *cols) {
    SrCols O{};
    for (int k = 0; k < 14 + 3 * C; ++k) {
        ST_REQUIRE(cols[k], ST_ERR_ARG, "sog: NULL column");
        O.c[k] = cols[k];
    }
    const uint8_t *tex[7] = {t.means_l, t.means_u, t.quats, t.scales, t.sh0, t.shn_centroids, t.shn_labels};
    for (int k = 0; k < 7; ++k) {
        if (k >= 5 && !C) continue;
        ST_REQUIRE(tex[k], ST_ERR_ARG, "sog: NULL texture");
        ST_REQUIRE(((uintptr_t)tex[k] & 3) == 0, ST_ERR_ARG, "sog: textures must be 4-byte aligned");
    }
    // the codebooks and the zeroed counter: 3 x 256 floats + one word through a pinned slot (its
    // last word receives the counter back)
    float *h_cb = (float *)pinned_slot(c, "sogr.cb", 3 * 256 * 4 + 8);
    std::memcpy(h_cb, m.scales_codebook, 1024);
    std::memcpy(h_cb + 256, m.sh0_codebook, 1024);
    std::memcpy(h_cb + 512, m.shn_codebook, 1024);
    std::memset(h_cb + 768, 0, 4);
    float *d_cb = wsT<float>(c, "sogr.cb", 3 * 256 + 1);
    ST_HIP(hipMemcpyAsync(d_cb, h_cb, 3 * 256 * 4 + 4, hipMemcpyHostToDevice, c->stream));
    SrPlan P{};
    P.means_l = (const uint32_t *)t.means_l, P.means_u = (const uint32_t *)t.means_u;
    P.quats = (const uint32_t *)t.quats, P.scales = (const uint32_t *)t.scales, P.sh0 = (const uint32_t *)t.sh0;
    P.labels = C ? (const uint32_t *)t.shn_labels : nullptr;
    P.centroids = C ? (const uint32_t *)t.shn_centroids : nullptr;
    P.codebooks = d_cb;
    for (int a = 0; a < 3; ++a) {
        P.mins[a] = m.means_min[a];
        P.span[a] = m.means_max[a] - m.means_min[a];
    }
    P.count = count;
    P.C = (uint32_t)C;
    P.palette = C ? (uint32_t)m.palette_size : 1u;
    uint32_t *d_bad = (uint32_t *)(d_cb + 768);
    {
        KTimer kt(c, "rd.sog");
        hipLaunchKernelGGL(k_sog_decode, dim3(grid_for(count, SR_TILE)), dim3(SR_TILE), 0, c->stream, P, O, d_bad);
        ST_LAUNCH_CHECK();
    }
    return d_bad;
}

// waits for the kernel; throws when a label lay outside the palette
void sog_decode_finish(st_ctx *c, const uint32_t *d_bad) {
    uint32_t *h_bad = (uint32_t *)pinned_slot(c, "sogr.cb", 3 * 256 * 4 + 8) + 3 * 256 + 1;
    ST_HIP(hipMemcpyAsync(h_bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    if (*h_bad) throw Error(ST_ERR_ARG, std::to_string(*h_bad) + " shN labels outside the palette");
}

void sog_decode_dev(st_ctx *c, const st_sog_meta &m, uint64_t count, const st_sog_textures &t, float *const *cols) {
    int32_t wh[7][2];
    wh_of_meta(m, wh);
    const int C = sog_read_layout(m, count, wh);
    ST_REQUIRE(count < (1ull << 38), ST_ERR_UNSUPPORTED, "sog: too many rows for one launch");
    sog_decode_finish(c, sog_decode_launch(c, m, count, C, t, cols));
}

const char *const SR_FILES[7] = {"means_l.webp", "means_u.webp", "quats.webp",        "scales.webp",
                                 "sh0.webp",     "shN_centroids.webp", "shN_labels.webp"};

// a whole .sog in host memory -> device columns
void sog_read_dev(st_ctx *c, const uint8_t *data, uint64_t len, const st_sog_meta &meta_in, uint64_t count,
                  float *const *cols, const std::function<float *const *(int)> &cols_for) {
    std::vector<st_zip_entry> es;
    try {
        es = zip_index(data, len);
    } catch (const ZipIndexError &e) {
        throw Error(e.code, e.msg);
    }
    ST_REQUIRE(meta_in.sh_bands >= 0 && meta_in.sh_bands <= 3, ST_ERR_ARG, "sog: shN.bands must be 0..3");
    const int ntex = meta_in.sh_bands ? 7 : 5;
    const uint8_t *file[7] = {nullptr};
    uint64_t file_len[7] = {0};
    int32_t wh[7][2] = {{0, 0}};
    for (int k = 0; k < ntex; ++k) {
        const size_t nl = std::strlen(SR_FILES[k]);
        for (const st_zip_entry &e : es)  // the first entry of the name
            if (e.name_len == nl && std::memcmp(data + e.name_offset, SR_FILES[k], nl) == 0) {
                file[k] = data + e.offset;
                file_len[k] = e.size;
                break;
            }
        if (!file[k]) throw Error(ST_ERR_ARG, std::string("sog: the archive has no ") + SR_FILES[k]);
        const int rc = st_webp_info(file[k], file_len[k], &wh[k][0], &wh[k][1]);
        if (rc != ST_OK) throw Error(rc, std::string(SR_FILES[k]) + ": " + st_last_error());
    }
    st_sog_meta m = meta_in;
    m.width = wh[0][0], m.height = wh[0][1];
    m.shn_width = ntex == 7 ? wh[5][0] : 0, m.shn_height = ntex == 7 ? wh[5][1] : 0;
    const int C = sog_read_layout(m, count, wh);
    ST_REQUIRE(count < (1ull << 38), ST_ERR_UNSUPPORTED, "sog: too many rows for one launch");
    if (!cols) cols = cols_for(14 + 3 * C);

    // one host thread per texture decodes into its pinned slot; this thread uploads each as it
    // finishes (every HIP call stays on the caller's thread)
    uint8_t *host[7] = {nullptr}, *dev[7] = {nullptr};
    uint64_t bytes[7] = {0};
    for (int k = 0; k < ntex; ++k) {
        bytes[k] = (uint64_t)wh[k][0] * (uint64_t)wh[k][1] * 4;
        host[k] = (uint8_t *)pinned_slot(c, std::string("sogr.h") + std::to_string(k), bytes[k]);
        dev[k] = wsT<uint8_t>(c, std::string("sogr.t") + std::to_string(k), bytes[k]);
    }
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> done;  // textures in the order they finished
    int rcs[7] = {0};
    std::string errs[7];
    std::vector<std::thread> workers;
    for (int k = 0; k < ntex; ++k)
        workers.emplace_back([&, k] {
            rcs[k] = st_webp_decode_lossless(file[k], file_len[k], host[k], wh[k][0] * 4);
            if (rcs[k] != ST_OK) errs[k] = st_last_error();  // (thread-local: read on the worker)
            std::lock_guard<std::mutex> lk(mu);
            done.push_back(k);
            cv.notify_one();
        });
    int failed = -1;
    hipError_t copy_err = hipSuccess;
    for (int taken = 0; taken < ntex; ++taken) {
        int k;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return (int)done.size() > taken; });
            k = done[taken];
        }
        if (rcs[k] != ST_OK) {
            if (failed < 0) failed = k;
            continue;
        }
        if (failed < 0 && copy_err == hipSuccess)
            copy_err = hipMemcpyAsync(dev[k], host[k], bytes[k], hipMemcpyHostToDevice, c->stream);
    }
    for (std::thread &t : workers) t.join();
    if (failed >= 0) {
        (void)hipStreamSynchronize(c->stream);  // the pinned slots are still being read
        throw Error(rcs[failed], std::string(SR_FILES[failed]) + ": " + errs[failed]);
    }
    ST_HIP(copy_err);
    st_sog_textures t{};
    t.means_l = dev[0], t.means_u = dev[1], t.quats = dev[2], t.scales = dev[3], t.sh0 = dev[4];
    t.shn_centroids = dev[5], t.shn_labels = dev[6];
    sog_decode_finish(c, sog_decode_launch(c, m, count, C, t, cols));
}

}  // namespace
}  // namespace st

using namespace st;

extern "C" {

int st_sog_read_layout(const st_sog_meta *meta, uint64_t count, const int32_t tex_wh[7][2], uint64_t *n,
                       int32_t *nsh) {
    return guard([&] {
        ST_REQUIRE(meta && tex_wh && n && nsh, ST_ERR_ARG, "NULL argument");
        const int C = sog_read_layout(*meta, count, tex_wh);
        *n = count;
        *nsh = 3 * C;
    });
}

int st_dev_sog_decode(st_ctx *c, const st_sog_meta *meta, uint64_t count, const st_sog_textures *dev_tex,
                      float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && meta && dev_tex && cols, ST_ERR_ARG, "NULL argument");
        use_device(c);
        sog_decode_dev(c, *meta, count, *dev_tex, cols);
    });
}

int st_dev_sog_read(st_ctx *c, const uint8_t *data, uint64_t len, const st_sog_meta *meta, uint64_t count,
                    float *const *cols) {
    return guard([&] {
        ST_REQUIRE(c && data && meta && cols, ST_ERR_ARG, "NULL argument");
        use_device(c);
        sog_read_dev(c, data, len, *meta, count, cols, nullptr);
    });
}

int st_sog_read(st_ctx *c, const uint8_t *data, uint64_t len, const st_sog_meta *meta, uint64_t count,
                float *const *host_cols) {
    return guard([&] {
        ST_REQUIRE(c && data && meta && host_cols, ST_ERR_ARG, "NULL argument");
        use_device(c);
        std::vector<float *> d;
        sog_read_dev(c, data, len, *meta, count, nullptr, [&](int ncol) {
            d.resize((size_t)ncol);
            for (int k = 0; k < ncol; ++k) d[k] = wsT<float>(c, "rd.col" + std::to_string(k), count);
            return (float *const *)d.data();
        });
        std::vector<HostXfer> down;
        for (size_t k = 0; k < d.size(); ++k) {
            ST_REQUIRE(host_cols[k], ST_ERR_ARG, "NULL host column");
            down.push_back(HostXfer{host_cols[k], d[k], count * 4});
        }
        staged_d2h(c, down);
    });
}

}  // extern "C"
