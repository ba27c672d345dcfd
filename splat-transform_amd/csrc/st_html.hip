// st_html.hip -- writeHtml (writers/write-html.ts:10-59): the viewer page with the scene embedded as
// fetch("data:application/ply;base64,...") whose payload is the compressed-PLY file.
//
// k_base64  the RFC 4648 text of a virtual byte stream -- up to four (device pointer, length)
//           segments back to back, never copied together -- written contiguously.  A workgroup
//           takes B64_SPAN = 256 x 12 consecutive stream bytes.  They come into LDS with aligned
//           4-byte loads: every segment's piece of the span gets a region of its own whose first
//           byte sits at the piece's source address modulo 4, so lane i of the copy loads the i-th
//           aligned word that holds a byte of the piece and stores it as it is.  A lane then
//           owns 12 stream bytes: four LDS words (stride 3 words across lanes: no bank conflict)
//           funnel-shifted into three, 16 characters by 4-wide SWAR arithmetic (no table), one
//           16-byte store -- a wavefront writes 1 KiB contiguously.  A lane whose 12 bytes cross a
//           segment boundary (or several: segments may be shorter than 12 bytes, or empty) and the
//           lane holding the stream's last partial group gather their bytes one by one from LDS
//           and store whole 4-character groups, '=' padded.
// html_parts  the page text around the payload, on the host: pad(), JSON.stringify of the settings
//           and String.prototype.replace with a string pattern, on UTF-8 bytes.
#include <cmath>
#include <cstring>

#include "st_internal.h"
#include "st_numfmt.h"

namespace st {
namespace {

constexpr uint32_t B64_LANE = 12, B64_SPAN = 256 * B64_LANE;
// a piece's region: up to 3 bytes of lead, its bytes, rounded up to a word -- at most 4 pieces in a
// span; one more word because an aligned lane reads a fourth word it does not use
constexpr uint32_t B64_LDS_WORDS = (B64_SPAN + B64_MAX_SEGS * 6) / 4 + 2;

struct B64Stream {
    const uint8_t *ptr[B64_MAX_SEGS];
    uint64_t start[B64_MAX_SEGS + 1];  // the segments' first bytes in the stream; [4] = its length
};

// the segment that holds stream byte x (< start[4]): the last one that starts at or before it
__device__ inline uint32_t seg_of(const B64Stream &sg, uint64_t x) {
    return (uint32_t)(x >= sg.start[1]) + (uint32_t)(x >= sg.start[2]) + (uint32_t)(x >= sg.start[3]);
}

__device__ inline int32_t pick4(uint32_t s, const int32_t (&v)[B64_MAX_SEGS]) {
    return s == 0 ? v[0] : s == 1 ? v[1] : s == 2 ? v[2] : v[3];
}

// four 6-bit values, one per byte -> their characters: 'A' + x, then +6 from 26 ('a'), -75 from 52
// ('0'), -15 at 62 ('+'), +3 at 63 ('/').  x + (128 - k) has bit 7 set iff x >= k; t - (t >> 7)
// turns those bits into 0x7f byte masks.  Every final byte is a character, so the dword sums are exact.
__device__ inline uint32_t b64_chars(uint32_t x) {
    const auto mask = [](uint32_t v, uint32_t bias) {
        const uint32_t t = (v + bias) & 0x80808080u;
        return t - (t >> 7);
    };
    uint32_t c = x + 0x41414141u;
    c += mask(x, 0x66666666u) & 0x06060606u;
    c -= mask(x, 0x4c4c4c4cu) & 0x4b4b4b4bu;
    c -= mask(x, 0x42424242u) & 0x0f0f0f0fu;
    c += mask(x, 0x41414141u) & 0x03030303u;
    return c;
}

// three bytes given as (b0 << 16) | (b1 << 8) | b2 -> four characters, the first in the low byte
__device__ inline uint32_t b64_group(uint32_t v) {
    const uint32_t x = ((v >> 18) & 0x3fu) | ((v >> 4) & 0x3f00u) | ((v << 10) & 0x3f0000u) | ((v << 24) & 0x3f000000u);
    return b64_chars(x);
}

typedef uint32_t b64_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// the text of stream bytes [byte0, byte0 + nbytes) at out (4-byte aligned): byte0 % 3 == 0, and
// nbytes % 3 != 0 only when the range ends the stream (the host checks both)
__global__ __launch_bounds__(256) void k_base64(B64Stream sg, uint64_t byte0, uint64_t nbytes,
                                                uint8_t *__restrict__ out) {
    __shared__ uint32_t lds32[B64_LDS_WORDS];
    const uint8_t *lds8 = (const uint8_t *)lds32;
    const uint64_t rel0 = (uint64_t)blockIdx.x * B64_SPAN;  // the span's first byte in the range
    const uint64_t s0 = byte0 + rel0;                       // ... and in the stream
    const uint64_t left = nbytes - rel0;
    const uint32_t span = left < B64_SPAN ? (uint32_t)left : B64_SPAN;
    // image[rel[s] + i] = stream byte s0 + i wherever that byte is segment s's
    int32_t rel[B64_MAX_SEGS];
    uint32_t w = 0;
#pragma unroll
    for (int s = 0; s < B64_MAX_SEGS; ++s) {
        const uint64_t lo = sg.start[s] > s0 ? sg.start[s] : s0;
        const uint64_t hi = sg.start[s + 1] < s0 + span ? sg.start[s + 1] : s0 + span;
        rel[s] = 0;
        if (lo < hi) {  // (uniform over the workgroup)
            const uint8_t *src = sg.ptr[s] + (lo - sg.start[s]);
            const uint32_t lead = (uint32_t)((uintptr_t)src & 3), len = (uint32_t)(hi - lo);
            const uint32_t words = (lead + len + 3) >> 2;  // each holds a byte of the piece
            const uint32_t *src32 = (const uint32_t *)(src - lead);
#pragma unroll 4
            for (uint32_t i = threadIdx.x; i < words; i += 256) lds32[w + i] = src32[i];  // (at most 4 turns)
            rel[s] = (int32_t)(w * 4 + lead) - (int32_t)(lo - s0);
            w += words;
        }
    }
    __syncthreads();
    const uint32_t at = threadIdx.x * B64_LANE;
    if (at >= span) return;
    const uint32_t n = span - at < B64_LANE ? span - at : B64_LANE;
    const uint64_t x0 = s0 + at;
    const uint32_t sa = seg_of(sg, x0);
    uint32_t d0, d1, d2;  // the lane's bytes 0-3, 4-7, 8-11
    if (n == B64_LANE && seg_of(sg, x0 + (B64_LANE - 1)) == sa) {
        const uint32_t a = (uint32_t)(pick4(sa, rel) + (int32_t)at);
        const uint32_t *p = lds32 + (a >> 2);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
        d0 = __builtin_amdgcn_alignbyte(w1, w0, a & 3);
        d1 = __builtin_amdgcn_alignbyte(w2, w1, a & 3);
        d2 = __builtin_amdgcn_alignbyte(w3, w2, a & 3);
    } else {
        d0 = d1 = d2 = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t b = lds8[(uint32_t)(pick4(seg_of(sg, x0 + j), rel) + (int32_t)(at + j))];
            const uint32_t v = b << (8 * (j & 3));
            if (j < 4) d0 |= v;
            else if (j < 8) d1 |= v;
            else d2 |= v;
        }
    }
    // byte triples, big-endian: (0 1 2) (3 4 5) (6 7 8) (9 10 11)
    uint32_t g[4];
    g[0] = b64_group(__builtin_bswap32(d0) >> 8);
    g[1] = b64_group(__builtin_bswap32(__builtin_amdgcn_alignbyte(d1, d0, 3)) >> 8);
    g[2] = b64_group(__builtin_bswap32(__builtin_amdgcn_alignbyte(d2, d1, 2)) >> 8);
    g[3] = b64_group(__builtin_bswap32(d2 >> 8) >> 8);
    uint32_t *dst = (uint32_t *)(out + (rel0 / 3) * 4 + (uint64_t)threadIdx.x * 16);
    if (n == B64_LANE) {
        b64_u32x4 v;
        v.x = g[0], v.y = g[1], v.z = g[2], v.w = g[3];
        *(b64_u32x4 *)dst = v;
        return;
    }
    // the stream's end: whole groups, the last one padded
    const uint32_t groups = (n + 2) / 3, rem = n % 3;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (k >= groups) break;
        uint32_t v = g[k];
        if (k + 1 == groups && rem == 1) v = (v & 0x0000ffffu) | 0x3d3d0000u;
        if (k + 1 == groups && rem == 2) v = (v & 0x00ffffffu) | 0x3d000000u;
        dst[k] = v;
    }
}

// ---- the page text (host) ---------------------------------------------------------------------------

// String.prototype.replace(pattern, replacement) with a string pattern (ECMA-262 GetSubstitution
// without captures): the first occurrence only; $$ $& $` $' substitute, any other '$' stays
std::string js_replace(const std::string &text, const std::string &pattern, const std::string &repl) {
    const size_t at = text.find(pattern);
    if (at == std::string::npos) return text;
    const size_t tail = at + pattern.size();
    std::string out(text, 0, at);
    for (size_t i = 0; i < repl.size(); ++i) {
        const char nx = repl[i] == '$' && i + 1 < repl.size() ? repl[i + 1] : 0;
        if (nx == '$') out += '$', ++i;
        else if (nx == '&') out += pattern, ++i;
        else if (nx == '`') out.append(text, 0, at), ++i;
        else if (nx == '\'') out.append(text, tail, std::string::npos), ++i;
        else out += repl[i];
    }
    out.append(text, tail, std::string::npos);
    return out;
}

// write-html.ts:11-14: `spaces` blanks before every '\n'-separated line, empty ones too
std::string pad_lines(const std::string &text, int spaces) {
    const std::string blank(spaces, ' ');
    std::string out = blank;
    for (const char ch : text) {
        out += ch;
        if (ch == '\n') out += blank;
    }
    return out;
}

// JSON.stringify of a number: Number::toString, null when not finite
std::string json_number(double v) {
    if (!std::isfinite(v)) return "null";
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    const numfmt::Dec d = numfmt::dec_f64_bits(bits, numfmt_host_table());
    std::string s(numfmt::dec_len(d), '\0');
    numfmt::dec_put(d, &s[0]);
    return s;
}

std::string json_vec3(const double *v) {
    return "[" + json_number(v[0]) + "," + json_number(v[1]) + "," + json_number(v[2]) + "]";
}

char *malloc_copy(const std::string &s) {
    char *p = static_cast<char *>(std::malloc(s.size() + 1));
    ST_REQUIRE(p, ST_ERR_NOMEM, "html parts: allocation failed");
    std::memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

}  // namespace

uint64_t base64_size(uint64_t nbytes) { return nbytes / 3 * 4 + (nbytes % 3 ? 4 : 0); }

uint64_t base64_check(const st_bytes_seg *segs, int nseg, uint64_t byte0, uint64_t nbytes) {
    ST_REQUIRE(nseg >= 0 && nseg <= B64_MAX_SEGS && (segs || nseg == 0), ST_ERR_ARG, "base64: at most four segments");
    uint64_t total = 0;
    for (int s = 0; s < nseg; ++s) {
        ST_REQUIRE(segs[s].ptr || !segs[s].len, ST_ERR_ARG, "base64: NULL segment");
        ST_REQUIRE(segs[s].len <= UINT64_MAX / 2 - total, ST_ERR_ARG, "base64: the stream is too long");
        total += segs[s].len;
    }
    ST_REQUIRE(byte0 % 3 == 0, ST_ERR_ARG, "base64: a range starts at a multiple of 3");
    ST_REQUIRE(byte0 <= total && nbytes <= total - byte0, ST_ERR_ARG, "base64: range outside the stream");
    ST_REQUIRE(nbytes % 3 == 0 || byte0 + nbytes == total, ST_ERR_ARG,
               "base64: only a range that ends the stream may have a partial last group");
    return base64_size(nbytes);
}

void base64_dev(st_ctx *c, const st_bytes_seg *segs, int nseg, uint64_t byte0, uint64_t nbytes, uint8_t *out) {
    base64_check(segs, nseg, byte0, nbytes);
    ST_REQUIRE(((uintptr_t)out & 3) == 0, ST_ERR_ARG, "base64: output must be 4-byte aligned");
    if (!nbytes) return;
    ST_REQUIRE(out, ST_ERR_ARG, "NULL argument");
    const uint64_t blocks = (nbytes + B64_SPAN - 1) / B64_SPAN;
    ST_REQUIRE(blocks <= 0x7fffffffull, ST_ERR_UNSUPPORTED, "base64: range too long for one launch");
    B64Stream sg{};
    uint64_t run = 0;
    for (int s = 0; s < B64_MAX_SEGS; ++s) {
        sg.ptr[s] = s < nseg ? segs[s].ptr : nullptr;
        sg.start[s] = run;
        run += s < nseg ? segs[s].len : 0;
    }
    sg.start[B64_MAX_SEGS] = run;
    KTimer kt(c, "base64");
    hipLaunchKernelGGL(k_base64, dim3((unsigned)blocks), dim3(256), 0, c->stream, sg, byte0, nbytes, out);
    ST_LAUNCH_CHECK();
}

HtmlParts html_parts(const char *html, const char *css, const char *js, const double *camera, const double *target) {
    ST_REQUIRE(html && css && js && camera && target, ST_ERR_ARG, "html parts: NULL argument");
    // write-html.ts:24-36; animTrack is undefined, which JSON.stringify leaves out
    const std::string settings = "{\"camera\":{\"fov\":50,\"position\":" + json_vec3(camera) + ",\"target\":" +
                                 json_vec3(target) +
                                 ",\"startAnim\":\"none\"},\"background\":{\"color\":[0.4,0.4,0.4]},\"animTracks\":[]}";
    std::string t = js_replace(html, "<link rel=\"stylesheet\" href=\"./index.css\">",
                               "<style>\n" + pad_lines(css, 12) + "\n        </style>");
    t = js_replace(t, "<script type=\"module\" src=\"./index.js\"></script>",
                   "<script type=\"module\">\n" + pad_lines(js, 12) + "\n        </script>");
    t = js_replace(t, "settings: fetch(settingsUrl).then(response => response.json())", "settings: " + settings);
    // the fourth replacement holds no '$': the page splits around the payload
    static const std::string content = "fetch(contentUrl)";
    HtmlParts p;
    const size_t at = t.find(content);
    p.embeds = at != std::string::npos;
    if (!p.embeds) {
        p.prefix = std::move(t);
        return p;
    }
    p.prefix = t.substr(0, at) + "fetch(\"data:application/ply;base64,";
    p.suffix = "\")" + t.substr(at + content.size());
    return p;
}

}  // namespace st

using namespace st;

extern "C" {

uint64_t st_base64_size(uint64_t nbytes) { return base64_size(nbytes); }

int st_dev_base64(st_ctx *c, const st_bytes_seg *segs, int32_t nseg, uint64_t byte0, uint64_t nbytes, uint8_t *dev_out,
                  uint64_t cap, uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(c && size, ST_ERR_ARG, "NULL argument");
        *size = base64_size(nbytes);
        base64_check(segs, nseg, byte0, nbytes);
        ST_REQUIRE(((uintptr_t)dev_out & 3) == 0, ST_ERR_ARG, "base64: output must be 4-byte aligned");
        ST_REQUIRE(*size <= cap, ST_ERR_ARG, "base64: the output buffer is too small");
        use_device(c);
        base64_dev(c, segs, nseg, byte0, nbytes, dev_out);
    });
}

int st_html_parts(const char *html, const char *css, const char *js, const double *camera, const double *target,
                  char **prefix, uint64_t *prefix_size, char **suffix, uint64_t *suffix_size, int32_t *embeds) {
    return guard([&] {
        ST_REQUIRE(prefix && prefix_size && suffix && suffix_size && embeds, ST_ERR_ARG, "NULL argument");
        const HtmlParts p = html_parts(html, css, js, camera, target);
        char *a = malloc_copy(p.prefix);
        char *b = static_cast<char *>(std::malloc(p.suffix.size() + 1));
        if (!b) std::free(a);
        ST_REQUIRE(b, ST_ERR_NOMEM, "html parts: allocation failed");
        std::memcpy(b, p.suffix.c_str(), p.suffix.size() + 1);
        *prefix = a, *prefix_size = p.prefix.size();
        *suffix = b, *suffix_size = p.suffix.size();
        *embeds = p.embeds ? 1 : 0;
    });
}

}  // extern "C"
