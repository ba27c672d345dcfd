// TEST INFRASTRUCTURE ONLY: the .splat / .ksplat / .spz decoders of st_readers.hip run on the host.
//
// The decode functions are __host__ __device__, so this program includes the product source,
// stands in for the few runtime pieces it links against (never called here) and runs the layout
// call and the per-splat decode of one file on the CPU -- the arithmetic and the host-side walks
// checked against the reference's vectors without a GPU (tests/test_readers_cpu.py).
//
//   readers_cpu_check <splat|ksplat|spz> <input file> <output file>
//
// prints "OK <n> <nsh>" and writes the 14 + nsh float32 columns one after another, or prints
// "ERR <status> <message>" for an input the layout call rejects.  (.spz: the inflated stream.)
#include "../../splat-transform_amd/csrc/st_readers.hip"

#include <cstdio>

namespace st {
void set_last_error(const std::string &) {}
bool g_sync_check = false;
KTimer::KTimer(st_ctx *ctx, const char *nm, hipStream_t stream) : c(ctx), name(nm), s(stream) {}
KTimer::~KTimer() {}
void use_device(st_ctx *) {}
void staged_h2d(st_ctx *, const std::vector<HostXfer> &) {}
void staged_d2h(st_ctx *, const std::vector<HostXfer> &) {}
void *Workspace::get(const std::string &, size_t) { return nullptr; }
void stream_rows_dev(st_ctx *, int, uint64_t, uint64_t, uint64_t, uint32_t,
                     const std::function<void(const uint8_t *, uint64_t, uint64_t)> &, ChunkSink *, const char *) {}
}  // namespace st

using namespace st;

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string fmt = argv[1];
    std::vector<uint8_t> d;
    {
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        uint8_t b[65536];
        size_t r;
        while ((r = std::fread(b, 1, sizeof b, f)) > 0) d.insert(d.end(), b, b + r);
        std::fclose(f);
    }
    // exactly the file's bytes at a 4-byte aligned address (what the kernels are handed): a read
    // past them is a heap overflow a sanitizer build of this program reports
    uint8_t *buf = d.empty() ? nullptr : static_cast<uint8_t *>(std::malloc(d.size()));  // (16-byte aligned)
    if (!d.empty()) std::memcpy(buf, d.data(), d.size());
    const uint64_t len = d.size();
    uint64_t n = 0;
    int nsh = 0;
    std::vector<std::vector<float>> cols;
    RdCols C{};
    auto alloc = [&](int nc) {
        cols.assign(nc, std::vector<float>(n, 123.0f));
        for (int k = 0; k < nc; ++k) C.c[k] = cols[k].data();
    };
    try {
        if (fmt == "splat") {
            splat_layout(len, &n);
            alloc(14);
            for (uint64_t i = 0; i < n; ++i) {
                uint32_t w[8];
                std::memcpy(w, buf + 32 * i, 32);
                splat_decode(w, i, C);
            }
        } else if (fmt == "ksplat") {
            KsPlan P;
            ks_plan(buf, len, len, P);
            n = P.n;
            nsh = P.nsh;
            alloc(14 + nsh);
            std::vector<uint32_t> ends;
            for (size_t i = 0; i < P.sections.size(); ++i) {
                KsSection &S = P.sections[i];
                S.ends_at = (uint32_t)ends.size();
                if (S.mode != 0 && S.count > S.full_splats && P.partial_count[i])
                    ks_bucket_ends(S, (const uint32_t *)(buf + P.partial_off[i]), P.partial_count[i], ends);
                S.nends = (uint32_t)ends.size() - S.ends_at;
            }
            for (const KsSection &S : P.sections)
                for (uint32_t s = 0; s < S.count; ++s)
                    ks_decode(buf + S.data_off + (uint64_t)s * S.stride, s, S, (const uint32_t *)(buf + S.centres_off),
                              ends.data(), C);
        } else if (fmt == "spz") {
            SpzPlan P;
            spz_plan(buf, len, P);
            n = P.n;
            nsh = (int)P.nsh;
            alloc(14 + nsh);
            for (uint64_t s = 0; s < n; ++s)
                spz_decode(buf + P.pos + 9 * s, buf[P.alpha + s], buf + P.colour + 3 * s, buf + P.scale + 3 * s,
                           buf + P.rot + (P.version == 2 ? 3 * s : s), buf + P.sh + P.nsh * s, P, s, C);
        } else {
            return 2;
        }
    } catch (const Error &e) {
        std::printf("ERR %d %s\n", e.code, e.what());
        return 0;
    }
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    for (auto &c : cols) std::fwrite(c.data(), 4, n, o);
    std::fclose(o);
    std::printf("OK %llu %d\n", (unsigned long long)n, nsh);
    std::free(buf);
    return 0;
}
