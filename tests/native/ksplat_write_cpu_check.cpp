// TEST INFRASTRUCTURE ONLY: the .ksplat writer's __host__ __device__ functions run on the host.
//
// This program includes the product sources (st_writers.hip for wr_table, st_ksplat_write.hip and
// through it st_ksplat_encode.h), stands in for the few runtime pieces they link against (never
// called here) and, on the CPU: picks the columns, checks the parameters (ksplat_params), writes
// the two headers (ksplat_headers), encodes every record through a grid read from a file
// (ksplat_encode) and evaluates the grid functions (ks_cell, ks_centre) for every row.  The test
// (tests/test_write_ksplat_cpu.py) compares all of it byte for byte with the numpy restatement.
//
//   ksplat_write_cpu_check <mode> <degree> <sh_min> <sh_max> <block> <quant> <table> <grid> <out> <public>
//
// public 1: block goes through the public writer's check (ksplat_params); 0: it is a file's own.
//
// table: u64 n, u32 ncol, u32 0, then per column u32 type (ST_PLY_*) and a 28-byte NUL-padded name,
// then the columns' elements one column after another.
// grid:  u64 nrec, u64 nbuckets, u64 F, u64 P, f64 lo[3], then u32 order[nrec], u32 bucket[nrec],
// f32 centres[3 * nbuckets].
// out:   the 5120 header bytes, nrec records, then per table row u64 key, u32 clamped values and
// f32 centre[3] of its cell.  Prints "OK <n> <file sh_coeffs>" or "ERR <status> <message>".
// Every column and table sits in an allocation of exactly its bytes: a read past one is a heap
// overflow a sanitizer build of this program reports.
#include "../../splat-transform_amd/csrc/st_writers.hip"
#include "../../splat-transform_amd/csrc/st_ksplat_write.hip"

#include <cstdio>

namespace st {
void set_last_error(const std::string &) {}
bool g_sync_check = false;
KTimer::KTimer(st_ctx *ctx, const char *nm, hipStream_t stream) : c(ctx), name(nm), s(stream) {}
KTimer::~KTimer() {}
void use_device(st_ctx *) {}
void *Workspace::get(const std::string &, size_t) { return nullptr; }
void *pinned_slot(st_ctx *, const std::string &, size_t) { return nullptr; }
void scan_u32(st_ctx *, const uint32_t *, uint32_t *, uint64_t, uint32_t *) {}
void radix_sort_u64(st_ctx *, uint64_t *, uint32_t *, uint64_t, int, int, const std::string &) {}
int type_size(int32_t type) {
    switch (type) {
        case ST_PLY_CHAR: case ST_PLY_UCHAR: return 1;
        case ST_PLY_SHORT: case ST_PLY_USHORT: return 2;
        case ST_PLY_INT: case ST_PLY_UINT: case ST_PLY_FLOAT: return 4;
        case ST_PLY_DOUBLE: return 8;
        default: return 0;
    }
}
int band_coeffs(const std::function<bool(const char *)> &has) {
    int first_missing = -1;
    for (int i = 0; i < 45 && first_missing < 0; ++i)
        if (!has(("f_rest_" + std::to_string(i)).c_str())) first_missing = i;
    return first_missing == 9 ? 3 : first_missing == 24 ? 8 : first_missing == -1 ? 15 : 0;
}
}  // namespace st

using namespace st;

template <typename T>
static T *read_exact(FILE *f, size_t count) {
    T *p = static_cast<T *>(std::malloc(count * sizeof(T) ? count * sizeof(T) : 1));
    if (count && std::fread(p, sizeof(T), count, f) != count) std::exit(2);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 11) return 2;
    const bool is_public = std::atoi(argv[10]) != 0;
    const int mode = std::atoi(argv[1]), degree = std::atoi(argv[2]);
    const float sh_min = (float)std::atof(argv[3]), sh_max = (float)std::atof(argv[4]);
    const float block = (float)std::atof(argv[5]);
    const unsigned long quant = std::strtoul(argv[6], nullptr, 10);
    FILE *f = std::fopen(argv[7], "rb");
    if (!f) return 2;
    uint64_t n = 0;
    uint32_t ncol = 0, zero = 0;
    if (std::fread(&n, 8, 1, f) != 1 || std::fread(&ncol, 4, 1, f) != 1 || std::fread(&zero, 4, 1, f) != 1) return 2;
    std::vector<int32_t> types(ncol);
    std::vector<std::string> names(ncol);
    for (uint32_t i = 0; i < ncol; ++i) {
        char nm[29] = {0};
        if (std::fread(&types[i], 4, 1, f) != 1 || std::fread(nm, 28, 1, f) != 1) return 2;
        names[i] = nm;
    }
    std::vector<void *> cols(ncol, nullptr);
    for (uint32_t i = 0; i < ncol; ++i) cols[i] = read_exact<uint8_t>(f, n * (size_t)type_size(types[i]));
    std::fclose(f);
    f = std::fopen(argv[8], "rb");
    if (!f) return 2;
    uint64_t g[4];
    double lo[3];
    if (std::fread(g, 8, 4, f) != 4 || std::fread(lo, 8, 3, f) != 3) return 2;
    const uint64_t nrec = g[0], nbuckets = g[1];
    uint32_t *order = read_exact<uint32_t>(f, nrec), *bucket = read_exact<uint32_t>(f, nrec);
    float *centres = read_exact<float>(f, 3 * nbuckets);
    std::fclose(f);

    std::vector<const char *> cn;
    for (auto &s : names) cn.push_back(s.c_str());
    const st_ttable t{n, (int32_t)ncol, cn.data(), types.data(), cols.data()};
    std::vector<uint8_t> out;
    int c_out = 0;
    int rc = 0;
    try {
        const WrTable W = wr_table(&t, true, "ksplat image");
        // the public writer's checks; the grid's own block and range are the file's
        const KswParams P = ksplat_params(W, mode, degree, is_public ? (double)block : 5.0, sh_min, sh_max);
        c_out = P.c_out;
        KswParams H = P;
        H.B = block;
        const uint32_t stride = ksplat_stride(mode, c_out);
        out.resize(5120 + nrec * stride + n * 24);
        ksplat_headers(n, H, g[2], g[3], out.data());
        KsRecArgs A{};
        A.ps = (double)block / 2.0 / (double)quant;
        A.range = (double)quant;
        A.sh_lo = (double)P.sh_min;
        A.sh_span = (double)P.sh_max - (double)P.sh_min;
        A.sh_fast = ks_sh8_fast((double)P.sh_min, (double)P.sh_max);
        A.mode = mode, A.c_src = W.C, A.c_out = c_out;
        for (uint64_t r = 0; r < nrec; ++r) {
            if (order[r] >= n || (mode != 0 && bucket[r] >= nbuckets)) return 2;
            uint8_t *rec = out.data() + 5120 + r * stride;
            const float *centre = mode != 0 ? centres + 3 * (uint64_t)bucket[r] : nullptr;
            if (W.f32) ksplat_encode<true>(W.cols, A, order[r], centre, rec);
            else ksplat_encode<false>(W.cols, A, order[r], centre, rec);
        }
        uint8_t *cells = out.data() + 5120 + nrec * stride;
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t key = 0;
            uint32_t cl = 0;
            float centre[3];
            for (int a = 0; a < 3; ++a) {
                bool clamped;
                const uint32_t cell = ks_cell(ta_load(W.cols.c[a].p, W.cols.c[a].t, i), lo[a], (double)block, &clamped);
                cl += clamped;
                key |= (uint64_t)cell << (21 * a);
                centre[a] = ks_centre(lo[a], cell, (double)block);
            }
            std::memcpy(cells + 24 * i, &key, 8);
            std::memcpy(cells + 24 * i + 8, &cl, 4);
            std::memcpy(cells + 24 * i + 12, centre, 12);
        }
    } catch (const Error &e) {
        std::printf("ERR %d %s\n", e.code, e.what());
        rc = 1;
    }
    if (!rc) {
        FILE *o = std::fopen(argv[9], "wb");
        if (!o) return 2;
        std::fwrite(out.data(), 1, out.size(), o);
        std::fclose(o);
        std::printf("OK %llu %d\n", (unsigned long long)n, c_out);
    }
    for (void *p : cols) std::free(p);
    std::free(order), std::free(bucket), std::free(centres);
    return 0;
}
