// summary_cpu_check -- the column summary's serial host form (splat-transform_amd/csrc/st_summary.h:
// summarize_host, the functions the kernels and the library's epilogue call, and summary_text) on
// the host, for tests/test_summary_cpu.py.  Build with -ffp-contract=off, as the library is.
//
//   summary_cpu_check summary <in> <out> <exact 0|1> <flush>
//       in: per column an int32 st_ply_type code, a uint64 count, then the elements as stored.
//       out: one st_col_summary (80 bytes) per column.  stdout: "C <column> <fast 0|1>" per column.
//   summary_cpu_check text <names> <summaries> <out>
//       names: one per line; summaries: st_col_summary records; out: st_summary_text's bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../splat-transform_amd/csrc/st_summary.h"

static std::vector<uint8_t> slurp(const char *path, bool *ok) {
    std::vector<uint8_t> v;
    *ok = false;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    *ok = !n || std::fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return v;
}

static bool spill(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    static_assert(sizeof(st_col_summary) == 80, "st_col_summary is ten 8-byte fields");
    bool ok;
    if (argc == 6 && !std::strcmp(argv[1], "summary")) {
        const std::vector<uint8_t> in = slurp(argv[2], &ok);
        if (!ok) return 2;
        const bool exact = std::atoi(argv[4]) != 0;
        const uint64_t flush = std::strtoull(argv[5], nullptr, 10);
        if (flush < 1 || flush > st::sm::FLUSH_MAX) return 2;
        std::vector<st_col_summary> out;
        size_t at = 0;
        while (at < in.size()) {
            if (in.size() - at < 12) return 2;
            int32_t type;
            uint64_t count;
            std::memcpy(&type, in.data() + at, 4);
            std::memcpy(&count, in.data() + at + 4, 8);
            at += 12;
            const int z = st::sm::elem_size(type);
            if (!z || (in.size() - at) / (size_t)z < count) return 2;
            // a copy of exactly the column's bytes: a read past either end is the sanitizer's to find
            std::vector<uint8_t> col(in.begin() + (long)at, in.begin() + (long)(at + count * (size_t)z));
            at += count * (size_t)z;
            st_col_summary s;
            bool fast = false;
            st::sm::summarize_host(type, col.data(), count, exact, flush, &s, &fast);
            std::printf("C %zu %d\n", out.size(), fast ? 1 : 0);
            out.push_back(s);
        }
        return spill(argv[3], out.data(), out.size() * sizeof(st_col_summary)) ? 0 : 2;
    }
    if (argc == 5 && !std::strcmp(argv[1], "text")) {
        const std::vector<uint8_t> nb = slurp(argv[2], &ok);
        if (!ok) return 2;
        const std::vector<uint8_t> sb = slurp(argv[3], &ok);
        if (!ok) return 2;
        std::vector<std::string> names;
        std::string cur;
        for (uint8_t ch : nb) {
            if (ch == '\n') names.push_back(cur), cur.clear();
            else cur.push_back((char)ch);
        }
        if (sb.size() != names.size() * sizeof(st_col_summary) || names.empty()) return 2;
        std::vector<st_col_summary> s(names.size());
        std::memcpy(s.data(), sb.data(), sb.size());
        std::vector<const char *> np;
        for (const std::string &n : names) np.push_back(n.c_str());
        std::vector<uint64_t> tab(2 * st::numfmt::POW10_ENTRIES);
        st::numfmt::numfmt_build_table(tab.data());
        const st_ttable t{0, (int32_t)names.size(), np.data(), nullptr, nullptr};
        const std::string text = st::sm::summary_text(&t, s.data(), tab.data());
        return spill(argv[4], text.data(), text.size()) ? 0 : 2;
    }
    std::fprintf(stderr, "usage: summary_cpu_check summary <in> <out> <exact> <flush> | text <names> <summaries> <out>\n");
    return 2;
}
