// csv_cpu_check -- the CSV writer's number formatting (splat-transform_amd/csrc/st_numfmt.h, the
// functions k_csv_len / k_csv_rows call per cell) on the host, for tests/test_write_csv_cpu.py.
//
//   csv_cpu_check values <in> <text out> <len out>
//       in: int32 st_ply_type code, uint64 count, then the count elements as stored in a column.
//       text out: every element's text followed by '\n'; len out: every element's len() as a byte.
//       put() must write exactly len() bytes (the bytes around them are checked) -- exit 1 if not.
//   csv_cpu_check table <out>
//       the power-of-ten table as 617 x (high, low) uint64.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../splat-transform_amd/csrc/st_numfmt.h"

using namespace st::numfmt;

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear();
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
    std::vector<uint64_t> tab(2 * POW10_ENTRIES);
    numfmt_build_table(tab.data());
    if (argc == 3 && !std::strcmp(argv[1], "table"))
        return spill(argv[2], tab.data(), tab.size() * 8) ? 0 : 2;
    if (argc != 5 || std::strcmp(argv[1], "values")) {
        std::fprintf(stderr, "usage: csv_cpu_check values <in> <text> <len> | table <out>\n");
        return 2;
    }
    const std::vector<uint8_t> in = slurp(argv[2]);
    if (in.size() < 12) return 2;
    int32_t type;
    uint64_t count;
    std::memcpy(&type, in.data(), 4);
    std::memcpy(&count, in.data() + 4, 8);
    static const size_t sizes[9] = {0, 1, 1, 2, 2, 4, 4, 4, 8};
    if (type < 1 || type > 8 || in.size() != 12 + count * sizes[type]) return 2;
    const size_t z = sizes[type];
    std::string text;
    text.reserve(count * 20);
    std::vector<uint8_t> lens(count);
    for (uint64_t i = 0; i < count; ++i) {
        uint64_t bits = 0;
        std::memcpy(&bits, in.data() + 12 + i * z, z);  // little-endian host
        char buf[4 + MAX_CELL + 4];
        std::memset(buf, 0x7f, sizeof buf);
        const uint32_t n = len(type, bits, tab.data());
        if (n < 1 || n > max_cell(type)) {
            std::fprintf(stderr, "element %llu: len %u outside 1..%u\n", (unsigned long long)i, n, max_cell(type));
            return 1;
        }
        put(type, bits, tab.data(), buf + 4);
        for (size_t k = 0; k < sizeof buf; ++k) {
            const bool inside = k >= 4 && k < 4 + n;
            if (inside == (buf[k] == 0x7f)) {
                std::fprintf(stderr, "element %llu: put wrote other than its %u bytes\n", (unsigned long long)i, n);
                return 1;
            }
        }
        lens[i] = (uint8_t)n;
        text.append(buf + 4, n);
        text.push_back('\n');
    }
    if (!spill(argv[3], text.data(), text.size()) || !spill(argv[4], lens.data(), lens.size())) return 2;
    std::printf("OK %llu\n", (unsigned long long)count);
    return 0;
}
