// neighbors_cpu_check -- the serial host form of splat-transform_amd/csrc/st_neighbors.h (the functions
// the kernels call: placed, d2, the k best, the argument rules, the threshold and the verdict) on the
// host, for tests/test_neighbors_cpu.py.  Build with -ffp-contract=off, as the library is.
//
//   neighbors_cpu_check <in> <out>
//   in:  uint64 n; three columns in the order x y z, each an int32 st_ply_type code and n elements as
//        stored; uint32 query count; per query an int32 kind and its parameters:
//          1 dist       int32 k (1..32)
//          2 outliers   int32 k, int32 mode, double value
//          3 bound      twelve doubles: node min x y z, node max, query min, query max
//   out: per query -- 1: n doubles; 2: a uint64 count and that many uint32 rows (count 2^64 - 1 and no
//        rows when k, the mode or the value is refused); 3: one double (box_bound).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../splat-transform_amd/csrc/st_neighbors.h"

using namespace st::nbr;

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

struct Reader {
    const std::vector<uint8_t> &in;
    size_t at = 0;
    bool bad = false;
    template <typename T>
    T get() {
        T v{};
        if (in.size() - at < sizeof(T)) bad = true;
        else std::memcpy(&v, in.data() + at, sizeof(T)), at += sizeof(T);
        return v;
    }
};

template <typename T>
static void put(std::vector<uint8_t> &out, const T *p, size_t count) {
    if (!count) return;
    const uint8_t *b = reinterpret_cast<const uint8_t *>(p);
    out.insert(out.end(), b, b + count * sizeof(T));
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: neighbors_cpu_check <in> <out>\n");
        return 2;
    }
    bool ok;
    const std::vector<uint8_t> in = slurp(argv[1], &ok);
    if (!ok) return 2;
    Reader r{in};
    const uint64_t n = r.get<uint64_t>();
    // a copy of exactly each column's bytes: a read past either end is the sanitizer's to find
    std::vector<std::vector<uint8_t>> data(3);
    Col cols[3];
    for (int k = 0; k < 3; ++k) {
        const int32_t type = r.get<int32_t>();
        const int z = st::sm::elem_size(type);
        if (r.bad || !z || (in.size() - r.at) / (size_t)z < n) return 2;
        data[k].assign(in.begin() + (long)r.at, in.begin() + (long)(r.at + n * (size_t)z));
        r.at += n * (size_t)z;
        static const uint64_t none = 0;
        cols[k] = Col{n ? (const void *)data[k].data() : (const void *)&none, type};
    }
    std::vector<uint8_t> out;
    std::map<int, std::vector<double>> dists;
    auto dist_of = [&](int k) -> const std::vector<double> & {
        auto it = dists.find(k);
        if (it == dists.end()) {
            it = dists.emplace(k, std::vector<double>(n)).first;
            dist_host(cols, n, k, it->second.data());
        }
        return it->second;
    };
    const uint32_t nq = r.get<uint32_t>();
    for (uint32_t q = 0; q < nq && !r.bad; ++q) {
        const int32_t kind = r.get<int32_t>();
        if (kind == 1) {
            const int32_t k = r.get<int32_t>();
            if (r.bad || !k_ok(k)) return 2;
            put(out, dist_of(k).data(), n);
        } else if (kind == 2) {
            const int32_t k = r.get<int32_t>(), mode = r.get<int32_t>();
            const double value = r.get<double>();
            if (r.bad) return 2;
            uint64_t count = ~0ull;
            std::vector<uint32_t> rows;
            if (k_ok(k) && outlier_args_ok(mode, value)) {
                rows = outliers_host(dist_of(k).data(), n, mode, value);
                count = rows.size();
            }
            put(out, &count, 1);
            put(out, rows.data(), rows.size());
        } else if (kind == 3) {
            double b[12];
            for (double &v : b) v = r.get<double>();
            const double lb = box_bound(b, b + 3, b + 6, b + 9);
            put(out, &lb, 1);
        } else {
            return 2;
        }
    }
    if (r.bad) return 2;
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool w = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && w ? 0 : 2;
}
