// jsmath_cpu_check -- the scalar rules of splat-transform_amd/csrc/st_jsmath.h on the host, through
// the expressions st_dev_probe evaluates on the device (csrc/st_probe_ops.h), for
// tests/test_jsmath_cpu.py and tests/test_probe_scalar_gpu.py.  Build with -ffp-contract=off, as the
// library is.
//
//   jsmath_cpu_check <op> <in0> <in1 | -> <s> <out>
//       op: an ST_PROBE_* scalar code.  in0, in1: float64 arrays of one length (in1 only for the
//       two-input ops).  s: LOGEXP's factor, as the 16 hex digits of its bits.  out: the results,
//       each in the op's output type.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../splat-transform_amd/csrc/st_probe_ops.h"

static std::vector<double> slurp(const char *path, bool *ok) {
    std::vector<double> v;
    *ok = false;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (n % 8 == 0) {
        v.resize((size_t)n / 8);
        *ok = !n || std::fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const int op = std::atoi(argv[1]);
    if (!st::probe::is_scalar(op)) return 2;
    bool ok;
    const std::vector<double> a = slurp(argv[2], &ok);
    if (!ok) return 2;
    std::vector<double> b;
    if (st::probe::two_inputs(op)) {
        b = slurp(argv[3], &ok);
        if (!ok || b.size() != a.size()) return 2;
    }
    const uint64_t sbits = std::strtoull(argv[4], nullptr, 16);
    double s;
    std::memcpy(&s, &sbits, 8);
    const size_t w = (size_t)st::probe::out_size(op);
    std::vector<uint8_t> out(a.size() * w);
    for (size_t i = 0; i < a.size(); ++i) {
        const uint64_t r = st::probe::scalar(op, a[i], b.empty() ? 0.0 : b[i], s);
        std::memcpy(out.data() + i * w, &r, w);  // little-endian: the low bytes
    }
    FILE *f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    const bool wrote = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && wrote) ? 0 : 2;
}
