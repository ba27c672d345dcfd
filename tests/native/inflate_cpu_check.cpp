// TEST INFRASTRUCTURE ONLY: the chunked INFLATE of st_inflate.h, serially on the host.
//
// Every rule of the decoder is __host__ __device__ and the kernels (st_inflate.hip) use the same
// rules in the same steps, so this program's bytes and statistics are the ones the device must give
// (tests/test_inflate_cpu.py checks it against zlib without a GPU, tests/test_inflate_gpu.py checks
// the device against it).
//
//   inflate_cpu_check inflate <in> <want> <expect> <chunk>...   the raw deflate stream of <in> by
//       inflate_chunked at each chunk size (0 = the default), compared with the bytes of <want>;
//       one line per chunk size:
//         "R <chunk> OK <chunks> <candidates> <kept> <discarded> <markers> <stored> <fixed> <dynamic>"
//         "R <chunk> DECLINED"       or      "R <chunk> WRONG <first differing byte>" (exit status 1)
//   inflate_cpu_check gunzip <in> <want> <expect> <chunk>...    the same for a gzip member: layout,
//       stream, CRC-32 and ISIZE; "L <stream offset> <stream bytes> <crc> <isize>" comes first
//   inflate_cpu_check head <in> <want bytes>     inflate_head: "H <got> <hex>" or "H BROKEN"
//   inflate_cpu_check starts <in>                a plain sequential decode of the raw stream: one line
//       "B <bit position> <BFINAL> <BTYPE> <candidate_at's answer>" per block, then "E <bytes>"
// The input sits in an allocation of exactly its bytes and the output in one of exactly <expect>:
// a read or write past either is a heap overflow that a sanitizer build of this program reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../splat-transform_amd/csrc/st_inflate.h"

using namespace st::infl;

static uint32_t crc32_bytes(const uint8_t *p, uint64_t n) {
    static uint32_t T[256];
    if (!T[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
            T[i] = c;
        }
    uint32_t c = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) c = T[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return ~c;
}

static std::unique_ptr<uint8_t[]> read_file(const char *path, uint64_t *n) {
    FILE *f = std::fopen(path, "rb");
    if (!f) std::perror(path), std::exit(2);
    std::fseek(f, 0, SEEK_END);
    *n = (uint64_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[*n]);
    if (*n && std::fread(buf.get(), 1, *n, f) != *n) std::perror(path), std::exit(2);
    std::fclose(f);
    return buf;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    uint64_t n = 0;
    const std::unique_ptr<uint8_t[]> in = read_file(argv[2], &n);
    if (mode == "head") {
        if (argc < 4) return 2;
        const uint64_t want = std::strtoull(argv[3], nullptr, 10);
        std::unique_ptr<uint8_t[]> out(new uint8_t[want]);
        uint64_t got = 0;
        if (!inflate_head(in.get(), n, out.get(), want, &got)) {
            std::printf("H BROKEN\n");
            return 0;
        }
        std::printf("H %llu ", (unsigned long long)got);
        for (uint64_t i = 0; i < got; ++i) std::printf("%02x", out[i]);
        std::printf("\n");
        return 0;
    }
    if (mode == "starts") {
        std::vector<uint8_t> tab(TABLE_BYTES);
        Tables T = tables_at(tab.data());
        Bits b;
        bits_at(b, in.get(), n, 0);
        SizeSink s{0, ~0ull, true};
        for (uint64_t k = max_blocks(n); k; --k) {
            const uint64_t p = bit_pos(b);
            bool final = false;
            uint32_t btype = 0;
            uint64_t budget = ~0ull;
            if (!decode_block(b, T, s, budget, final, btype)) {
                std::printf("X %llu\n", (unsigned long long)p);
                return 1;
            }
            std::printf("B %llu %d %u %d\n", (unsigned long long)p, (int)final, btype, (int)candidate_at(in.get(), n, p));
            if (final) break;
        }
        std::printf("E %llu\n", (unsigned long long)s.count);
        return 0;
    }
    if (argc < 6 || (mode != "inflate" && mode != "gunzip")) return 2;
    uint64_t nwant = 0;
    const std::unique_ptr<uint8_t[]> want = read_file(argv[3], &nwant);
    const uint64_t expect = std::strtoull(argv[4], nullptr, 10);
    const uint8_t *stream = in.get();
    uint64_t len = n;
    Member M{};
    bool member_ok = true;
    if (mode == "gunzip") {
        member_ok = member_layout(in.get(), n, M);
        if (member_ok) {
            std::printf("L %llu %llu %u %u\n", (unsigned long long)M.stream_off, (unsigned long long)M.stream_len, M.crc, M.isize);
            stream = in.get() + M.stream_off, len = M.stream_len;
        }
    }
    int rc = 0;
    for (int a = 5; a < argc; ++a) {
        const uint32_t chunk = (uint32_t)std::strtoul(argv[a], nullptr, 10);
        std::unique_ptr<uint8_t[]> out(new uint8_t[expect]);
        Stats st{};
        bool ok = member_ok && (mode != "gunzip" || M.isize == (uint32_t)expect);
        ok = ok && inflate_chunked(stream, len, out.get(), expect, chunk, st);
        ok = ok && (mode != "gunzip" || crc32_bytes(out.get(), expect) == M.crc);
        if (!ok) {
            std::printf("R %u DECLINED\n", chunk);
            continue;
        }
        uint64_t d = 0;
        while (d < expect && d < nwant && out[d] == want[d]) ++d;
        if (expect != nwant || d != expect) {
            std::printf("R %u WRONG %llu\n", chunk, (unsigned long long)d);
            rc = 1;
            continue;
        }
        std::printf("R %u OK %llu %llu %llu %llu %llu %llu %llu %llu\n", chunk, (unsigned long long)st.chunks,
                    (unsigned long long)st.candidates, (unsigned long long)st.kept, (unsigned long long)st.discarded,
                    (unsigned long long)st.markers, (unsigned long long)st.stored_blocks, (unsigned long long)st.fixed_blocks,
                    (unsigned long long)st.dynamic_blocks);
    }
    return rc;
}
