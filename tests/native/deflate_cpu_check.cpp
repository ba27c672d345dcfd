// TEST INFRASTRUCTURE ONLY: the serial DEFLATE encoder of st_deflate.h on the host.
//
// Every piece of the encoder is __host__ __device__ and the kernels (st_deflate.hip) use the same
// pieces, so this program's stream is the one the device must produce, byte for byte
// (tests/test_deflate_cpu.py checks it against zlib without a GPU, tests/test_deflate_gpu.py checks
// the device against it).  Built together with st_vp8l.cpp, whose huffman_lengths the code builder
// is printed beside.
//
//   deflate_cpu_check stream <in> <out>   the RFC 1951 stream of the file; prints "OK <n> <size>
//                                         <bound>", then per segment "SEG <i> <btype> <bytes>
//                                         <unlimited depth> <longest code>"
//   deflate_cpu_check gzip <in> <out>     the gzip member (st_dev_gzip's bytes)
//   deflate_cpu_check tokens <in>         one line per token: "L <byte>" or "M <length>", "E" after
//                                         each segment
//   deflate_cpu_check code <limit> <count>...   the code builder alone: "LEN <length>...", then
//                                         "COST <its coded bits> <vp8l::huffman_lengths' bits>
//                                         <unlimited depth>"
// The input sits in an allocation of exactly its bytes and the output in one of exactly the bound:
// a read or write past either is a heap overflow that a sanitizer build of this program reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../splat-transform_amd/csrc/st_deflate.h"
#include "../../splat-transform_amd/csrc/st_vp8l.h"

using namespace st::defl;

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
    std::unique_ptr<uint8_t[]> buf(new uint8_t[*n ? *n : 1]);
    if (*n && std::fread(buf.get(), 1, *n, f) != *n) std::perror(path), std::exit(2);
    std::fclose(f);
    if (!*n) buf.reset(new uint8_t[0]);
    return buf;
}

static void write_file(const char *path, const uint8_t *p, uint64_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) std::perror(path), std::exit(2);
    std::fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "code") {
        const uint32_t limit = (uint32_t)std::atoi(argv[2]);
        const int n = argc - 3;
        std::vector<uint32_t> cnt(n), w(n + 1);
        std::vector<uint64_t> cnt64(n);
        std::vector<uint16_t> order(n), par(2 * n + 2);
        std::vector<uint8_t> len(n), vlen(n);
        for (int i = 0; i < n; ++i) cnt64[i] = cnt[i] = (uint32_t)std::strtoul(argv[3 + i], nullptr, 10);
        const int m = sort_used(cnt.data(), n, order.data());
        std::vector<uint32_t> lw(n);
        for (int i = 0; i < m; ++i) lw[i] = cnt[order[i]];
        const uint32_t depth = code_lengths(lw.data(), n, order.data(), m, limit, w.data(), par.data(), len.data());
        st::vp8l::huffman_lengths(cnt64.data(), n, (int)limit, vlen.data());
        uint64_t cost = 0, vcost = 0;
        std::printf("LEN");
        for (int i = 0; i < n; ++i) {
            std::printf(" %u", len[i]);
            cost += cnt64[i] * len[i], vcost += cnt64[i] * vlen[i];
        }
        std::printf("\nCOST %llu %llu %u\n", (unsigned long long)cost, (unsigned long long)vcost, depth);
        return 0;
    }
    uint64_t n = 0;
    const std::unique_ptr<uint8_t[]> in = read_file(argv[2], &n);
    if (mode == "tokens") {
        for (uint64_t b = 0; b < n; b += SEG) {
            const uint32_t len = n - b < SEG ? (uint32_t)(n - b) : SEG;
            const uint8_t *p = in.get() + b;
            for (uint32_t s = 0; s < len;) {
                const uint32_t L = run_length(p, len, s);
                for (uint32_t o = 0; o < L; ++o) {
                    const uint32_t t = token_at(o, L);
                    if (t == 1) std::printf("L %u\n", p[s]);
                    else if (t) std::printf("M %u\n", t);
                }
                s += L;
            }
            std::printf("E\n");
        }
        return 0;
    }
    if (argc < 4 || (mode != "stream" && mode != "gzip")) return 2;
    const uint64_t bound = deflate_bound(n), head = mode == "gzip" ? 10 : 0, room = bound + (head ? 18 : 0);
    std::unique_ptr<uint8_t[]> out(new uint8_t[room]);
    uint8_t *o = out.get();
    if (head) {
        const uint8_t h[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
        std::memcpy(o, h, 10);
    }
    // segment by segment, as encode_stream goes, to report each segment's choice
    uint64_t size = 0;
    std::vector<std::string> lines;
    if (n == 0) {
        size = encode_stream(in.get(), 0, o + head);
    } else {
        Work W;
        Plan P;
        uint32_t cnt[NLIT], tab[NLIT], hdr[HDR_WORDS];
        for (uint64_t b = 0; b < n; b += SEG) {
            const uint32_t len = n - b < SEG ? (uint32_t)(n - b) : SEG;
            size += encode_segment(in.get() + b, len, b + len == n, o + head + size, W, cnt, tab, hdr, P);
            uint32_t longest = 0;
            if (P.btype == 2)
                for (int s = 0; s < NLIT; ++s) longest = (tab[s] >> 16) > longest ? tab[s] >> 16 : longest;
            char line[96];
            std::snprintf(line, sizeof line, "SEG %llu %u %u %u %u", (unsigned long long)(b / SEG), P.btype, P.bytes,
                          P.free_depth, longest);
            lines.push_back(line);
        }
        // the whole-stream entry point gives the same bytes
        std::unique_ptr<uint8_t[]> again(new uint8_t[bound]);
        if (encode_stream(in.get(), n, again.get()) != size || std::memcmp(again.get(), o + head, size)) {
            std::printf("ERR encode_stream differs from its segments\n");
            return 1;
        }
    }
    if (size > bound) {
        std::printf("ERR size %llu above the bound %llu\n", (unsigned long long)size, (unsigned long long)bound);
        return 1;
    }
    uint64_t total = head + size;
    if (head) {
        const uint32_t tail[2] = {crc32_bytes(in.get(), n), (uint32_t)n};
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 4; ++k) o[total++] = (uint8_t)(tail[i] >> (8 * k));
    }
    write_file(argv[3], o, total);
    std::printf("OK %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)size, (unsigned long long)bound);
    for (const std::string &l : lines) std::printf("%s\n", l.c_str());
    return 0;
}
