// TEST INFRASTRUCTURE ONLY: the host pieces of the .sog reader -- the WebP-lossless decoder
// (st_vp8l_dec.cpp) and the ZIP index (st_zip_index.h) -- in a stand-alone program, so that they
// can be checked without a GPU and under AddressSanitizer + UBSan (tests/test_read_sog_cpu.py).
// Never linked into libsplat_hip.
//
//   sog_read_cpu_check decode in.webp out.rgba    prints "W H"; exit 1 + the message on an error
//   sog_read_cpu_check index in.zip               one line per entry: name offset size crc
//   sog_read_cpu_check fuzz-webp in.webp seed n   every prefix truncation and n seeded single-byte
//   sog_read_cpu_check fuzz-zip in.zip seed n     corruptions: each must give an error or a full
//                                                 result; prints "ok <accepted> <rejected>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../splat-transform_amd/csrc/st_zip_index.h"

static std::string g_err;
namespace st {
void set_last_error(const std::string &m) { g_err = m; }
}  // namespace st

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// decode into an exactly sized heap block (ASan guards both ends); rc and the pixels
static int decode(const uint8_t *d, uint64_t n, std::vector<uint8_t> *out, int *w, int *h) {
    int32_t ww = 0, hh = 0;
    int rc = st_webp_info(d, n, &ww, &hh);
    if (rc != ST_OK) return rc;
    if (ww < 1 || hh < 1 || ww > 16384 || hh > 16384) {
        fprintf(stderr, "st_webp_info accepted a size out of range: %d x %d\n", ww, hh);
        exit(4);
    }
    uint8_t *px = (uint8_t *)malloc((size_t)ww * hh * 4);
    if (!px) return ST_ERR_NOMEM;
    rc = st_webp_decode_lossless(d, n, px, ww * 4);
    if (rc == ST_OK && out) out->assign(px, px + (size_t)ww * hh * 4);
    free(px);
    *w = ww, *h = hh;
    return rc;
}

static int check_zip(const uint8_t *d, uint64_t n) {
    try {
        const std::vector<st_zip_entry> es = st::zip_index(d, n);
        uint64_t sum = 0;
        for (const st_zip_entry &e : es) {
            if (e.name_offset > n || e.name_len > n - e.name_offset || e.offset > n || e.size > n - e.offset) {
                fprintf(stderr, "zip_index returned an entry outside the archive\n");
                exit(4);
            }
            // touch every byte it points at
            for (uint64_t k = 0; k < e.name_len; ++k) sum += d[e.name_offset + k];
            for (uint64_t k = 0; k < e.size; ++k) sum += d[e.offset + k];
        }
        return sum == ~0ull ? 2 : ST_OK;
    } catch (const st::ZipIndexError &e) {
        if (e.code != ST_ERR_ARG && e.code != ST_ERR_UNSUPPORTED) exit(4);
        return e.code;
    }
}

// xorshift64*: the corruptions' positions and values
static uint64_t rnd(uint64_t &s) {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    return s * 0x2545F4914F6CDD1Dull;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> file = slurp(argv[2]);
    if (mode == "decode" && argc == 4) {
        std::vector<uint8_t> px;
        int w = 0, h = 0;
        const int rc = decode(file.data(), file.size(), &px, &w, &h);
        if (rc != ST_OK) {
            printf("error %d %s\n", rc, g_err.c_str());
            return 1;
        }
        FILE *o = fopen(argv[3], "wb");
        if (!o || fwrite(px.data(), 1, px.size(), o) != px.size()) return 3;
        fclose(o);
        printf("%d %d\n", w, h);
        return 0;
    }
    if (mode == "index") {
        try {
            for (const st_zip_entry &e : st::zip_index(file.data(), file.size()))
                printf("%.*s %llu %llu %u\n", (int)e.name_len, (const char *)file.data() + e.name_offset,
                       (unsigned long long)e.offset, (unsigned long long)e.size, e.crc);
        } catch (const st::ZipIndexError &e) {
            printf("error %d %s\n", e.code, e.msg.c_str());
            return 1;
        }
        return 0;
    }
    if ((mode == "fuzz-webp" || mode == "fuzz-zip") && argc == 5) {
        const bool webp = mode == "fuzz-webp";
        uint64_t seed = strtoull(argv[3], nullptr, 10) * 2 + 1;
        const int ncorrupt = atoi(argv[4]);
        long accepted = 0, rejected = 0;
        auto run = [&](const uint8_t *d, uint64_t n) {
            int w = 0, h = 0;
            const int rc = webp ? decode(d, n, nullptr, &w, &h) : check_zip(d, n);
            if (rc == ST_OK)
                ++accepted;
            else if (rc == ST_ERR_ARG || rc == ST_ERR_UNSUPPORTED)
                ++rejected;
            else {
                fprintf(stderr, "unexpected status %d (%s)\n", rc, g_err.c_str());
                exit(4);
            }
        };
        // every prefix, each in a heap block of exactly its size
        for (size_t n = 0; n < file.size(); ++n) {
            uint8_t *cut = (uint8_t *)malloc(n ? n : 1);
            memcpy(cut, file.data(), n);
            run(cut, n);
            free(cut);
        }
        for (int k = 0; k < ncorrupt; ++k) {
            std::vector<uint8_t> bad = file;
            const size_t at = (size_t)(rnd(seed) % bad.size());
            bad[at] ^= (uint8_t)(1 + rnd(seed) % 255);
            uint8_t *blk = (uint8_t *)malloc(bad.size());
            memcpy(blk, bad.data(), bad.size());
            run(blk, bad.size());
            free(blk);
        }
        printf("ok %ld %ld\n", accepted, rejected);
        return 0;
    }
    return 2;
}
