// st_zip_index.h -- the index of a ZIP archive held in memory (plain C++, no HIP): the body of
// st_zip_index (st_zip.cpp), kept in a header so that tests/native/sog_read_cpu_check.cpp can
// compile it alone under AddressSanitizer.
//
// The end-of-central-directory record is searched backwards from the end (it may be followed by
// a comment of up to 65,535 bytes); the central directory gives each entry's name, sizes, CRC
// and local header offset.  Sizes come from the central directory: the reference's writer leaves
// them zero in the local headers and appends data descriptors (serialize/zip-writer.ts:43-74).
// The data begin after the local header's own name and extra field.  Stored entries only, no
// zip64.  Every offset and length is checked against `len` before it is used.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/st_abi.h"

namespace st {

struct ZipIndexError {
    int code;
    std::string msg;
};

inline std::vector<st_zip_entry> zip_index(const uint8_t *d, uint64_t len) {
    auto bad = [](const char *m) -> ZipIndexError { return ZipIndexError{ST_ERR_ARG, std::string("zip: ") + m}; };
    auto u16 = [&](uint64_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); };
    auto u32 = [&](uint64_t o) { return u16(o) | (u16(o + 2) << 16); };
    if (len < 22) throw bad("shorter than an end-of-central-directory record");
    uint64_t eocd = len;  // not found
    const uint64_t lowest = len - 22 > 65535 ? len - 22 - 65535 : 0;
    for (uint64_t o = len - 22;; --o) {
        if (u32(o) == 0x06054b50u && o + 22 + u16(o + 20) <= len) {
            eocd = o;
            break;
        }
        if (o == lowest) break;
    }
    if (eocd == len) throw bad("no end-of-central-directory record");
    const uint32_t disk = u16(eocd + 4), cd_disk = u16(eocd + 6), here = u16(eocd + 8), total = u16(eocd + 10);
    const uint64_t cd_size = u32(eocd + 12), cd_off = u32(eocd + 16);
    if (disk != 0 || cd_disk != 0 || here != total) throw bad("multi-disk archive");
    if (total == 0xffffu || cd_size == 0xffffffffu || cd_off == 0xffffffffu)
        throw ZipIndexError{ST_ERR_UNSUPPORTED, "zip: zip64 archive"};
    if (cd_off > eocd || cd_size > eocd - cd_off) throw bad("central directory outside the archive");
    std::vector<st_zip_entry> out;
    out.reserve(total);
    uint64_t o = cd_off;
    const uint64_t cd_end = cd_off + cd_size;
    for (uint32_t i = 0; i < total; ++i) {
        if (cd_end - o < 46) throw bad("central directory entry cut short");
        if (u32(o) != 0x02014b50u) throw bad("bad central directory signature");
        const uint32_t method = u16(o + 10), nl = u16(o + 28), xl = u16(o + 30), cl = u16(o + 32);
        const uint64_t csize = u32(o + 20), usize = u32(o + 24), local = u32(o + 42);
        if ((uint64_t)nl + xl + cl > cd_end - o - 46) throw bad("central directory entry cut short");
        if (method != 0) throw ZipIndexError{ST_ERR_UNSUPPORTED, "zip: compressed entry (stored entries only)"};
        if (csize != usize) throw bad("stored entry with unequal sizes");
        if (local > len || len - local < 30) throw bad("local header outside the archive");
        if (u32(local) != 0x04034b50u) throw bad("bad local header signature");
        const uint64_t data = local + 30 + (uint64_t)u16(local + 26) + u16(local + 28);
        if (data > len || usize > len - data) throw bad("entry data outside the archive");
        st_zip_entry e;
        e.name_offset = o + 46;
        e.name_len = nl;
        e.crc = u32(o + 16);
        e.offset = data;
        e.size = usize;
        out.push_back(e);
        o += 46 + (uint64_t)nl + xl + cl;
    }
    return out;
}

}  // namespace st
