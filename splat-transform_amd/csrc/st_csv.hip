// st_csv.hip -- writeCsv's rows (writers/write-csv.ts:15-22) on the device: typed columns in, the
// rows' text out -- per row the cells '' + column[i] joined by ',' and a '\n', every cell the exact
// text V8 prints (st_numfmt.h).
//
// Rows have no fixed width, so a piece of rows takes two passes:
//   k_csv_len   a lane is a row (each column's loads coalesce along rows): it walks the row's cells,
//               keeps each cell's offset inside the row (uint16, column-major) and the row's length;
//               scan_u32 over the lengths gives every row's offset in the piece and the total
//   k_csv_rows  a workgroup takes RB consecutive rows, as many as fit its LDS image by the worst-case
//               row width.  A thread is a cell (consecutive threads = consecutive rows of one column):
//               it formats the cell again straight to its place in the image -- known from the two
//               offsets, no atomics -- and the image leaves LDS as coalesced 4-byte stores.  A
//               block's text starts at any byte of the output: the image is laid out at the same
//               offset modulo 4, and the partial first and last words go out byte by byte, so no
//               byte outside the block's own text is written.
// The power-of-ten table (9872 bytes) lives in global memory: lanes index it by their value's
// exponent, which a __constant__ array would serialise; a scene's values share a few dozen
// entries, which stay in the vector L1.
#include <cstring>

#include "st_internal.h"
#include "st_numfmt.h"

namespace st {
namespace {

struct CsvCol {
    const void *ptr;
    int32_t type, pad;
};

__device__ inline uint64_t load_bits(const CsvCol &col, uint64_t row) {
    switch (col.type) {
        case ST_PLY_CHAR:
        case ST_PLY_UCHAR: return ((const uint8_t *)col.ptr)[row];
        case ST_PLY_SHORT:
        case ST_PLY_USHORT: return ((const uint16_t *)col.ptr)[row];
        case ST_PLY_INT:
        case ST_PLY_UINT:
        case ST_PLY_FLOAT: return ((const uint32_t *)col.ptr)[row];
        default: return ((const uint64_t *)col.ptr)[row];
    }
}

// rowlen[r] = the bytes of row row0 + r (cells + one separator each), rowlen[nrows] = 0 (the scan
// then leaves the total there); coff[c * nrows + r] = where cell c starts inside its row
__global__ __launch_bounds__(256) void k_csv_len(const CsvCol *__restrict__ cols, int ncol, uint64_t row0,
                                                 uint32_t nrows, const uint64_t *__restrict__ tab,
                                                 uint16_t *__restrict__ coff, uint32_t *__restrict__ rowlen) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == nrows) rowlen[nrows] = 0;
    if (r >= nrows) return;
    uint32_t run = 0;
    for (int p = 0; p < ncol; ++p) {
        const CsvCol col = cols[p];
        coff[(uint64_t)p * nrows + r] = (uint16_t)run;
        run += numfmt::len(col.type, load_bits(col, row0 + r), tab) + 1;
    }
    rowlen[r] = run;
}

// rows [row0 + blockIdx.x * RB, + RB) of the piece -> out[out_off + rowoff[first] ...): rowoff has
// nrows + 1 entries (the exclusive scan of k_csv_len's lengths); out is 4-byte aligned
__global__ __launch_bounds__(256) void k_csv_rows(const CsvCol *__restrict__ cols, int ncol, uint64_t row0,
                                                  uint32_t nrows, uint32_t RB, const uint64_t *__restrict__ tab,
                                                  const uint16_t *__restrict__ coff,
                                                  const uint32_t *__restrict__ rowoff, uint8_t *__restrict__ out,
                                                  uint64_t out_off) {
    extern __shared__ uint32_t lds32[];
    char *lds8 = (char *)lds32;
    const uint32_t r0 = blockIdx.x * RB;
    const uint32_t nr = nrows - r0 < RB ? nrows - r0 : RB;
    const uint32_t b0 = rowoff[r0], bytes = rowoff[r0 + nr] - b0;
    const uint64_t g = out_off + b0;           // the block's first byte in out
    const uint32_t shift = (uint32_t)(g & 3);  // ... and in the image
    const uint32_t total = nr * (uint32_t)ncol;
    for (uint32_t e = threadIdx.x; e < total; e += blockDim.x) {
        const uint32_t p = e / nr, r = e - p * nr;
        const CsvCol col = cols[p];
        const numfmt::Dec v = numfmt::dec_of(col.type, load_bits(col, row0 + r0 + r), tab);
        char *dst = lds8 + shift + (rowoff[r0 + r] - b0) + coff[(uint64_t)p * nrows + r0 + r];
        numfmt::dec_put(v, dst);
        dst[numfmt::dec_len(v)] = p + 1 == (uint32_t)ncol ? '\n' : ',';
    }
    __syncthreads();
    // image bytes [shift, shift + bytes) -> out[g ...): whole words between, bytes at the two ends
    const uint32_t end = shift + bytes;
    const uint32_t w0 = (shift + 3) >> 2, w1 = end >> 2;
    uint8_t *base = out + (g - shift);  // 4-byte aligned
    for (uint32_t i = w0 + threadIdx.x; i < w1; i += blockDim.x) ((uint32_t *)base)[i] = lds32[i];
    const uint32_t head_end = w0 * 4 < end ? w0 * 4 : end;
    const uint32_t tail = w1 * 4 > head_end ? w1 * 4 : head_end;
    if (shift + threadIdx.x < head_end) base[shift + threadIdx.x] = (uint8_t)lds8[shift + threadIdx.x];
    if (tail + threadIdx.x < end) base[tail + threadIdx.x] = (uint8_t)lds8[tail + threadIdx.x];
}

const uint64_t *host_table() {
    static const std::vector<uint64_t> tab = [] {
        std::vector<uint64_t> t(2 * numfmt::POW10_ENTRIES);
        numfmt::numfmt_build_table(t.data());
        return t;
    }();
    return tab.data();
}

}  // namespace

const uint64_t *numfmt_host_table() { return host_table(); }

uint64_t csv_max_row_bytes(const st_ttable *t) {
    ST_REQUIRE(t->ncol >= 0 && (t->ncol == 0 || t->types), ST_ERR_ARG, "csv: bad table");
    uint64_t w = 0;
    for (int p = 0; p < t->ncol; ++p) {
        const uint32_t m = numfmt::max_cell(t->types[p]);
        ST_REQUIRE(m > 0, ST_ERR_ARG, "csv: bad column type");
        w += m + 1;
    }
    return w;
}

std::string csv_header_text(const st_ttable *t) {
    ST_REQUIRE(t->ncol > 0 && t->names, ST_ERR_ARG, "csv: a table needs at least one column");
    std::string h;
    for (int p = 0; p < t->ncol; ++p) {
        ST_REQUIRE(t->names[p], ST_ERR_ARG, "csv: NULL column name");
        h += t->names[p];
        h += p + 1 == t->ncol ? '\n' : ',';
    }
    return h;
}

CsvRows::CsvRows(st_ctx *ctx, const st_ttable *t, const std::string &tg) : c(ctx), tag(tg) {
    ST_REQUIRE(t->ncol > 0 && t->types && t->cols, ST_ERR_ARG, "csv: a table needs at least one column");
    ncol = t->ncol;
    const uint64_t w = csv_max_row_bytes(t);
    ST_REQUIRE(w <= CSV_LDS_BYTES, ST_ERR_UNSUPPORTED, "csv: rows wider than 48 KiB of text");
    W = (uint32_t)w;
    std::vector<CsvCol> cs(ncol);
    for (int p = 0; p < ncol; ++p) {
        const uint32_t z = (uint32_t)type_size(t->types[p]);
        ST_REQUIRE(t->n == 0 || t->cols[p], ST_ERR_ARG, "csv: NULL column");
        ST_REQUIRE(((uintptr_t)t->cols[p] & (z - 1)) == 0, ST_ERR_ARG, "csv: misaligned column");
        cs[p] = CsvCol{t->cols[p], t->types[p], 0};
    }
    RB = (uint32_t)std::min<uint64_t>(256, CSV_LDS_BYTES / W);
    d_cols = wsT<CsvCol>(c, tag + ".cols", ncol);
    d_tab = wsT<uint64_t>(c, tag + ".pow10", 2 * numfmt::POW10_ENTRIES);
    ST_HIP(hipMemcpyAsync(d_cols, cs.data(), sizeof(CsvCol) * ncol, hipMemcpyHostToDevice, c->stream));
    ST_HIP(hipMemcpyAsync(d_tab, host_table(), 16 * numfmt::POW10_ENTRIES, hipMemcpyHostToDevice, c->stream));
}

uint64_t CsvRows::measure(uint64_t row0, uint64_t nrows) {
    if (!nrows) return 0;
    ST_REQUIRE(nrows * W <= CSV_PIECE_BYTES || nrows == 1, ST_ERR_INTERNAL, "csv: piece too large");
    coff = wsT<uint16_t>(c, tag + ".coff", (uint64_t)ncol * nrows);
    rowoff = wsT<uint32_t>(c, tag + ".off", nrows + 1);
    auto *total = static_cast<uint32_t *>(pinned_slot(c, "csv.total", 16));
    {
        KTimer kt(c, "csv.len");
        hipLaunchKernelGGL(k_csv_len, dim3(grid_for(nrows + 1, 256)), dim3(256), 0, c->stream,
                           (const CsvCol *)d_cols, ncol, row0, (uint32_t)nrows, (const uint64_t *)d_tab, coff, rowoff);
        ST_LAUNCH_CHECK();
    }
    {
        KTimer kt(c, "csv.scan");
        scan_u32(c, rowoff, rowoff, nrows + 1, nullptr);
    }
    ST_HIP(hipMemcpyAsync(total, rowoff + nrows, 4, hipMemcpyDeviceToHost, c->stream));
    ST_HIP(hipStreamSynchronize(c->stream));
    return *total;
}

void CsvRows::write(uint64_t row0, uint64_t nrows, uint8_t *out, uint64_t out_off) {
    if (!nrows) return;
    KTimer kt(c, "csv.rows");
    hipLaunchKernelGGL(k_csv_rows, dim3((unsigned)((nrows + RB - 1) / RB)), dim3(256), (size_t)RB * W + 8, c->stream,
                       (const CsvCol *)d_cols, ncol, row0, (uint32_t)nrows, RB, (const uint64_t *)d_tab,
                       (const uint16_t *)coff, (const uint32_t *)rowoff, out, out_off);
    ST_LAUNCH_CHECK();
}

uint64_t CsvRows::piece_rows(uint64_t bytes) const { return std::max<uint64_t>(1, bytes / W); }

}  // namespace st

using namespace st;

extern "C" {

uint64_t st_csv_max_row_bytes(const st_ttable *t) {
    uint64_t w = 0;
    guard([&] {
        ST_REQUIRE(t, ST_ERR_ARG, "NULL argument");
        w = csv_max_row_bytes(t);
    });
    return w;
}

int st_csv_header_text(const st_ttable *t, char **out, uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(t && out && size, ST_ERR_ARG, "NULL argument");
        const std::string h = csv_header_text(t);
        char *p = static_cast<char *>(std::malloc(h.size() + 1));
        ST_REQUIRE(p, ST_ERR_NOMEM, "csv header: allocation failed");
        std::memcpy(p, h.c_str(), h.size() + 1);
        *out = p;
        *size = h.size();
    });
}

int st_dev_csv_rows(st_ctx *c, const st_ttable *t, uint64_t row0, uint64_t nrows, uint8_t *dev_out, uint64_t cap,
                    uint64_t *size) {
    return guard([&] {
        ST_REQUIRE(c && t && size, ST_ERR_ARG, "NULL argument");
        ST_REQUIRE(row0 <= t->n && nrows <= t->n - row0, ST_ERR_ARG, "csv rows: rows outside the table");
        ST_REQUIRE(((uintptr_t)dev_out & 3) == 0, ST_ERR_ARG, "csv rows: output must be 4-byte aligned");
        use_device(c);
        CsvRows cr(c, t, "csvr");
        *size = 0;
        if (!nrows) return;
        // pieces of at most CSV_PIECE_BYTES of text by the worst-case width (32-bit offsets inside
        // one); the whole size is known, and checked against cap, before a byte is written
        const uint64_t per = cr.piece_rows(CSV_PIECE_BYTES);
        uint64_t total = 0;
        for (uint64_t r = 0; r < nrows; r += per) total += cr.measure(row0 + r, std::min(per, nrows - r));
        *size = total;
        ST_REQUIRE(total <= cap, ST_ERR_ARG, "csv rows: the output buffer is too small");
        ST_REQUIRE(dev_out, ST_ERR_ARG, "NULL argument");
        uint64_t off = 0;
        for (uint64_t r = 0; r < nrows; r += per) {
            const uint64_t nr = std::min(per, nrows - r);
            const uint64_t nb = nrows > per ? cr.measure(row0 + r, nr) : total;
            cr.write(row0 + r, nr, dev_out, off);
            off += nb;
        }
    });
}

}  // extern "C"
