// st_chain.hip -- processDataTable (process.ts:64-145) over a table resident in HBM, and the
// CLI's `in.ply [actions] out.compressed.ply` (index.ts:463-496 -> writeCompressedPly,
// write-compressed-ply.ts:31-115) as one call: the table crosses PCIe once in each direction
// (columns up, packed chunk / vertex / sh bytes down) instead of once per action.
//
// The chain holds the current table as (name, type, device pointer) columns.  A transform
// updates float32 columns in place; a filter gathers the survivors into the other of two
// workspace generations (ping-pong), so a long action list needs at most two copies of the
// table beside the input.
#include <unistd.h>

#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <thread>

#include <chrono>

#include "st_internal.h"
#include "st_typed.h"
#include "st_webp.h"

namespace st {
namespace {

struct ChainCol {
    std::string name;
    int32_t type;
    void *ptr;
};

struct Chain {
    st_ctx *c;
    uint64_t n = 0;
    std::vector<ChainCol> cols;
    int gen = 0;                  // workspace generation the next filter writes
    std::string tag = "chain";    // workspace slot prefix (several chains alive at once)

    // views over the current columns (rebuilt on demand; pointers stay valid until the next change)
    std::vector<const char *> names;
    std::vector<int32_t> types;
    std::vector<void *> ptrs;
    std::vector<float *> fptrs;
    std::vector<const char *> fnames;
    st_ttable tt{};
    st_table ft{};

    const st_ttable *typed() {
        names.clear(), types.clear(), ptrs.clear();
        for (auto &k : cols) names.push_back(k.name.c_str()), types.push_back(k.type), ptrs.push_back(k.ptr);
        tt = st_ttable{n, (int32_t)cols.size(), names.data(), types.data(), ptrs.data()};
        return &tt;
    }
    // the float32 columns as an st_table (the transform / pack kernels read columns by name)
    const st_table *f32() {
        fnames.clear(), fptrs.clear();
        for (auto &k : cols)
            if (k.type == ST_PLY_FLOAT) fnames.push_back(k.name.c_str()), fptrs.push_back(static_cast<float *>(k.ptr));
        ft = st_table{n, (int32_t)fptrs.size(), fnames.data(), fptrs.data()};
        return &ft;
    }
    bool has(const std::string &nm) const {
        for (auto &k : cols)
            if (k.name == nm) return true;
        return false;
    }
    int coeffs() const {  // the band of the current columns
        return band_coeffs([&](const char *nm) { return has(nm); });
    }
    // the kernels read these by name from the float32 columns: a same-named column of another
    // type would be silently skipped (the reference reads any type through getRow)
    void require_f32(const std::string &nm, const char *what) const {
        for (auto &k : cols)
            if (k.name == nm && k.type != ST_PLY_FLOAT)
                throw Error(ST_ERR_UNSUPPORTED, std::string(what) + ": column " + nm + " is not float32");
    }

    void gather(const uint32_t *idx, uint64_t m) {
        const st_ttable *src = typed();
        std::vector<void *> dst(cols.size());
        for (size_t i = 0; i < cols.size(); ++i)
            dst[i] = ws(c, tag + ".g" + std::to_string(gen) + "." + std::to_string(i), m * type_size(cols[i].type) + 16);
        st_ttable d = *src;
        d.n = m;
        d.cols = dst.data();
        permute_rows_tdev(c, src, idx, m, &d);
        for (size_t i = 0; i < cols.size(); ++i) cols[i].ptr = dst[i];
        n = m;
        gen ^= 1;
    }
};

void run_actions(Chain &ch, const st_action *actions, int nactions) {
    const int in_coeffs = ch.coeffs();  // filterBands reads the ORIGINAL table (process.ts:111)
    // the importance kinds' argument errors before anything is launched (no action adds or removes
    // a scale or opacity column, and the amount's validity does not depend on the row count)
    // (filterOutliers alike: no action adds or removes a position column)
    for (int a = 0; a < nactions; ++a) {
        if (actions[a].kind == ST_ACTION_FILTER_OUTLIERS) outliers_require(ch.typed(), actions[a]);
        if (actions[a].kind == ST_ACTION_FILTER_CLUSTERS) filter_clusters_require(ch.typed(), actions[a]);
        if (actions[a].kind != ST_ACTION_DECIMATE && actions[a].kind != ST_ACTION_ORDER_IMPORTANCE) continue;
        const bool dec = actions[a].kind == ST_ACTION_DECIMATE;
        importance_require(ch.typed(), dec ? "decimate" : "orderByImportance");
        if (dec) (void)decimate_rows_checked(actions[a], 0);
    }
    for (int a = 0; a < nactions; ++a) {
        const st_action &act = actions[a];
        switch (act.kind) {
            case ST_ACTION_TRANSFORM:
                // every column type, as getRow / setRow (transform.ts:24-63)
                transform_tdev(ch.c, ch.typed(), &act.transform);
                break;
            case ST_ACTION_FILTER_NAN:
            case ST_ACTION_FILTER_VALUE: {
                if (ch.n == 0) break;
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                const uint64_t m = act.kind == ST_ACTION_FILTER_NAN
                                       ? filter_finite_tdev(ch.c, ch.typed(), idx)
                                       : filter_value_tdev(ch.c, ch.typed(), act.column, act.compare, act.value, idx);
                if (m != ch.n) ch.gather(idx, m);  // all rows kept: permuteRows by the identity
                break;
            }
            case ST_ACTION_FILTER_BANDS: {
                ST_REQUIRE(act.bands >= 0 && act.bands <= 3, ST_ERR_ARG, "filterBands: bands must be 0..3");
                static const int coeffs[4] = {0, 3, 8, 15};
                const int out_coeffs = coeffs[act.bands];
                if (out_coeffs >= in_coeffs) break;  // outputBands < inputBands only (:115)
                std::vector<ChainCol> next;
                for (auto &k : ch.cols) {
                    int hit = -1, to = -1;
                    for (int i = 0; i < in_coeffs && hit < 0; ++i)
                        for (int j = 0; j < 3 && hit < 0; ++j)
                            if (k.name == "f_rest_" + std::to_string(i + j * in_coeffs)) {
                                hit = 1;
                                if (i < out_coeffs) to = i + j * out_coeffs;
                            }
                    if (hit < 0) next.push_back(k);
                    else if (to >= 0) next.push_back(ChainCol{"f_rest_" + std::to_string(to), k.type, k.ptr});
                }
                ch.cols.swap(next);
                break;
            }
            case ST_ACTION_PARAM:
                break;
            // this project's own kinds (st_abi.h, "importance, decimation and crops"): row
            // selections and one reordering, all through permuteRows like the filters
            case ST_ACTION_FILTER_BOX:
            case ST_ACTION_FILTER_SPHERE: {
                if (ch.n == 0) break;
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                const uint64_t m = act.kind == ST_ACTION_FILTER_BOX
                                       ? filter_box_tdev(ch.c, ch.typed(), act.box_min, act.box_max, ch.tag, idx)
                                       : filter_sphere_tdev(ch.c, ch.typed(), act.center, act.radius, ch.tag, idx);
                if (m != ch.n) ch.gather(idx, m);
                break;
            }
            case ST_ACTION_DECIMATE: {
                const uint64_t m = decimate_rows_checked(act, ch.n);
                if (m == ch.n) break;  // every row kept: permuteRows by the identity
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                if (m) importance_top_tdev(ch.c, ch.typed(), m, ch.tag, idx);
                ch.gather(idx, m);
                break;
            }
            case ST_ACTION_ORDER_IMPORTANCE: {
                if (ch.n <= 1) break;
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                importance_order_tdev(ch.c, ch.typed(), ch.tag, idx);
                ch.gather(idx, ch.n);
                break;
            }
            // st_abi.h, "neighbour distances and outliers": dist_k into a slot under the chain's tag,
            // the threshold from the summary's device steps on that column, a stable selection
            case ST_ACTION_FILTER_OUTLIERS: {
                if (ch.n == 0) break;
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                const uint64_t m = filter_outliers_tdev(ch.c, ch.typed(), act, ch.tag, idx);
                if (m != ch.n) ch.gather(idx, m);
                break;
            }
            // st_abi.h, "clusters": the sizes of the link graph's components, a stable selection
            case ST_ACTION_FILTER_CLUSTERS: {
                if (ch.n == 0) break;
                auto *idx = wsT<uint32_t>(ch.c, ch.tag + ".idx", ch.n);
                const uint64_t m = filter_clusters_tdev(ch.c, ch.typed(), act, ch.tag, idx);
                if (m != ch.n) ch.gather(idx, m);
                break;
            }
            default:
                throw Error(ST_ERR_ARG, "process: unknown action kind " + std::to_string(act.kind));
        }
    }
}

// writeCompressedPly's device part on the processed table: Morton order of the identity
// (write-compressed-ply.ts:59-64), then the chunk loop
// (any column types: the chunk members go through CompressedChunk's Float32Arrays
// (compressed-chunk.ts:28-41), the ordering and the SH bytes read the row's JS numbers
// (ordering.ts:32-47, write-compressed-ply.ts:85))
const char *const SH_NAMES[45] = {
    "f_rest_0",  "f_rest_1",  "f_rest_2",  "f_rest_3",  "f_rest_4",  "f_rest_5",  "f_rest_6",  "f_rest_7",  "f_rest_8",
    "f_rest_9",  "f_rest_10", "f_rest_11", "f_rest_12", "f_rest_13", "f_rest_14", "f_rest_15", "f_rest_16", "f_rest_17",
    "f_rest_18", "f_rest_19", "f_rest_20", "f_rest_21", "f_rest_22", "f_rest_23", "f_rest_24", "f_rest_25", "f_rest_26",
    "f_rest_27", "f_rest_28", "f_rest_29", "f_rest_30", "f_rest_31", "f_rest_32", "f_rest_33", "f_rest_34", "f_rest_35",
    "f_rest_36", "f_rest_37", "f_rest_38", "f_rest_39", "f_rest_40", "f_rest_41", "f_rest_42", "f_rest_43", "f_rest_44"};

void compressed_tail(Chain &ch, float *chunk, uint32_t *vertex, uint8_t *sh, int32_t *out_coeffs) {
    static const char *pcols[] = {"x", "y", "z", "scale_0", "scale_1", "scale_2", "f_dc_0",
                                  "f_dc_1", "f_dc_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3"};
    const int C = ch.coeffs();
    *out_coeffs = C;
    if (ch.n == 0) return;
    const st_ttable *tt = ch.typed();
    std::vector<const char *> fn;
    std::vector<float *> fp;
    TCol xyz[3];
    for (int i = 0; i < 14; ++i) {
        const TCol col = tcol_or_null(tt, pcols[i]);
        ST_REQUIRE(col.p, ST_ERR_ARG, std::string("pack_compressed: missing column ") + pcols[i]);
        if (i < 3) xyz[i] = col;
        fn.push_back(pcols[i]);
        fp.push_back(const_cast<float *>(as_f32_dev(ch.c, col, ch.n, ch.tag + ".m32." + std::to_string(i))));
    }
    bool sh32 = true;
    std::vector<const double *> sh64;
    for (int i = 0; i < 3 * C; ++i) sh32 = sh32 && tcol_or_null(tt, SH_NAMES[i]).t == ST_PLY_FLOAT;
    for (int i = 0; i < 3 * C; ++i) {
        const TCol col = tcol_or_null(tt, SH_NAMES[i]);
        if (sh32) fn.push_back(SH_NAMES[i]), fp.push_back(static_cast<float *>(col.p));
        else sh64.push_back(as_f64_dev(ch.c, col, ch.n, ch.tag + ".sh64." + std::to_string(i)));
    }
    const st_table t{ch.n, (int32_t)fp.size(), fn.data(), fp.data()};
    auto *order = wsT<uint32_t>(ch.c, "chain.order", ch.n);
    iota_u32(ch.c, order, ch.n);
    const void *xp[3] = {xyz[0].p, xyz[1].p, xyz[2].p};
    const int32_t xt[3] = {xyz[0].t, xyz[1].t, xyz[2].t};
    morton_order_tdev(ch.c, xp, xt, order, ch.n);
    pack_compressed_dev(ch.c, &t, order, chunk, vertex, sh, sh32 ? nullptr : sh64.data(), C);
}

void check_src(const st_ttable *src) {
    ST_REQUIRE(src->ncol >= 0 && (src->ncol == 0 || (src->names && src->types && src->cols)), ST_ERR_ARG,
               "process: bad table");
    for (int i = 0; i < src->ncol; ++i) {
        ST_REQUIRE(type_size(src->types[i]) > 0, ST_ERR_ARG, "process: bad column type");
        ST_REQUIRE(src->n == 0 || src->cols[i], ST_ERR_ARG, "process: NULL column");
    }
}

// upload the host table once
void upload_chain(st_ctx *c, const st_ttable *src, Chain &ch) {
    ch.n = src->n;
    std::vector<HostXfer> up;
    for (int i = 0; i < src->ncol; ++i) {
        const int sz = type_size(src->types[i]);
        void *d = ws_upload(c, "chain.in." + std::to_string(i), src->cols[i], src->n * sz, up);
        ch.cols.push_back(ChainCol{src->names[i], src->types[i], d});
    }
    staged_h2d(c, up);
}

// the element's rows straight from the file into HBM columns (page cache -> pinned -> HBM,
// st_dev_ply_read); element < 0 selects the one named "vertex" (read-ply.ts's splat element)
void ply_chain(st_ctx *c, int fd, const st_ply_header *h, int element, Chain &ch) {
    if (element < 0)
        for (int e = 0; e < h->nelements && element < 0; ++e)
            if (std::strcmp(h->elements[e].name, "vertex") == 0) element = e;
    ST_REQUIRE(element >= 0 && element < h->nelements, ST_ERR_ARG, "ply: no such element");
    const st_ply_element &el = h->elements[element];
    std::vector<void *> cols(el.nprops);
    for (int p = 0; p < el.nprops; ++p) {
        cols[p] = ws(c, "chain.in." + std::to_string(p), el.count * type_size(el.props[p].type) + 16);
        ch.cols.push_back(ChainCol{el.props[p].name, el.props[p].type, cols[p]});
    }
    ch.n = el.count;
    ply_read_dev(c, fd, *h, element, cols.data());
}

// the processed table as the multi-GPU writeSog takes it: float32 columns by name (the sharded
// path moves float32 columns only; a single device takes every type through sog_tdev)
const st_table *sog_view(Chain &ch) {
    for (auto &nm : sog_columns()) ch.require_f32(nm, "multi-GPU writeSog");
    return ch.f32();
}

// ---- writeCompressedPly into a file (write-compressed-ply.ts:31-115 + the CLI's write) --------
// the header text of write-compressed-ply.ts:35-54
std::string compressed_ply_header(uint64_t m, int C, const char *version) {
    static const char *chunk_props[18] = {"min_x", "min_y", "min_z", "max_x", "max_y", "max_z",
                                          "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y",
                                          "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"};
    static const char *vertex_props[4] = {"packed_position", "packed_rotation", "packed_scale", "packed_color"};
    std::string h = "ply\nformat binary_little_endian 1.0\ncomment Generated by splat-transform ";
    h += (version && *version) ? version : "0.10.1";
    h += "\nelement chunk " + std::to_string((m + 255) / 256) + "\n";
    for (auto *p : chunk_props) h += std::string("property float ") + p + "\n";
    h += "element vertex " + std::to_string(m) + "\n";
    for (auto *p : vertex_props) h += std::string("property uint ") + p + "\n";
    if (C) {
        h += "element sh " + std::to_string(m) + "\n";
        for (int i = 0; i < 3 * C; ++i) h += "property uchar f_rest_" + std::to_string(i) + "\n";
    }
    return h + "end_header\n";
}

// device bytes on their way into a file: pinned slots filled by device-to-host copies on the
// context's stream while a host thread writes the slot before (ext4 / xfs serialise buffered
// writes to one file, so one writer).  next() hands out the next slot once the writer is done with
// it; the caller queues a copy into it and submit()s it with its file offset; finish() waits for
// the writer and rethrows its error.  ST_CPF_SLOT_MB: the slot size (32 MiB).
struct FileRing {
    static constexpr int SLOTS = 4;
    st_ctx *c;
    int fd;
    uint64_t slot = 32ull << 20;
    uint8_t *ring;
    struct Piece {
        int s;
        uint64_t bytes, off;
        hipEvent_t ev;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Piece> q;
    bool busy[SLOTS] = {}, fin = false;
    std::exception_ptr err;
    std::thread writer;
    int k = 0, cur = -1;
    FileRing(st_ctx *ctx, int f) : c(ctx), fd(f) {
        if (const char *e = std::getenv("ST_CPF_SLOT_MB")) slot = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) << 20;
        ring = static_cast<uint8_t *>(pinned_slot(c, "cpf.ring", SLOTS * slot));
        writer = std::thread([this] { loop(); });
    }
    void loop() {
        for (;;) {
            Piece p;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return fin || !q.empty(); });
                if (q.empty()) return;
                p = q.front();
                q.pop_front();
            }
            try {
                const hipError_t e = hipEventSynchronize(p.ev);
                (void)hipEventDestroy(p.ev);
                ST_HIP(e);
                bool skip;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    skip = (bool)err;
                }
                if (!skip) write_at(fd, ring + p.s * slot, p.bytes, p.off);
            } catch (...) {
                std::lock_guard<std::mutex> lk(mu);
                if (!err) err = std::current_exception();
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                busy[p.s] = false;
            }
            cv.notify_all();
        }
    }
    // the next pinned slot, free to be copied into; null after an error (finish() rethrows it)
    uint8_t *next() {
        cur = k++ % SLOTS;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy[cur] || err; });
        if (err) return nullptr;
        busy[cur] = true;
        return ring + cur * slot;
    }
    // what the stream holds so far fills the slot of the last next(): its `bytes` go to file offset off
    void submit(uint64_t bytes, uint64_t off) {
        hipEvent_t ev;
        ST_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const hipError_t e = hipEventRecord(ev, c->stream);
        if (e != hipSuccess) (void)hipEventDestroy(ev);
        ST_HIP(e);
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back({cur, bytes, off, ev});
        }
        cv.notify_all();
    }
    void fail(std::exception_ptr e) {
        std::lock_guard<std::mutex> lk(mu);
        if (!err) err = e;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu);
            fin = true;
        }
        cv.notify_all();
        if (writer.joinable()) writer.join();
    }
    void finish() {
        stop();
        if (err) std::rethrow_exception(err);
    }
    ~FileRing() { stop(); }
};

// one piece of a file's body: `bytes` for file offset `off`; no bytes: the body has ended
struct Part {
    uint64_t bytes, off;
};

// a file's body through the ring, piece by piece: plan(k) sizes piece k (it may wait for the device
// to learn the size), source(k) queues the device work that makes the piece and returns where its
// bytes will be in HBM; the copy into the pinned slot follows them on the context's stream.  plan
// runs before the slot is waited for and source after, so a ring already in error gets no more
// work queued.  An error in here goes to the ring, whose finish() rethrows it.
template <typename Plan, typename Source>
void pump(FileRing &ring, Plan plan, Source source) {
    try {
        for (uint64_t k = 0;; ++k) {
            const Part p = plan(k);
            if (!p.bytes) break;
            uint8_t *host = ring.next();
            if (!host) break;
            const uint8_t *dev = source(k);
            ST_HIP(hipMemcpyAsync(host, dev, p.bytes, hipMemcpyDeviceToHost, ring.c->stream));
            ring.submit(p.bytes, p.off);
        }
    } catch (...) {
        ring.fail(std::current_exception());
    }
}

// bytes that lie whole in HBM to file offset `off`, one ring slot a piece
void device_bytes_to_file(FileRing &ring, const uint8_t *dev, uint64_t bytes, uint64_t off) {
    pump(
        ring,
        [&](uint64_t k) {
            const uint64_t o = k * ring.slot;
            return Part{o < bytes ? std::min(ring.slot, bytes - o) : 0, off + o};
        },
        [&](uint64_t k) { return dev + k * ring.slot; });
}

// the output's first byte: the descriptor's position, as the reference's FileHandle.write calls go
// (the CLI's fresh output: 0)
uint64_t file_base(int fd, const char *what) {
    const off_t pos = lseek(fd, 0, SEEK_CUR);
    ST_REQUIRE(pos >= 0, ST_ERR_ARG, std::string(what) + ": the descriptor has no position");
    return (uint64_t)pos;
}

// the file ends at the output's last byte, and the position is left there
void file_end(int fd, uint64_t total, const char *what) {
    sog_file_truncate(fd, total);
    ST_REQUIRE(lseek(fd, (off_t)total, SEEK_SET) == (off_t)total, ST_ERR_ARG, std::string(what) + ": lseek failed");
}

// writeCompressedPly's arrays of the chain's table, in workspace slots: m rows, C coefficients a channel
struct CplyArrays {
    uint64_t m;
    int32_t C;
    float *chunk;
    uint32_t *vert;
    uint8_t *sh;
};
CplyArrays compressed_arrays(Chain &ch) {
    st_ctx *c = ch.c;
    const uint64_t m = ch.n, nch = (m + 255) / 256;
    CplyArrays a{m, 0, wsT<float>(c, "chain.chunk", nch * 18), wsT<uint32_t>(c, "chain.vert", m * 4),
                 wsT<uint8_t>(c, "chain.sh", m * 3 * (uint64_t)ch.coeffs() + 1)};
    compressed_tail(ch, a.chunk, a.vert, a.sh, &a.C);
    return a;
}

// what follows the header in a .compressed.ply file (write-compressed-ply.ts:112-114): the chunk,
// vertex and sh arrays in HBM, in file order, the empty ones left out; `off` = a region's first
// byte counted from the header's end
struct Region {
    const uint8_t *dev;
    uint64_t bytes, off;
};
std::vector<Region> compressed_ply_regions(const CplyArrays &a) {
    const uint64_t nch = (a.m + 255) / 256;
    std::vector<Region> rs;
    uint64_t off = 0;
    for (const Region &r : {Region{reinterpret_cast<const uint8_t *>(a.chunk), nch * 72, 0},
                            Region{reinterpret_cast<const uint8_t *>(a.vert), a.m * 16, 0},
                            Region{a.sh, a.C ? a.m * 3 * (uint64_t)a.C : 0, 0}}) {
        if (r.bytes) rs.push_back({r.dev, r.bytes, off});
        off += r.bytes;
    }
    return rs;
}

// the device arrays to fd at offsets from its position through the ring (one writer thread for
// the whole file); the file ends at the last byte
uint64_t compressed_ply_to_file(st_ctx *c, const CplyArrays &a, int fd, const char *version) {
    const std::string head = compressed_ply_header(a.m, a.C, version);
    const uint64_t base = file_base(fd, "compressed ply file");
    write_at(fd, reinterpret_cast<const uint8_t *>(head.data()), head.size(), base);
    const std::vector<Region> rs = compressed_ply_regions(a);
    const uint64_t body = base + head.size();
    const uint64_t total = body + (rs.empty() ? 0 : rs.back().off + rs.back().bytes);
    FileRing ring(c, fd);
    for (const Region &r : rs) device_bytes_to_file(ring, r.dev, r.bytes, body + r.off);
    ring.finish();
    file_end(fd, total, "compressed ply file");
    return total - base;
}

// writeHtml's file (write-html.ts:51-57) to fd from its position: the page's prefix, the base64 text
// of header | chunk | vertex | sh, its suffix.  The compressed file is a virtual stream over the
// header (uploaded) and the arrays where compressed_tail left them; a piece is one ring slot of text
// (slot / 4 * 3 stream bytes) encoded into one of two device staging buffers, then copied into the
// slot while the writer thread writes the slot before.  A page without fetch(contentUrl) is written
// alone.
uint64_t html_to_file(st_ctx *c, const HtmlParts &page, const CplyArrays &a, int fd, const char *version) {
    const uint64_t base = file_base(fd, "html file");
    write_at(fd, reinterpret_cast<const uint8_t *>(page.prefix.data()), page.prefix.size(), base);
    uint64_t total = base + page.prefix.size();
    if (page.embeds) {
        const std::string head = compressed_ply_header(a.m, a.C, version);
        auto *dhead = wsT<uint8_t>(c, "htmlw.head", head.size());
        ST_HIP(hipMemcpyAsync(dhead, head.data(), head.size(), hipMemcpyHostToDevice, c->stream));
        ST_HIP(hipStreamSynchronize(c->stream));  // (head is pageable and leaves with this scope)
        std::vector<st_bytes_seg> segs{{dhead, head.size()}};
        uint64_t bytes = head.size();
        for (const Region &r : compressed_ply_regions(a)) {
            segs.push_back({r.dev, r.bytes});
            bytes += r.bytes;
        }
        FileRing ring(c, fd);
        const uint64_t piece = ring.slot / 4 * 3;  // a multiple of 3: the slot is whole MiB
        uint8_t *stage[2] = {wsT<uint8_t>(c, "htmlw.stage0", ring.slot), wsT<uint8_t>(c, "htmlw.stage1", ring.slot)};
        uint64_t b = 0, nb = 0;  // the piece's first stream byte and its stream bytes
        pump(
            ring,
            [&](uint64_t k) {
                b = k * piece, nb = b < bytes ? std::min(piece, bytes - b) : 0;
                return Part{base64_size(nb), total + b / 3 * 4};
            },
            [&](uint64_t k) {
                base64_dev(c, segs.data(), (int)segs.size(), b, nb, stage[k & 1]);
                return stage[k & 1];
            });
        ring.finish();
        total += base64_size(bytes);
        write_at(fd, reinterpret_cast<const uint8_t *>(page.suffix.data()), page.suffix.size(), total);
        total += page.suffix.size();
    }
    file_end(fd, total, "html file");
    return total - base;
}

// writePly's rows (write-ply.ts:37-67) of a device table to fd at file offset `off`: rows are
// interleaved piece by piece (whole workgroups of rows, one ring slot each) into two device staging
// buffers and come down through the ring -- the m * R bytes never exist in HBM at once.  Returns
// the bytes written.
uint64_t ply_rows_to_file(st_ctx *c, const st_ttable *t, int fd, uint64_t off) {
    PlyRows pr(c, t, "plyw");
    if (!t->n || !pr.R) return 0;
    FileRing ring(c, fd);
    const uint64_t per = (uint64_t)pr.RB * pr.R;  // <= 48 KiB
    const uint64_t piece_rows = std::max<uint64_t>(1, ring.slot / per) * pr.RB;
    uint8_t *stage[2] = {wsT<uint8_t>(c, "plyw.stage0", piece_rows * pr.R), wsT<uint8_t>(c, "plyw.stage1", piece_rows * pr.R)};
    uint64_t row = 0, nr = 0;
    pump(
        ring,
        [&](uint64_t k) {
            row = k * piece_rows, nr = row < t->n ? std::min(piece_rows, t->n - row) : 0;
            return Part{nr * pr.R, off + row * pr.R};
        },
        [&](uint64_t k) {
            pr.run(row, nr, stage[k & 1]);
            return stage[k & 1];
        });
    ring.finish();
    return t->n * pr.R;
}

// `head` (a header, or nothing: an element's rows alone) + the table's rows to fd from its position
uint64_t ply_table_to_file(st_ctx *c, const std::string &head, const st_ttable *t, int fd) {
    const uint64_t base = file_base(fd, "ply file");
    write_at(fd, reinterpret_cast<const uint8_t *>(head.data()), head.size(), base);
    const uint64_t total = base + head.size() + ply_rows_to_file(c, t, fd, base + head.size());
    file_end(fd, total, "ply file");
    return total - base;
}

// writeCsv's rows (write-csv.ts:15-22) of a device table to fd at file offset `off`: a piece is as
// many rows as fit one ring slot by the worst-case row width; its length pass and scan run first
// and its byte count is read back (submit() needs it and the next piece's file offset), then the
// text goes into one of two device staging buffers and down through the ring while the writer
// thread writes the slot before.  Returns the bytes written.
uint64_t csv_rows_to_file(st_ctx *c, CsvRows &cr, const st_ttable *t, int fd, uint64_t off) {
    if (!t->n) return 0;
    FileRing ring(c, fd);
    const uint64_t piece_rows = cr.piece_rows(std::min<uint64_t>(ring.slot, CSV_PIECE_BYTES));
    const uint64_t stage_bytes = piece_rows * cr.W + 8;
    uint8_t *stage[2] = {wsT<uint8_t>(c, "csvw.stage0", stage_bytes), wsT<uint8_t>(c, "csvw.stage1", stage_bytes)};
    uint64_t row = 0, nr = 0, next = off;  // the piece's rows; the file offset after the pieces measured so far
    pump(
        ring,
        [&](uint64_t k) {
            row = k * piece_rows;
            if (row >= t->n) return Part{0, next};
            nr = std::min(piece_rows, t->n - row);
            const Part p{cr.measure(row, nr), next};
            next += p.bytes;
            return p;
        },
        [&](uint64_t k) {
            cr.write(row, nr, stage[k & 1], 0);
            return stage[k & 1];
        });
    ring.finish();
    return next - off;
}

// header + rows of a device table to out_fd from its position (writeCsv, index.ts:117-118)
uint64_t csv_table_to_file(st_ctx *c, const st_ttable *t, int fd) {
    const std::string head = csv_header_text(t);
    const uint64_t base = file_base(fd, "csv file");
    CsvRows cr(c, t, "csvw");  // the table's own errors before the first byte is written
    write_at(fd, reinterpret_cast<const uint8_t *>(head.data()), head.size(), base);
    const uint64_t total = base + head.size() + csv_rows_to_file(c, cr, t, fd, base + head.size());
    file_end(fd, total, "csv file");
    return total - base;
}

// the .splat rows of a device table to fd from its position: pieces of one ring slot of 32-byte
// rows are encoded into two device staging buffers and come down through the ring -- the n x 32
// bytes never exist in HBM at once.  The table's own errors come before the first byte is written
uint64_t splat_table_to_file(st_ctx *c, const st_ttable *t, int fd) {
    const WrTable W = wr_table(t, false, "splat file");
    ST_REQUIRE(W.n != 0, ST_ERR_ARG, "splat file: a .splat file of no rows is one the reader refuses");
    const uint64_t base = file_base(fd, "splat file");
    {
        FileRing ring(c, fd);
        const uint64_t piece_rows = std::max<uint64_t>(1, ring.slot / 32);
        uint8_t *stage[2] = {wsT<uint8_t>(c, "splatw.stage0", piece_rows * 32), wsT<uint8_t>(c, "splatw.stage1", piece_rows * 32)};
        uint64_t row = 0, nr = 0;
        pump(
            ring,
            [&](uint64_t k) {
                row = k * piece_rows, nr = row < W.n ? std::min(piece_rows, W.n - row) : 0;
                return Part{nr * 32, base + row * 32};
            },
            [&](uint64_t k) {
                splat_rows_dev(c, W, row, nr, stage[k & 1]);
                return stage[k & 1];
            });
        ring.finish();
    }
    file_end(fd, base + W.n * 32, "splat file");
    return W.n * 32;
}

// an image that lies whole in HBM to fd from `base`, the position it was found at
void image_to_file(st_ctx *c, const uint8_t *image, uint64_t size, int fd, uint64_t base, const char *what) {
    {
        FileRing ring(c, fd);
        device_bytes_to_file(ring, image, size, base);
        ring.finish();
    }
    file_end(fd, base + size, what);
}

// the raw .spz image (header + six planes) of a device table to fd from its position: built whole
// in HBM -- it is smaller than the table it comes from -- and copied down through the ring.  gz: the
// gzip member around the image (st_deflate.hip), made in HBM beside it, is what goes down
uint64_t spz_table_to_file(st_ctx *c, const st_ttable *t, int fractional_bits, int fd, uint64_t *clamped, bool gz) {
    const WrTable W = wr_table(t, true, "spz file");
    spz_check(W, fractional_bits);
    const uint64_t base = file_base(fd, "spz file");
    uint64_t size = spz_image_size(W.n, W.C);
    auto *image = wsT<uint8_t>(c, "spzw.image", size);
    spz_image_dev(c, W, fractional_bits, image, clamped);
    if (gz) {
        const uint64_t cap = st_gzip_bound(size);
        auto *member = wsT<uint8_t>(c, "spzw.gz", cap);
        size = gzip_dev(c, image, size, member, cap);
        image = member;
    }
    image_to_file(c, image, size, fd, base, "spz file");
    return size;
}

// the .ksplat image (headers, bucket tables, records) of a device table to fd from its position: built
// whole in HBM -- it is smaller than the table it comes from -- and copied down through the ring
uint64_t ksplat_table_to_file(st_ctx *c, const st_ttable *t, int mode, int degree, float block_size, float sh_min,
                              float sh_max, int fd, uint64_t *clamped) {
    const WrTable W = wr_table(t, true, "ksplat file");
    const KswParams P = ksplat_params(W, mode, degree, block_size, sh_min, sh_max);
    const uint64_t base = file_base(fd, "ksplat file");
    const KswPlan K = ksplat_plan_begin(c, W, P.B);
    if (clamped) *clamped = K.clamped;
    const uint64_t size = ksplat_plan_image_size(K, P);
    auto *image = wsT<uint8_t>(c, "ksw.image", size);
    ksplat_image_from_plan(c, W, P, K, image);
    image_to_file(c, image, size, fd, base, "ksplat file");
    return size;
}

// ---- where a one-call form's table comes from -----------------------------------------------
// ok(): the source's own arguments are there (else "NULL argument"); check(): the table's errors
// that need no device; load(): the table into the chain's device columns; table(): the processed
// table as a writer takes it.

// a host table, uploaded once
struct HostSrc {
    const st_ttable *t;
    bool ok() const { return t; }
    void check() const { check_src(t); }
    void load(Chain &ch) const { upload_chain(ch.c, t, ch); }
    const st_ttable *table(Chain &ch) const { return ch.typed(); }
};

// an element of a .ply file behind a descriptor, read straight into HBM
struct PlySrc {
    int32_t fd;
    const st_ply_header *h;
    int32_t element;
    bool ok() const { return h && fd >= 0; }
    void check() const {}
    void load(Chain &ch) const { ply_chain(ch.c, fd, h, element, ch); }
    const st_ttable *table(Chain &ch) const { return ch.typed(); }
};

// a table already in HBM.  Its forms take no actions and the writer gets the caller's st_ttable as
// it is: a column name may be NULL there (check_src and wr_table allow it), which a ChainCol's
// std::string cannot hold, so the chain learns the row count alone
struct DevSrc {
    const st_ttable *t;
    bool ok() const { return t; }
    void check() const { check_src(t); }
    void load(Chain &ch) const { ch.n = t->n; }
    const st_ttable *table(Chain &) const { return t; }
};

// a one-call file form: the source's table, the actions, the format's writer into out_fd.  A
// caller sees the checks in this order: NULL arguments, the format's parameters (`pre`), the
// source table, the output descriptor; the device comes after all of them.  write(chain, table)
// returns the bytes written.  (A device form has no row count to report: it passes a local.)
template <typename Src, typename Pre, typename Write>
void file_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t out_fd, uint64_t *out_m,
               uint64_t *size, Pre pre, Write write) {
    ST_REQUIRE(c && src.ok() && out_m && size && (actions || nactions == 0), ST_ERR_ARG, "NULL argument");
    pre();
    src.check();
    sog_file_check(out_fd);
    use_device(c);
    Chain ch{c};
    src.load(ch);
    run_actions(ch, actions, nactions);
    *size = write(ch, src.table(ch));
    *out_m = ch.n;
}

// the forms of each format: its parameter checks and its writer around file_form
template <typename Src>
int html_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, const char *html, const char *css,
              const char *js, const double *camera, const double *target, int32_t out_fd, const char *version,
              uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size) {
    return guard([&] {
        HtmlParts page;
        file_form(
            c, src, actions, nactions, out_fd, out_m, size,
            [&] {
                ST_REQUIRE(out_sh_coeffs, ST_ERR_ARG, "NULL argument");
                page = html_parts(html, css, js, camera, target);
            },
            [&](Chain &ch, const st_ttable *) {
                const CplyArrays a = compressed_arrays(ch);
                const uint64_t bytes = html_to_file(c, page, a, out_fd, version);
                *out_sh_coeffs = a.C;
                return bytes;
            });
    });
}

// the rows alone (no header, no actions)
template <typename Src>
int ply_rows_form(st_ctx *c, const Src &src, int32_t out_fd, uint64_t *size) {
    return guard([&] {
        uint64_t rows;
        file_form(c, src, nullptr, 0, out_fd, &rows, size, [] {},
                  [&](Chain &, const st_ttable *t) { return ply_table_to_file(c, "", t, out_fd); });
    });
}

// writePly with one element named "vertex" (index.ts:126-133)
template <typename Src>
int ply_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, const char *const *comments,
             int32_t ncomments, int32_t out_fd, uint64_t *out_m, uint64_t *size) {
    return guard([&] {
        file_form(
            c, src, actions, nactions, out_fd, out_m, size,
            [&] { ST_REQUIRE(ncomments >= 0 && (comments || ncomments == 0), ST_ERR_ARG, "ply file: NULL comments"); },
            [&](Chain &, const st_ttable *t) {
                return ply_table_to_file(c, ply_header_text(t, "vertex", comments, ncomments, false), t, out_fd);
            });
    });
}

template <typename Src>
int csv_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t out_fd, uint64_t *out_m,
             uint64_t *size) {
    return guard([&] {
        file_form(c, src, actions, nactions, out_fd, out_m, size, [] {},
                  [&](Chain &, const st_ttable *t) { return csv_table_to_file(c, t, out_fd); });
    });
}

template <typename Src>
int splat_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t out_fd, uint64_t *out_m,
               uint64_t *size) {
    return guard([&] {
        file_form(c, src, actions, nactions, out_fd, out_m, size, [] {},
                  [&](Chain &, const st_ttable *t) { return splat_table_to_file(c, t, out_fd); });
    });
}

// gz: the gzip member around the image, deflated on the device
template <typename Src>
int spz_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t fractional_bits,
             int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped, bool gz) {
    return guard([&] {
        file_form(
            c, src, actions, nactions, out_fd, out_m, size,
            [&] {
                ST_REQUIRE(fractional_bits >= 0 && fractional_bits <= 23, ST_ERR_ARG, "spz: fractional_bits must be 0..23");
            },
            [&](Chain &, const st_ttable *t) { return spz_table_to_file(c, t, fractional_bits, out_fd, out_clamped, gz); });
    });
}

template <typename Src>
int ksplat_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t mode, int32_t degree,
                float block_size, float sh_min, float sh_max, int32_t out_fd, uint64_t *out_m, uint64_t *size,
                uint64_t *out_clamped) {
    return guard([&] {
        file_form(
            c, src, actions, nactions, out_fd, out_m, size,
            [&] {  // the parameter checks that need no table (the table's own follow in ksplat_params)
                ST_REQUIRE(mode >= 0 && mode <= 2, ST_ERR_ARG, "ksplat: mode must be 0, 1 or 2");
                ST_REQUIRE(degree >= -1 && degree <= 3, ST_ERR_ARG, "ksplat: degree must be -1..3");
                ST_REQUIRE(block_size > 0.0f && block_size < __builtin_inff(), ST_ERR_ARG,
                           "ksplat: block_size must be finite and > 0 as a float32");
            },
            [&](Chain &, const st_ttable *t) {
                return ksplat_table_to_file(c, t, mode, degree, block_size, sh_min, sh_max, out_fd, out_clamped);
            });
    });
}

// processDataTable + writeCompressedPly's arrays into the caller's host arrays
template <typename Src>
int compressed_ply_arrays_form(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, float *chunk,
                               uint32_t *vertex, uint8_t *sh, uint64_t *out_m, int32_t *out_sh_coeffs) {
    return guard([&] {
        ST_REQUIRE(c && src.ok() && out_m && out_sh_coeffs && (actions || nactions == 0), ST_ERR_ARG, "NULL argument");
        src.check();
        use_device(c);
        Chain ch{c};
        src.load(ch);
        run_actions(ch, actions, nactions);
        ST_REQUIRE(ch.n == 0 || (chunk && vertex), ST_ERR_ARG, "compressed_ply: NULL output");
        const CplyArrays a = compressed_arrays(ch);
        ST_REQUIRE(a.C == 0 || a.m == 0 || sh, ST_ERR_ARG, "compressed_ply: sh output is NULL");
        std::vector<HostXfer> down;
        if (a.m) {
            down.push_back(HostXfer{chunk, a.chunk, (a.m + 255) / 256 * 72});
            down.push_back(HostXfer{vertex, a.vert, a.m * 16});
            if (a.C) down.push_back(HostXfer{sh, a.sh, a.m * 3 * (uint64_t)a.C});
        }
        staged_d2h(c, down);
        *out_m = a.m;
        *out_sh_coeffs = a.C;
    });
}

// processDataTable + writeSog on the source's table, into the sink.  One device takes every
// column type (sog_tdev); with the st_set_devices group the processed float32 columns are
// sharded over it from the host.
template <typename Src>
void sog_chain(st_ctx *c, const Src &src, const st_action *actions, int32_t nactions, int32_t iters,
               const double *draws, uint64_t ndraws, uint64_t *used, const SogSink &to) {
    const auto group = sog_group();  // held for the whole call
    ST_ARG(c && to.ok(), "NULL argument");
    ST_ARG(actions || nactions == 0, "NULL argument");
    use_device(c);
    ST_ARG(src.ok(), "NULL argument");
    src.check();
    Chain ch{c};
    src.load(ch);
    run_actions(ch, actions, nactions);
    if (group) {
        const st_table *t = sog_view(ch);
        std::vector<std::vector<float>> host;  // the processed columns, sharded from the host
        std::vector<float *> hcols;
        std::vector<HostXfer> down;
        for (int i = 0; i < t->ncol; ++i) {
            host.emplace_back(t->n);
            down.push_back(HostXfer{host.back().data(), t->cols[i], t->n * 4});
        }
        staged_d2h(c, down);
        for (auto &h : host) hcols.push_back(h.data());
        const st_table ht{t->n, t->ncol, t->names, hcols.data()};
        if (!ht.ncol) return;  // no float32 column left: nothing to shard
        const st_table *tp = &ht;
        return group_sog_to(group.get(), &tp, 1, nullptr, nullptr, nullptr, iters, draws, ndraws, used, to);
    }
    const st_sog_textures dt = sog_textures(c, ch.n, ch.coeffs());
    st_sog_meta meta{};
    const uint64_t u = sog_tdev(c, ch.typed(), iters, draws, ndraws, &meta, &dt);
    sog_deliver(c, dt, meta, ch.n, to);
    if (used) *used = u;
}

}  // namespace

// processDataTable on a device float32 table (transforms in place, filters into workspace slots
// under `tag`): the processed table's columns in `out`
void chain_apply_f32(st_ctx *c, const st_table *in, const st_action *actions, int nactions, const std::string &tag,
                     ProcessedF32 &out) {
    Chain ch{c};
    ch.tag = tag;
    ch.n = in->n;
    for (int i = 0; i < in->ncol; ++i) ch.cols.push_back(ChainCol{in->names[i], ST_PLY_FLOAT, in->cols[i]});
    run_actions(ch, actions, nactions);
    out.names.clear();
    out.cn.clear();
    out.cols.clear();
    for (auto &k : ch.cols) out.names.push_back(k.name), out.cols.push_back(static_cast<float *>(k.ptr));
    for (auto &nm : out.names) out.cn.push_back(nm.c_str());
    out.t = st_table{ch.n, (int32_t)out.cols.size(), out.cn.data(), out.cols.data()};
}

}  // namespace st

using namespace st;

extern "C" {

int st_process(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, const st_ttable *dst,
               uint64_t *out_m) {
    return guard([&] {
        const HostSrc host{src};
        ST_REQUIRE(c && host.ok() && dst && out_m && (actions || nactions == 0), ST_ERR_ARG, "NULL argument");
        host.check();
        use_device(c);
        Chain ch{c};
        host.load(ch);
        run_actions(ch, actions, nactions);
        std::vector<int> from(dst->ncol, -1);
        for (int j = 0; j < dst->ncol; ++j) {
            for (size_t i = 0; i < ch.cols.size() && from[j] < 0; ++i)
                if (ch.cols[i].name == dst->names[j] && ch.cols[i].type == dst->types[j]) from[j] = (int)i;
            ST_REQUIRE(from[j] >= 0, ST_ERR_ARG, std::string("process: result has no column ") + dst->names[j]);
        }
        std::vector<HostXfer> down;
        for (int j = 0; j < dst->ncol; ++j)
            down.push_back(HostXfer{dst->cols[j], ch.cols[from[j]].ptr, ch.n * type_size(dst->types[j])});
        staged_d2h(c, down);
        *out_m = ch.n;
    });
}

int st_compressed_ply(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, float *chunk,
                      uint32_t *vertex, uint8_t *sh, uint64_t *out_m, int32_t *out_sh_coeffs) {
    return compressed_ply_arrays_form(c, HostSrc{src}, actions, nactions, chunk, vertex, sh, out_m, out_sh_coeffs);
}

int st_dev_compressed_ply(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions,
                          float *chunk, uint32_t *vertex, uint8_t *sh, uint64_t *out_m, int32_t *out_sh_coeffs) {
    return guard([&] {
        ST_REQUIRE(c && src && out_m && out_sh_coeffs && (actions || nactions == 0), ST_ERR_ARG, "NULL argument");
        check_src(src);
        use_device(c);
        Chain ch{c};
        ch.n = src->n;
        for (int i = 0; i < src->ncol; ++i) ch.cols.push_back(ChainCol{src->names[i], src->types[i], src->cols[i]});
        run_actions(ch, actions, nactions);
        ST_REQUIRE(ch.n == 0 || (chunk && vertex), ST_ERR_ARG, "compressed_ply: NULL output");
        int32_t C = 0;
        if (ch.coeffs() && ch.n) ST_REQUIRE(sh, ST_ERR_ARG, "compressed_ply: sh output is NULL");
        compressed_tail(ch, chunk, vertex, sh, &C);
        *out_m = ch.n;
        *out_sh_coeffs = C;
    });
}

int st_ply_compressed_ply(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                          int32_t nactions, float *chunk, uint32_t *vertex, uint8_t *sh, uint64_t *out_m,
                          int32_t *out_sh_coeffs) {
    return compressed_ply_arrays_form(c, PlySrc{fd, h, element}, actions, nactions, chunk, vertex, sh, out_m,
                                      out_sh_coeffs);
}

// file_form's steps longhand: ST_DEBUG's stamps want the stream drained after the ingest and after
// the arrays are made, which no other form does
int st_ply_compressed_ply_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element,
                               const st_action *actions, int32_t nactions, int32_t out_fd, const char *version,
                               uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size) {
    return guard([&] {
        const PlySrc ply{fd, h, element};
        ST_REQUIRE(c && ply.ok() && out_m && out_sh_coeffs && size && (actions || nactions == 0), ST_ERR_ARG,
                   "NULL argument");
        sog_file_check(out_fd);
        use_device(c);
        using clk = std::chrono::steady_clock;
        const auto t0 = clk::now();
        Chain ch{c};
        ply.load(ch);
        ST_HIP(hipStreamSynchronize(c->stream));  // (ST_DEBUG's stamps: the ingest alone)
        const auto t1 = clk::now();
        run_actions(ch, actions, nactions);
        const CplyArrays a = compressed_arrays(ch);
        ST_HIP(hipStreamSynchronize(c->stream));
        const auto t2 = clk::now();
        *size = compressed_ply_to_file(c, a, out_fd, version);
        *out_m = a.m;
        *out_sh_coeffs = a.C;
        if (std::getenv("ST_DEBUG")) {
            const auto ms = [](clk::time_point from, clk::time_point to) {
                return std::chrono::duration<double, std::milli>(to - from).count();
            };
            fprintf(stderr, "[st cply file] ingest %.1f ms, chain %.1f ms, file %.1f ms (%llu rows)\n", ms(t0, t1),
                    ms(t1, t2), ms(t2, clk::now()), (unsigned long long)a.m);
        }
    });
}

int st_compressed_ply_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t out_fd,
                           const char *version, uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size) {
    return guard([&] {
        file_form(
            c, HostSrc{src}, actions, nactions, out_fd, out_m, size,
            [&] { ST_REQUIRE(out_sh_coeffs, ST_ERR_ARG, "NULL argument"); },
            [&](Chain &ch, const st_ttable *) {
                const CplyArrays a = compressed_arrays(ch);
                const uint64_t bytes = compressed_ply_to_file(c, a, out_fd, version);
                *out_sh_coeffs = a.C;
                return bytes;
            });
    });
}

int st_html_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, const char *html,
                 const char *css, const char *js, const double *camera, const double *target, int32_t out_fd,
                 const char *version, uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size) {
    return html_form(c, HostSrc{src}, actions, nactions, html, css, js, camera, target, out_fd, version, out_m,
                     out_sh_coeffs, size);
}

int st_ply_html_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                     int32_t nactions, const char *html, const char *css, const char *js, const double *camera,
                     const double *target, int32_t out_fd, const char *version, uint64_t *out_m,
                     int32_t *out_sh_coeffs, uint64_t *size) {
    return html_form(c, PlySrc{fd, h, element}, actions, nactions, html, css, js, camera, target, out_fd, version,
                     out_m, out_sh_coeffs, size);
}

int st_dev_ply_rows_file(st_ctx *c, const st_ttable *t, int32_t out_fd, uint64_t *size) {
    return ply_rows_form(c, DevSrc{t}, out_fd, size);
}

int st_ply_rows_file(st_ctx *c, const st_ttable *src, int32_t out_fd, uint64_t *size) {
    return ply_rows_form(c, HostSrc{src}, out_fd, size);
}

int st_ply_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions,
                const char *const *comments, int32_t ncomments, int32_t out_fd, uint64_t *out_m, uint64_t *size) {
    return ply_form(c, HostSrc{src}, actions, nactions, comments, ncomments, out_fd, out_m, size);
}

int st_ply_ply_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, const char *const *comments, int32_t ncomments, int32_t out_fd,
                    uint64_t *out_m, uint64_t *size) {
    return ply_form(c, PlySrc{fd, h, element}, actions, nactions, comments, ncomments, out_fd, out_m, size);
}

int st_dev_csv_file(st_ctx *c, const st_ttable *t, int32_t out_fd, uint64_t *size) {
    uint64_t rows;
    return csv_form(c, DevSrc{t}, nullptr, 0, out_fd, &rows, size);
}

int st_csv_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t out_fd,
                uint64_t *out_m, uint64_t *size) {
    return csv_form(c, HostSrc{src}, actions, nactions, out_fd, out_m, size);
}

int st_ply_csv_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, int32_t out_fd, uint64_t *out_m, uint64_t *size) {
    return csv_form(c, PlySrc{fd, h, element}, actions, nactions, out_fd, out_m, size);
}

int st_dev_splat_file(st_ctx *c, const st_ttable *t, int32_t out_fd, uint64_t *size) {
    uint64_t rows;
    return splat_form(c, DevSrc{t}, nullptr, 0, out_fd, &rows, size);
}

int st_splat_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t out_fd,
                  uint64_t *out_m, uint64_t *size) {
    return splat_form(c, HostSrc{src}, actions, nactions, out_fd, out_m, size);
}

int st_ply_splat_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                      int32_t nactions, int32_t out_fd, uint64_t *out_m, uint64_t *size) {
    return splat_form(c, PlySrc{fd, h, element}, actions, nactions, out_fd, out_m, size);
}

int st_dev_spz_file(st_ctx *c, const st_ttable *t, int32_t fractional_bits, int32_t out_fd, uint64_t *size,
                    uint64_t *out_clamped) {
    uint64_t rows;
    return spz_form(c, DevSrc{t}, nullptr, 0, fractional_bits, out_fd, &rows, size, out_clamped, false);
}

int st_spz_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t fractional_bits,
                int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped) {
    return spz_form(c, HostSrc{src}, actions, nactions, fractional_bits, out_fd, out_m, size, out_clamped, false);
}

int st_ply_spz_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size,
                    uint64_t *out_clamped) {
    return spz_form(c, PlySrc{fd, h, element}, actions, nactions, fractional_bits, out_fd, out_m, size, out_clamped,
                    false);
}

// the same three with the gzip member around the image, deflated on the device
int st_dev_spz_gz_file(st_ctx *c, const st_ttable *t, int32_t fractional_bits, int32_t out_fd, uint64_t *size,
                       uint64_t *out_clamped) {
    uint64_t rows;
    return spz_form(c, DevSrc{t}, nullptr, 0, fractional_bits, out_fd, &rows, size, out_clamped, true);
}

int st_spz_gz_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions,
                   int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped) {
    return spz_form(c, HostSrc{src}, actions, nactions, fractional_bits, out_fd, out_m, size, out_clamped, true);
}

int st_ply_spz_gz_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                       int32_t nactions, int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size,
                       uint64_t *out_clamped) {
    return spz_form(c, PlySrc{fd, h, element}, actions, nactions, fractional_bits, out_fd, out_m, size, out_clamped,
                    true);
}

int st_dev_ksplat_file(st_ctx *c, const st_ttable *t, int32_t mode, int32_t degree, float block_size, float sh_min,
                       float sh_max, int32_t out_fd, uint64_t *size, uint64_t *out_clamped) {
    uint64_t rows;
    return ksplat_form(c, DevSrc{t}, nullptr, 0, mode, degree, block_size, sh_min, sh_max, out_fd, &rows, size,
                       out_clamped);
}

int st_ksplat_file(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t mode,
                   int32_t degree, float block_size, float sh_min, float sh_max, int32_t out_fd, uint64_t *out_m,
                   uint64_t *size, uint64_t *out_clamped) {
    return ksplat_form(c, HostSrc{src}, actions, nactions, mode, degree, block_size, sh_min, sh_max, out_fd, out_m,
                       size, out_clamped);
}

int st_ply_ksplat_file(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                       int32_t nactions, int32_t mode, int32_t degree, float block_size, float sh_min, float sh_max,
                       int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped) {
    return ksplat_form(c, PlySrc{fd, h, element}, actions, nactions, mode, degree, block_size, sh_min, sh_max, out_fd,
                       out_m, size, out_clamped);
}

int st_ply_sog_bundle(st_ctx *c, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                      int32_t nactions, int32_t iters, const double *draws, uint64_t ndraws, uint64_t *used,
                      uint16_t dos_time, uint16_t dos_date, uint8_t **out, uint64_t *out_size) {
    return guard([&] {
        sog_chain(c, PlySrc{fd, h, element}, actions, nactions, iters, draws, ndraws, used,
                  SogSink::buffer(out, out_size, dos_time, dos_date));
    });
}

int st_sog_bundle_process(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t iters,
                          const double *draws, uint64_t ndraws, uint64_t *used, uint16_t dos_time, uint16_t dos_date,
                          uint8_t **out, uint64_t *out_size) {
    return guard([&] {
        sog_chain(c, HostSrc{src}, actions, nactions, iters, draws, ndraws, used,
                  SogSink::buffer(out, out_size, dos_time, dos_date));
    });
}

int st_sog_process(st_ctx *c, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t iters,
                   const double *draws, uint64_t ndraws, uint64_t *used, st_sog_meta *meta,
                   const st_sog_textures *out) {
    return guard([&] {
        sog_chain(c, HostSrc{src}, actions, nactions, iters, draws, ndraws, used, SogSink::textures(meta, out));
    });
}

int st_dev_sog_t(st_ctx *c, const st_ttable *t, int32_t iters, const double *draws, uint64_t ndraws, uint64_t *used,
                 st_sog_meta *meta, const st_sog_textures *out) {
    return guard([&] {
        ST_REQUIRE(c && t && meta && out, ST_ERR_ARG, "NULL argument");
        check_src(t);
        use_device(c);
        const uint64_t u = sog_tdev(c, t, iters, draws, ndraws, meta, out);
        if (used) *used = u;
    });
}

}  // extern "C"
