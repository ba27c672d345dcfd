// st_internal.h -- shared runtime pieces of libsplat_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <functional>

#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/st_abi.h"

namespace st {

// ---------------------------------------------------------------------------
// errors: internal code throws st::Error, the extern "C" boundary converts it
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string &msg);

// a host form that ran on st_ply_read's device twins of the caller's columns while the columns
// were compared with their pinned twins (st_host_api.hip: run_host_sog) stops with this when the
// compare finds a changed byte; the call then uploads the columns and runs again
struct SpecAbort : Error {
    SpecAbort() : Error(ST_ERR_INTERNAL, "speculative run abandoned: the host columns changed since st_ply_read") {}
};

#define ST_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            throw ::st::Error(ST_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ST_SYNC_CHECK=1 (read when a context is created): every launch check also synchronizes the
// device, so a kernel's fault is reported at the launch that caused it (debugging)
extern bool g_sync_check;
#define ST_LAUNCH_CHECK()                                       \
    do {                                                        \
        ST_HIP(hipGetLastError());                              \
        if (::st::g_sync_check) ST_HIP(hipDeviceSynchronize()); \
    } while (0)

#define ST_REQUIRE(cond, code, msg)                  \
    do {                                             \
        if (!(cond)) throw ::st::Error((code), (msg)); \
    } while (0)
#define ST_ARG(cond, msg) ST_REQUIRE(cond, ST_ERR_ARG, msg)

// runs f at the extern "C" boundary: st::Error -> its code + st_last_error()
template <typename F>
inline int guard(F &&f) {
    try {
        f();
        return ST_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("host allocation failed");
        return ST_ERR_NOMEM;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return ST_ERR_INTERNAL;
    }
}

// ---------------------------------------------------------------------------
// grow-only device workspace, one buffer per named slot
struct Workspace {
    struct Buf {
        void *ptr = nullptr;
        size_t bytes = 0;
    };
    std::map<std::string, Buf> bufs;
    void *get(const std::string &slot, size_t bytes);
    void release();
};

struct StageTimer {
    hipEvent_t ev;
    std::string name;
};

}  // namespace st

struct st_ctx {
    int device = 0;
    // max |x| over the k-means point set, found by check_finite in the same pass as the
    // finiteness test (negative: not known, nd_prepare computes it)
    float km_absmax = -1.0f;
    // the next kmeans_dev's points are finite by construction (the SOG writer's codebook over
    // the SH centroids: data rows and means of finite rows): no finiteness pass and read-back
    bool km_finite_known = false;
    // the N-D k-means point set prepared by nd_prepare (fp16 scale and shape)
    float kn_sigma = 1.0f;
    uint64_t kn_n = 0;
    int kn_d = 0;
    // the last st_dev_kmeans_partials call (member lists kept for st_dev_kmeans_seqsum)
    int ds_nseg = 0, ds_k = 0, ds_d = 0;
    uint64_t ds_n = 0;
    // 1-D partials taken without the member sort (dist_assign_partials1d): the (segment,
    // label) order is built from these only if a pending chain needs it
    const float *ds_pts = nullptr;
    const uint32_t *ds_labels = nullptr;
    bool ds_sorted = true;
    // 1-D k-means: read the uncertified-cluster count back every iteration (set for a rerun
    // after ERR_K1_MANY)
    bool k1_sync = false;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // a second stream of this context (side_stream): independent work of one call that
    // overlaps latency-bound chains on `stream`, joined by the two events
    hipStream_t side = nullptr;
    hipEvent_t side_ev[2] = {nullptr, nullptr};
    // the N-D assign's read-backs: behind the sweep, behind the fix-up (created on first use)
    hipEvent_t kn_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    st::Workspace ws;
    // pinned host staging for small readbacks
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    // named pinned host buffers (pinned_slot): readbacks queued ahead of the sync that waits for them
    std::map<std::string, std::pair<void *, size_t>> pinned_slots;
    // pinned host buffer of the last .sog archive (st_dev_sog_bundle*)
    void *archive = nullptr;
    size_t archive_bytes = 0;
    // pinned host chunks of the PLY reader
    void *io = nullptr;
    size_t io_bytes = 0;
    // staged host <-> device copies of pageable buffers (staged_h2d / staged_d2h): pinned
    // slots, their events and the host threads that fill / drain them
    void *xfer = nullptr;
    hipEvent_t xfer_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void *xfer_pool = nullptr;
    std::vector<st::StageTimer> marks;
    bool timing = false;
    std::string last_timings = "{}";
    // the N-D assign's classification summed over the last N-D kmeans_dev call's iterations
    // (st_ctx_last_kmeans_stats): points the sweep decided, pair points, ambiguous points, those
    // whose first candidate list overflowed, those the second list did not hold either (the
    // KdTree walk), and the exact ties walked
    struct KnStats {
        uint64_t assigns = 0, points = 0, pairs = 0, ambiguous = 0, overflow = 0, walked_overflow = 0, ties = 0;
    } kn_stats;
    std::string last_kn_stats = "{}";
    // the last column summary's sum paths (st_ctx_last_summary_stats)
    std::string last_summary_stats = "{}";
    // the last neighbour search's sizes and work (st_ctx_last_neighbor_stats)
    std::string last_neighbor_stats = "{}";
    // the last cluster search's sizes and work (st_ctx_last_cluster_stats)
    std::string last_cluster_stats = "{}";
    // kernel profiling (st_ctx_set_profiling)
    bool profiling = false;
    struct KEv {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<KEv> kevents;
    std::vector<hipEvent_t> event_pool;
    // side context on the same device (multi-GPU writeSog: rank 0's Morton order runs there)
    st_ctx *aux = nullptr;
    // called by the SOG step once the five textures that precede the SH k-means are queued on
    // the stream (sog_file_dev streams them to the file meanwhile); empty otherwise
    std::function<void(st_ctx *)> sog_early;
    // st_ctx_set_verify: snapshot of the last N-D k-means (prev / final centroids, labels)
    bool verify = false;
    int vf_d = 0, vf_k = 0;
    uint64_t vf_n = 0;
    // host columns whose values are also resident in HBM (workspace slots "plyh.e<element>.c<p>"):
    //  * st_ply_read filled `host` and a host twin `shadow` (every byte as the device copy has it):
    //    the writeSog host forms run on `dev` while other threads compare `host` with `shadow`
    //    (exact: memcmp); a changed byte sends the call back to an upload (st_host_api.hip).  The
    //    twins share one buffer: dropped by the next st_ply_read.  ST_HOST_MIRROR=0: off.
    //  * st_ply_read_resident left `host` unfilled (`lazy`): the values exist only in `dev`, a device
    //    block of the mirror's own (`dev_bytes`), until st_ply_materialize copies them down (the
    //    mirror is then dropped: the caller may change them).  The writeSog host forms read `dev`
    //    directly; every other host form materializes first (the staged copies' bookkeeping).
    //    Only this context can: every lazy range is also in the process-wide record (lazy_range_add),
    //    and another context's upload of one is refused.  st_ply_forget drops one whose host memory goes away.  A dropped mirror's block goes to
    //    dev_pool for the next resident read's columns of the same size (freed with the context).
    // mirror_mu guards the list and the pool (the Node addon's finalizers call st_ply_forget from
    // any thread).
    struct HostMirror {
        const void *host;
        uint64_t bytes;
        const void *shadow;  // null when lazy
        const void *dev;
        int element;
        bool lazy;
        uint64_t dev_bytes;  // > 0: dev is this mirror's own block (lazy), returned to dev_pool when dropped
    };
    std::vector<HostMirror> mirrors;
    std::vector<std::pair<void *, uint64_t>> dev_pool;
    std::mutex mirror_mu;
    void *shadow = nullptr;  // the mirrors' host twins (pageable, huge pages, grow-only)
    size_t shadow_bytes = 0;
    // set while a host form runs on mirrors: the compare raises *spec_abort on a mismatch (the
    // N-D k-means checks it every iteration), spec_verdict waits for the compare (true = equal)
    std::atomic<bool> *spec_abort = nullptr;
    std::function<bool()> spec_verdict;
    uint64_t last_reuse_cols = 0, last_reuse_bytes = 0;  // st_ctx_last_host_reuse
    // set by the one-device N-D k-means loop: an assign's pair / ambiguous fix-ups run on the side
    // stream beside the decided points' fix-up (nd_assign_core); ST_FIX_SERIAL=1: one stream
    bool fix_overlap = false;
};

namespace st {

inline void *ws(st_ctx *c, const std::string &slot, size_t bytes) { return c->ws.get(slot, bytes); }
template <typename T>
inline T *wsT(st_ctx *c, const std::string &slot, size_t count) {
    return static_cast<T *>(c->ws.get(slot, count * sizeof(T) + 16));
}
void *pinned(st_ctx *c, size_t bytes);  // host pinned scratch (reused)
hipStream_t side_stream(st_ctx *c);     // c->side, created on first use (non-blocking)
void *pinned_slot(st_ctx *c, const std::string &name, size_t bytes);  // named, grow-only
void *archive_buf(st_ctx *c, size_t bytes);  // host pinned archive buffer (reused, grow-only)
void *io_buf(st_ctx *c, size_t bytes);       // host pinned file-chunk buffer (reused, grow-only)
// copies between pageable host buffers and HBM for the one-call host forms: the bytes move
// through pinned slots that several host threads fill (drain) while the DMA engine moves the
// previous slot, instead of the runtime's single-threaded pageable staging.  Stream-ordered on
// c->stream; both return when every byte has arrived (the host buffers may be reused).
struct HostXfer {
    void *host;
    void *dev;
    size_t bytes;
};
void staged_h2d(st_ctx *c, const std::vector<HostXfer> &xs);
void staged_d2h(st_ctx *c, const std::vector<HostXfer> &xs);
// a workspace slot (16 bytes of padding) that receives `bytes` of host memory with xs' staged_h2d
inline void *ws_upload(st_ctx *c, const std::string &slot, const void *host, size_t bytes, std::vector<HostXfer> &xs) {
    void *d = ws(c, slot, bytes + 16);
    xs.push_back(HostXfer{const_cast<void *>(host), d, bytes});
    return d;
}
void staged_h2d_raw(st_ctx *c, const std::vector<HostXfer> &xs);  // without the mirrors' bookkeeping
void staged_d2h_raw(st_ctx *c, const std::vector<HostXfer> &xs);  // without the mirrors' bookkeeping
// st_ctx::HostMirror bookkeeping of the staged copies (st_ply.hip): lazy sources are copied down
// before an upload reads them; overwritten destinations stop being mirrors (a lazy one that is
// only partly overwritten is copied down first: its other rows exist nowhere else)
void mirrors_before_h2d(st_ctx *c, const std::vector<HostXfer> &xs);
void mirrors_before_d2h(st_ctx *c, const std::vector<HostXfer> &xs);
// host-side copy over the context's copy threads (large copies split; small ones inline)
void host_copy(st_ctx *c, char *dst, const char *src, size_t bytes);
// fn(t, nt) on each of the context's nt copy threads; returns when all are done
void host_parallel(st_ctx *c, const std::function<void(int, int)> &fn);
// a speculative host form's gate before it writes anything outside the device: throws SpecAbort
// when the compare found the host columns changed (waits for the compare)
inline void spec_gate(st_ctx *c) {
    if (c->spec_verdict && !c->spec_verdict()) throw SpecAbort();
}
void use_device(st_ctx *c);
void mark(st_ctx *c, const char *name);  // records a hipEvent when timing is on

// brackets one kernel launch with hipEvents when profiling is enabled
struct KTimer {
    st_ctx *c;
    hipEvent_t a = nullptr, b = nullptr;
    const char *name;
    hipStream_t s;  // the stream the timed kernels run on (the context's unless given)
    KTimer(st_ctx *ctx, const char *nm, hipStream_t stream = nullptr);
    ~KTimer();
};

inline unsigned grid_for(uint64_t work, unsigned per_block, unsigned cap = 1u << 30) {
    uint64_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// ---------------------------------------------------------------------------
// primitives (st_prims.hip)

// exclusive scan of n u32 values (out may alias in); returns nothing, total written to *d_total if not null
void scan_u32(st_ctx *c, const uint32_t *in, uint32_t *out, uint64_t n, uint32_t *d_total);

// stable LSD radix sort of (key, value) pairs on bits [begin_bit, end_bit)
void radix_sort_u32(st_ctx *c, uint32_t *keys, uint32_t *vals, uint64_t n, int begin_bit, int end_bit,
                    const std::string &tag);
// the same from read-only keys with the identity permutation as values, into out_keys / out_vals
void radix_sort_u32_iota(st_ctx *c, const uint32_t *in_keys, uint64_t n, int begin_bit, int end_bit,
                         uint32_t *out_keys, uint32_t *out_vals, const std::string &tag);
// the general form: in_vals null = the identity permutation; out_vals may alias in_vals when the
// pass count is even (the first pass writes the scratch pair).  hist0, when not null, holds the
// first digit's per-tile counts in the sort's layout (count of digit d in tile t at
// d * radix_tiles(n) + t, tiles of RADIX_TILE elements), produced by the caller's key kernel;
// it is scanned in place and reused as the histogram buffer of the later passes
constexpr int RADIX_TILE = 4096;
inline uint32_t radix_tiles(uint64_t n) { return (uint32_t)((n + RADIX_TILE - 1) / RADIX_TILE); }
void radix_sort_u32_from(st_ctx *c, const uint32_t *in_keys, const uint32_t *in_vals, uint64_t n, int begin_bit,
                         int end_bit, uint32_t *out_keys, uint32_t *out_vals, uint32_t *hist0, const std::string &tag);
// as radix_sort_u32, but the result stays in whichever buffer pair the last pass wrote
// (the caller's or the workspace's): *out_keys / *out_vals point at it
void radix_sort_u32_inplace_or_swap(st_ctx *c, uint32_t *keys, uint32_t *vals, uint64_t n, int b0, int b1,
                                    const std::string &tag, uint32_t **out_keys, uint32_t **out_vals);
void radix_sort_u64(st_ctx *c, uint64_t *keys, uint32_t *vals, uint64_t n, int begin_bit, int end_bit,
                    const std::string &tag);

// iota
// min and max of each column as order-preserving u32 keys (NaN ignored; an all-NaN or empty
// column gives min 0xffffffff, max 0): out[2a] = min, out[2a + 1] = max.  cols: host array of
// device pointers, ncols <= 64
void minmax_keys_dev(st_ctx *c, const float *const *cols, int ncols, uint64_t n, uint32_t *out);
void iota_u32(st_ctx *c, uint32_t *out, uint64_t n);

// column lookups on an st_table
int find_col(const st_table *t, const char *name);
float *col_or_null(const st_table *t, const char *name);
// band rule (transform.ts:20 / write-sog.ts:296): the SH coefficients per channel from the first
// f_rest_i that `has` does not find -- { '9': 1, '24': 2, '-1': 3 }[index] ?? 0 bands: 3, 8, 15 or 0
int band_coeffs(const std::function<bool(const char *)> &has);
int sh_coeffs_of(const st_table *t);  // of one table's columns

// module entry points (device pointers)
void transform_dev(st_ctx *c, const st_table *t, const st_transform_params *p);
uint64_t filter_finite_dev(st_ctx *c, const st_table *t, uint32_t *out_idx);
void permute_rows_dev(st_ctx *c, const st_table *src, const uint32_t *idx, uint64_t m, const st_table *dst);
void concat_rows_dev(st_ctx *c, const st_table *const *srcs, int nsrc, const st_table *dst);
// typed tables (st_table.hip)
int type_size(int32_t st_ply_type);  // 0 for an unknown code
uint64_t filter_finite_tdev(st_ctx *c, const st_ttable *t, uint32_t *out_idx);
// stable compaction: out_idx = the rows with flags[i] != 0, ascending; returns their count (syncs)
uint64_t compact_flags_dev(st_ctx *c, const uint32_t *flags, uint64_t n, uint32_t *out_idx);
uint64_t filter_value_tdev(st_ctx *c, const st_ttable *t, const char *column, int32_t cmp, double value,
                           uint32_t *out_idx);
void permute_rows_tdev(st_ctx *c, const st_ttable *src, const uint32_t *idx, uint64_t m, const st_ttable *dst);
// importance, decimation and crops (st_importance.hip; the rules: st_importance.h).  Workspace slots
// go under `tag`.  importance_require: ST_ERR_ARG unless t has scale_0..2 and opacity (no launch).
// importance_top_tdev wants 0 < m < n.  The crops and the top return the kept rows' count (sync)
void importance_require(const st_ttable *t, const char *what);
void importance_scores_tdev(st_ctx *c, const st_ttable *t, double *scores);
void importance_order_tdev(st_ctx *c, const st_ttable *t, const std::string &tag, uint32_t *out_idx);
uint64_t importance_top_tdev(st_ctx *c, const st_ttable *t, uint64_t m, const std::string &tag, uint32_t *out_idx);
uint64_t filter_box_tdev(st_ctx *c, const st_ttable *t, const double lo[3], const double hi[3], const std::string &tag,
                         uint32_t *out_idx);
uint64_t filter_sphere_tdev(st_ctx *c, const st_ttable *t, const double centre[3], double radius,
                            const std::string &tag, uint32_t *out_idx);
uint64_t decimate_rows_checked(const st_action &act, uint64_t n);  // decimate's m, or ST_ERR_ARG
// neighbour distances and outliers (st_neighbors.hip; the rules: st_neighbors.h).  Workspace slots go
// under `tag`.  neighbors_require: ST_ERR_ARG unless t has x, y and z and k is in 1..32 (no launch);
// outliers_require: that, and the action's mode and value.  neighbor_dist_tdev queues dist_k of every
// row into dist (n doubles) and waits once on the way (the placed count).  filter_outliers_tdev:
// the kept rows ascending into out_idx, their count returned (sync)
void neighbors_require(const st_ttable *t, int32_t k, const char *what);
void outliers_require(const st_ttable *t, const st_action &act);
void neighbor_dist_tdev(st_ctx *c, const st_ttable *t, int32_t k, const std::string &tag, double *dist);
uint64_t filter_outliers_tdev(st_ctx *c, const st_ttable *t, const st_action &act, const std::string &tag,
                              uint32_t *out_idx);
// clusters (st_clusters.hip; the rules: st_clusters.h), over the same tree (st_nbtree.h).  Workspace
// slots go under `tag`.  clusters_require: ST_ERR_ARG unless t has x, y and z and the radius is >= 0
// (no launch); filter_clusters_require: that, and the action's mode and minimum.  clusters_tdev:
// label and size of every row (n uint32 each, either may be null); it waits for the stream, leaves
// st_ctx_last_cluster_stats and returns the largest size.  filter_clusters_tdev: the kept rows
// ascending into out_idx, their count returned (sync)
void clusters_require(const st_ttable *t, double radius, const char *what);
void filter_clusters_require(const st_ttable *t, const st_action &act);
uint32_t clusters_tdev(st_ctx *c, const st_ttable *t, double radius, const std::string &tag, uint32_t *label,
                       uint32_t *size);
uint64_t filter_clusters_tdev(st_ctx *c, const st_ttable *t, const st_action &act, const std::string &tag,
                              uint32_t *out_idx);
int combine_layout(const st_ttable *const *srcs, int nsrc, int32_t *col_table, int32_t *col_index);
void combine_tdev(st_ctx *c, const st_ttable *const *srcs, int nsrc, const st_ttable *dst);
void morton_order_dev(st_ctx *c, const float *x, const float *y, const float *z, uint32_t *indices, uint64_t n);
void morton_order_dev_f64(st_ctx *c, const double *x, const double *y, const double *z, uint32_t *indices,
                          uint64_t n);
// x / y / z of any column types (ST_PLY_*): float64 keys when any is not float32 (st_morton.hip)
void morton_order_tdev(st_ctx *c, const void *const xyz[3], const int32_t types[3], uint32_t *indices, uint64_t n);
// transform() over a typed table in place (st_transform.hip)
void transform_tdev(st_ctx *c, const st_ttable *t, const st_transform_params *p);
// (sh64: the 3 sh_coeffs SH columns' JS numbers as float64 when they are not all float32; the
// SH bytes are computed from those and t's f_rest columns are not read)
void pack_compressed_dev(st_ctx *c, const st_table *t, const uint32_t *order, float *chunk, uint32_t *vertex,
                         uint8_t *sh, const double *const *sh64 = nullptr, int sh_coeffs = 0);
// returns draws consumed
// initializeCentroids over a table of n rows: rows (device) = the k distinct floor(draw * n) in
// draw order, *used = draws consumed (device window with the host loop as fallback)
void kmeans_init_rows(st_ctx *c, const double *draws, uint64_t ndraws, uint64_t n, int k, uint32_t *rows,
                      uint64_t *used);
// out[c * k + i] = cols[c][rows[i] - offset] where offset <= rows[i] < offset + n_local, bits 0 elsewhere
void gather_owned_rows(st_ctx *c, const float *const *cols, int d, uint64_t n_local, uint64_t offset,
                       const uint32_t *rows, int k, float *out);
// (host_init: initializeCentroids by the host's loop instead of on the device)
// (sum64: float64 columns (host array of device pointers) summed by calcAverage instead of cols:
// the JS numbers of columns that are not float32, D > 1)
uint64_t kmeans_dev(st_ctx *c, const float *const *cols, int d, uint64_t n, int k, int iters, const double *draws,
                    uint64_t ndraws, float *centroids, uint32_t *labels, bool host_init = false,
                    const double *const *sum64 = nullptr);
// st_ctx_last_kmeans_stats' JSON from c->kn_stats (the N-D k-means writers call it at their end)
void kn_stats_publish(st_ctx *c);
uint64_t cluster1d_dev(st_ctx *c, const float *const *cols, int ncols, uint64_t n, int iters, const double *draws,
                       uint64_t ndraws, float *centroids256, uint8_t *labels);
uint64_t sog_dev(st_ctx *c, const st_table *t, int iters, const double *draws, uint64_t ndraws, st_sog_meta *meta,
                 const st_sog_textures *out);
// writeSog's device part over a table of any column types (write-sog.ts reads the members as JS
// numbers, cluster1d and the k-means points through Float32Arrays): float32 tables take sog_dev
uint64_t sog_tdev(st_ctx *c, const st_ttable *t, int iters, const double *draws, uint64_t ndraws,
                  st_sog_meta *meta, const st_sog_textures *out);
void codebook_dev(st_ctx *c, const float *cen, const uint32_t *lab, uint64_t total, float *centroids256,
                  uint8_t *labels);
void sog_scatter_dev(st_ctx *c, const st_table *t, const uint32_t *pos, const double lo[3], const double hi[3],
                     const uint8_t *scale_lab, const uint8_t *color_lab, const uint32_t *shn_lab, st_sog_meta *meta,
                     const st_sog_textures *out);
void shn_centroids_dev(st_ctx *c, const uint8_t *cl, int C, int pal, uint8_t *out);
// the scales / sh0 texels of n rows in row order (byte labels: three planes of n; opacity nullable)
void sog_table_rows(st_ctx *c, uint64_t n, const uint8_t *lab, const float *opacity, uint8_t *out);
// cluster1d of the scales (a) and the colours (b) as the single-device writer runs them (b beside a
// on the context `side`, speculatively from draw 0); returns the draws both took
uint64_t cluster1d_pair_dev(st_ctx *c, st_ctx *side, const float *const *a, const float *const *b, uint64_t n,
                            int iters, const double *draws, uint64_t ndraws, float *cb_a, uint8_t *lab_a, float *cb_b,
                            uint8_t *lab_b);

// PLY ingest / compressed-PLY reader (st_ply.hip)
// a host consumer of the PLY reader's pinned row chunks (st_ply_read's host transpose)
struct ChunkSink {
    virtual ~ChunkSink() = default;
    // rows [row, row + nrows) of the element are in the pinned chunk buffer b (0 / 1): consume
    // them asynchronously
    virtual void take(int b, const uint8_t *rows, uint64_t row, uint64_t nrows) = 0;
    // before buffer b is refilled: returns once the host is done with its last chunk
    virtual void wait(int b) = 0;
};
void ply_read_dev(st_ctx *c, int fd, const st_ply_header &h, int element, void *const *cols,
                  ChunkSink *sink = nullptr);
// the chunk loop of ply_read_dev for any file of fixed-size rows (the .splat reader, st_readers.hip):
// `count` rows of R bytes at file offset `off` go page cache -> pinned double buffer -> HBM in
// chunks of whole multiples of RB rows; run(rows, nr, row) queues the work on a staged chunk
// (device rows, their count, the index of the first); short_msg: the error of a short file
void stream_rows_dev(st_ctx *c, int fd, uint64_t off, uint64_t count, uint64_t R, uint32_t RB,
                     const std::function<void(const uint8_t *, uint64_t, uint64_t)> &run, ChunkSink *sink,
                     const char *short_msg);
// st_ply_read: into the caller's host columns, and the element's mirrors (st_ctx::HostMirror)
void ply_read_host(st_ctx *c, int fd, const st_ply_header &h, int element, void *const *host_cols, bool lazy = false);
// st_ply_materialize: the lazy mirrors among these host columns copied down and dropped (upload()
// calls it first: no host form reads an unfilled column)
void materialize_lazy(st_ctx *c, const void *const *host, int n);
// (mirror_mu held) the mirrors `pick` selects removed, their own device blocks pooled
void drop_mirrors_locked(st_ctx *c, const std::function<bool(const st_ctx::HostMirror &)> &pick);
// the process-wide record of lazy host ranges (address, bytes, owning context; one mutex, taken
// after a context's mirror_mu where both are held): a lazy column is unfilled memory to every
// context but the one that read it.  Added where ply_read_host registers lazy mirrors, removed by
// drop_mirrors_locked and st_ctx_destroy.
void lazy_range_add(st_ctx *c, const void *host, uint64_t bytes);
void lazy_range_remove(st_ctx *c, const void *host);
void lazy_ranges_forget(st_ctx *c);
// ST_ERR_ARG when an upload's source overlaps a lazy range of a context other than c (staged_h2d
// after c's own mirrors came down, resident_table's uploads; not staged_h2d_raw itself)
void refuse_foreign_lazy(st_ctx *c, const std::vector<HostXfer> &xs);
void decompress_ply_dev(st_ctx *c, uint64_t n, const float *const *chunk, const uint32_t *const *vertex,
                        const uint8_t *const *sh, int nsh, float *const *out);
// the PLY writer (write-ply.ts): k_ply_rows over one device table, the inverse of the reader's
// transpose.  The constructor checks the table (ST_ERR_ARG for a bad type or a misaligned column,
// ST_ERR_UNSUPPORTED for rows longer than 12 KiB) and uploads its layout once; run() queues rows
// [row0, row0 + nrows) as nrows x R bytes at out (4-byte aligned, device) on the context stream
struct PlyRows {
    st_ctx *c;
    uint32_t R = 0, RB = 64;  // row bytes, rows per workgroup
    int ncol = 0;
    void *d_props = nullptr;
    void **d_cols = nullptr;
    PlyRows(st_ctx *ctx, const st_ttable *t, const std::string &tag);
    void run(uint64_t row0, uint64_t nrows, uint8_t *out);
};
// write-ply.ts:19-35 for one element ("vertex" when element is null): the whole header, or only the
// element / property lines
std::string ply_header_text(const st_ttable *t, const char *element, const char *const *comments, int ncomments,
                            bool element_only);

// the CSV writer (write-csv.ts, st_csv.hip): one device table's rows as text, a piece at a time.
// The constructor checks the table (ST_ERR_ARG: no columns, a bad type, a misaligned column;
// ST_ERR_UNSUPPORTED: a worst-case row -- every cell at its type's longest text, plus a separator
// per cell -- above CSV_LDS_BYTES) and uploads its layout and the power-of-ten table.  measure()
// runs the length pass and the scan over rows [row0, row0 + nrows) and returns their bytes (it
// waits for the stream); write() then queues the same rows' text at out + out_off (out 4-byte
// aligned, out_off any byte).  A piece holds at most CSV_PIECE_BYTES by the worst-case width.
constexpr uint64_t CSV_LDS_BYTES = 48 * 1024, CSV_PIECE_BYTES = 256ull << 20;
struct CsvRows {
    st_ctx *c;
    std::string tag;
    uint32_t W = 0, RB = 1;  // worst-case row bytes, rows per workgroup: min(256, CSV_LDS_BYTES / W)
    int ncol = 0;
    void *d_cols = nullptr;
    uint64_t *d_tab = nullptr;
    uint16_t *coff = nullptr;
    uint32_t *rowoff = nullptr;
    CsvRows(st_ctx *ctx, const st_ttable *t, const std::string &tag);
    uint64_t measure(uint64_t row0, uint64_t nrows);
    void write(uint64_t row0, uint64_t nrows, uint8_t *out, uint64_t out_off);
    uint64_t piece_rows(uint64_t bytes) const;  // the rows that fit `bytes` whatever their values
};
uint64_t csv_max_row_bytes(const st_ttable *t);
std::string csv_header_text(const st_ttable *t);  // write-csv.ts:9-10
// st_numfmt.h's power-of-ten table on the host (built at first use): 2 * POW10_ENTRIES words
const uint64_t *numfmt_host_table();

// the .splat and .spz writers (st_writers.hip; the rules: st_abi.h, "the .splat and .spz writers").
// wr_table picks the fourteen required columns by name (the first of a name wins; a missing one,
// a bad type or a misaligned column is ST_ERR_ARG under `what`) and, with_sh, the 3C f_rest
// columns of the table's band.  Slots: x y z scale_0..2 f_dc_0..2 opacity rot_0..3 f_rest_0..
struct WrCol {
    const void *p;
    int32_t t, pad;
};
struct WrCols {
    WrCol c[14 + 45];
};
struct WrTable {
    WrCols cols;
    uint64_t n;
    int C;     // SH coefficients per channel: 0 without with_sh
    bool f32;  // every picked column is float32
};
WrTable wr_table(const st_ttable *t, bool with_sh, const char *what);
// rows [row0, row0 + nrows) as nrows x 32 bytes at out (device, 4-byte aligned), queued on the stream
void splat_rows_dev(st_ctx *c, const WrTable &W, uint64_t row0, uint64_t nrows, uint8_t *out);
uint64_t spz_image_size(uint64_t n, int C);  // 0 for a C that is no band or n >= 2^32
void spz_check(const WrTable &W, int fractional_bits);  // ST_ERR_ARG / ST_ERR_UNSUPPORTED of the rules
// header + six planes of the whole table at out (device, any alignment, spz_image_size bytes);
// waits for the stream; *clamped (nullable) = the position values clamped.  Returns the size
uint64_t spz_image_dev(st_ctx *c, const WrTable &W, int fractional_bits, uint8_t *out, uint64_t *clamped);
// st_deflate.hip: the RFC 1951 stream / the gzip member of dev_in[0..n) at dev_out (any alignment);
// returns its size; above cap: ST_ERR_ARG and nothing is written.  Both wait for their kernels.
uint64_t deflate_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap);
uint64_t gzip_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap);
// st_inflate.hip: the raw deflate stream / gzip member dev_in[0..n) into dev_out[0..expect); false =
// declined (st_abi.h, "inflating a gzip member on the device").  Both wait for the kernels.
bool inflate_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_bytes,
                 st_inflate_stats *stats);
bool gunzip_dev(st_ctx *c, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect, uint64_t chunk_bytes,
                st_inflate_stats *stats);

// the column summary (st_summary.hip; the rules: st_abi.h, "column summary"): one st_col_summary per
// column of a device table read in place / of a host table uploaded through the staged copies; both
// wait for the stream and leave the sum paths taken in c->last_summary_stats
void summary_dev(st_ctx *c, const st_ttable *t, st_col_summary *out);
void summary_host(st_ctx *c, const st_ttable *t, st_col_summary *out);
// the same device steps on one float64 column, for a caller inside the library (filterOutliers'
// threshold): waits for the stream, leaves st_ctx_last_summary_stats as it was
void summary_f64_dev(st_ctx *c, const double *col, uint64_t n, st_col_summary *out);

// the .ksplat writer (st_ksplat_write.hip; the rules: st_abi.h, "the .ksplat writer").  ksplat_params
// checks mode, degree (-1: the table's own), block size and harmonics range against a table picked
// with_sh (ST_ERR_ARG / ST_ERR_UNSUPPORTED of the rules); modes 0 and 1 get the default range
struct KswParams {
    float B, sh_min, sh_max;
    int mode, c_out;  // c_out: SH coefficients per channel of the file
};
KswParams ksplat_params(const WrTable &W, int mode, int degree, double block_size, float sh_min, float sh_max);
uint64_t ksplat_image_size(uint64_t n, int C, int mode, uint64_t full, uint64_t partial);  // 0 for a bad argument
// a plan in the workspace between its two steps: the sorted keys and rows, the cells' scans, and what
// came back to the host
struct KswPlan {
    uint64_t n, F, P, clamped;
    float B;
    int sort_bits;  // key bits the sort went over
    uint64_t *keys;
    uint32_t *rows, *cid, *cstart, *fulloff, *partoff, *prow;
    const void *stats;
};
// keys, sort and the scans over the cells: F, P and the clamp count are read back (waits for the stream)
KswPlan ksplat_plan_begin(st_ctx *c, const WrTable &W, float B);
uint64_t ksplat_plan_image_size(const KswPlan &K, const KswParams &P);
// headers, bucket tables and records of a begun plan at out (device, any alignment,
// ksplat_plan_image_size bytes); waits for the stream
void ksplat_image_from_plan(st_ctx *c, const WrTable &W, const KswParams &P, const KswPlan &K, uint8_t *out);

// the HTML viewer writer (write-html.ts, st_html.hip).  base64_dev queues k_base64 on the context
// stream: the RFC 4648 text of bytes [byte0, byte0 + nbytes) of the stream that up to B64_MAX_SEGS
// device segments make back to back, contiguous at out (device, 4-byte aligned).  base64_check
// throws ST_ERR_ARG for a range the kernel does not take (byte0 not a multiple of 3, a range
// outside the stream, a partial last group before the stream's end) and returns the text's size;
// base64_dev runs it first.  html_parts: the page of write-html.ts:46-55 split around the payload.
constexpr int B64_MAX_SEGS = 4;
uint64_t base64_size(uint64_t nbytes);
uint64_t base64_check(const st_bytes_seg *segs, int nseg, uint64_t byte0, uint64_t nbytes);
void base64_dev(st_ctx *c, const st_bytes_seg *segs, int nseg, uint64_t byte0, uint64_t nbytes, uint8_t *out);
struct HtmlParts {
    std::string prefix, suffix;  // the file is prefix + base64 + suffix when embeds, else prefix
    bool embeds = false;
};
HtmlParts html_parts(const char *html, const char *css, const char *js, const double *camera, const double *target);

// multi-GPU building blocks (st_dist.hip)
void minmax_dev(st_ctx *c, const float *const *cols, int ncols, uint64_t n, double *lo, double *hi);
void dist_prepare(st_ctx *c, const float *const *cols, int d, uint64_t n);
void dist_assign(st_ctx *c, const float *const *cols, int d, uint64_t n, int k, const float *cen, uint32_t *labels);
// dist_assign + dist_partials of a 1-D point set with k <= 256 in one pass (no member sort)
void dist_assign_partials1d(st_ctx *c, const float *pts, uint64_t n, int nseg, int k, const float *cen,
                            uint32_t *labels, double *sums, double *sabs, int32_t *emin, uint32_t *counts);
// dist_assign + dist_partials of an N-D shard (one segment) in one pass: the fused fix-up's
// sums, the member order built only for pending pairs; false (nothing written but the labels):
// the assign could not fuse, the caller takes dist_partials
// (dcols: the shard's column pointers, a device array)
bool dist_assign_partials_nd(st_ctx *c, const float *const *dcols, int d, uint64_t n, int k, const float *cen,
                             uint32_t *labels, double *sums, double *sabs, int32_t *emin, uint32_t *counts);
void dist_partials(st_ctx *c, const float *const *cols, int d, uint64_t n, int nseg, int k, const uint32_t *labels,
                   double *sums, double *sabs, int32_t *emin, uint32_t *counts);
void dist_seqsum(st_ctx *c, int d, int k, int seg, const uint32_t *pairs, uint32_t npairs, double *running,
                 const int32_t *emin, const double *sabs);
uint32_t dist_finish(st_ctx *c, int d, int k, const double *sums, const double *sabs, const int32_t *emin,
                     const uint32_t *counts, float *cen, uint32_t *pending);
void dist_average(st_ctx *c, int d, int k, const uint32_t *pairs, uint32_t npairs, const double *running,
                  const uint32_t *counts, float *cen);

// processDataTable on a device float32 table (st_chain.hip)
struct ProcessedF32 {
    std::vector<std::string> names;
    std::vector<const char *> cn;
    std::vector<float *> cols;
    st_table t{};
};
void chain_apply_f32(st_ctx *c, const st_table *in, const st_action *actions, int nactions, const std::string &tag,
                     ProcessedF32 &out);

// multi-GPU writeSog (st_multi.hip): the st_set_devices group a one-call form shards its rows over
// (ST_NUM_GPUS applied on first use; its error is thrown), empty: one device.  The returned
// reference keeps the group alive for the caller's call even if st_set_devices replaces it
std::shared_ptr<st_group> sog_group();

}  // namespace st
