/*
 * st_abi.h -- C-ABI of the MI355X splat-transform hot path (libsplat_hip.so).
 *
 * Plain pointers and sizes only.  Each entry point replaces one reference seam
 * (file:line into praveenpenumaka/splat-transform src/):
 *
 *   st_transform / st_dev_transform         transform(dataTable, t, r, s)      transform.ts:12-65
 *   st_quat_from_euler                      Quat.setFromEulerAngles             process.ts:75-79
 *   st_transform_params_make                Mat4.setTRS + Mat3.setFromQuat +
 *                                           new RotateSH(mat3)                  transform.ts:13-15,
 *                                                                               rotate-sh.ts:49-149
 *   st_filter_finite / st_dev_filter_finite filter(dt, isFinite-all) indices    process.ts:47-61,84-95
 *   st_filter_nan                           filterNaN: filter + permuteRows     process.ts:84-95
 *   st_dev_permute_rows[_t]                 DataTable.permuteRows               data-table.ts:135-149
 *   st_combine_layout / st_dev_combine      combine()                           index.ts:158-210
 *   st_dev_concat_rows                      combine() of float32 tables         index.ts:158-210
 *   st_morton_order / st_dev_morton_order   generateOrdering(dataTable, idx)    ordering.ts:4-110
 *   st_pack_compressed / st_dev_...         writeCompressedPly chunk loop +
 *                                           CompressedChunk.pack                write-compressed-ply.ts:56-109,
 *                                                                               compressed-chunk.ts:44-180
 *   st_kmeans / st_dev_kmeans               kmeans(points, k, iters) --no-gpu   k-means.ts:137-201,
 *                                                                               kd-tree.ts:9-100
 *   st_cluster1d / st_dev_cluster1d         cluster1d(dataTable, iters)         write-sog.ts:56-99
 *   st_sog / st_dev_sog                     writeSog texture + meta generation  write-sog.ts:110-370
 *   st_set_devices / st_group_sog /         writeSog with the rows sharded over
 *   st_dev_sog_sharded                      GPUs (RCCL; device choice of        write-sog.ts:241-243,313
 *                                           the reference's clusterer)
 *   st_dev_kmeans_* (step API)              one k-means iteration split at the
 *                                           centroid-sum exchange (multi-GPU)   k-means.ts:164-192
 *   st_dev_cluster1d_codebook               cluster1d's sorted codebook + byte
 *                                           labels                              write-sog.ts:69-88
 *   st_dev_sog_scatter / _shn_centroids     one shard's texels of writeSog      write-sog.ts:142-239,
 *                                                                               :319-348
 *   st_webp_lossless / st_dev_webp_lossless WebPEncodeLosslessRGBA (libwebp)   lib/webp_encode.c:19-29,
 *                                                                               utils/webp.ts:19-41
 *   st_dev_crc32                            Crc.update / value                  serialize/crc.ts:1-28
 *   st_zip_store                            ZipWriter (store, descriptors)      serialize/zip-writer.ts:35-135
 *   st_sog_meta_json                        JSON.stringify(meta)                write-sog.ts:271-293,350-361
 *   st_sog_bundle / st_dev_sog_bundle       writeSog to a .sog bundle           write-sog.ts:110-140,361-366
 *   st_ply_read_header / _parse_header      readPly header search + parseHeader readers/read-ply.ts:54-137
 *   st_ply_read / st_dev_ply_read           readPly element rows -> columns     read-ply.ts:139-188
 *   st_ply_read_resident (+ _materialize,   readPly, the values left in HBM     read-ply.ts:111-191
 *     _forget)                              until the host asks for them
 *   st_dev_ply_transpose                    (the same, rows already in HBM)     read-ply.ts:165-182
 *   st_decompress_ply / st_dev_...          decompressPly                       readers/decompress-ply.ts:82-232
 *   st_splat_layout / st_splat_read /       readSplat                           readers/read-splat.ts:14-148
 *     st_dev_splat_read / _decode             (size checks :21-29, row decode :71-138)
 *   st_ksplat_layout / st_ksplat_read /     readKsplat                          readers/read-ksplat.ts:103-384
 *     st_dev_ksplat_read / _decode            (headers and section views :111-232, :371;
 *                                             record decode :255-366, decodeFloat16 :29-60)
 *   st_spz_layout / st_spz_read /           readSpz after its gunzip            readers/read-spz.ts:62-241
 *     st_dev_spz_read / _decode               (header and plane views :65-107, decode :139-232)
 *   st_process                              processDataTable(dataTable, actions) process.ts:64-145
 *   st_ply_compressed_ply / st_ply_sog_bundle  readPly + processDataTable + writer, resident
 *                                           (the CLI's one-input path)           index.ts:463-496
 *   st_ply_compressed_ply_file /            the same + the output file written   write-compressed-ply.ts:31-115,
 *   st_compressed_ply_file                  at offsets as it leaves HBM          index.ts:101-154
 *   st_compressed_ply / st_dev_...          processDataTable + writeCompressedPly
 *                                           (CLI: in.ply [actions] out.compressed.ply) index.ts:463-496,
 *                                                                               write-compressed-ply.ts:31-115
 *   st_zip_index / st_webp_info /           (none: the reference writes SOG and cannot read it)
 *     st_webp_decode_lossless /               the inverse of writeSog: ZIP index, WebP-lossless
 *     st_sog_read_layout / st_dev_sog_decode  decode (RFC 9649) and the dequantising kernel;
 *     / st_sog_read / st_dev_sog_read         rules in "the .sog reader" below       write-sog.ts:162-268,319-348
 *   st_dev_csv_rows / st_dev_csv_file /     writeCsv (header line, rows of
 *   st_csv_file / st_ply_csv_file             Number::toString cells)            writers/write-csv.ts:5-23,
 *                                                                               index.ts:117-118
 *   st_dev_splat_rows / st_dev_splat_file / (none: the reference reads .splat and .spz and writes
 *     st_splat_file / st_ply_splat_file /     neither) each field the code its reader decodes to
 *     st_spz_image_size / st_dev_spz_planes   the nearest value; rules in "the .splat and .spz
 *     / st_dev_spz_image / st_dev_spz_file /  writers" below             readers/read-splat.ts:71-138,
 *     st_spz_file / st_ply_spz_file                                      readers/read-spz.ts:139-232
 *   st_ksplat_image_size /                  (none: the reference reads .ksplat and does not write
 *     st_dev_ksplat_plan /                    it) spatial buckets, then each field the code its
 *     st_dev_ksplat_records /                 reader decodes to the nearest value; rules in "the
 *     st_dev_ksplat_image / st_dev_ksplat_file  .ksplat writer" below      readers/read-ksplat.ts:103-384
 *     / st_ksplat_file / st_ply_ksplat_file
 *
 * Conventions
 *  - Columns are SoA float32 arrays of n rows (the reference's Float32Array
 *    columns, read-ply.ts:148-150).  st_* entry points take HOST pointers and
 *    copy through HBM; st_dev_* take DEVICE pointers and run on the context's
 *    stream (asynchronously unless the function must return a count).
 *  - Math.random: k-means draws are supplied by the caller as a buffer of
 *    doubles in [0,1) in the order the reference consumes them; `used`
 *    returns how many were consumed.  ST_ERR_DRAWS if the buffer is short.
 *  - Every function returns ST_OK (0) or a negative st_status; the message is
 *    available from st_last_error() (thread-local).  Data anomalies that the
 *    reference tolerates (NaN quantises to 0, degenerate extents skip the
 *    Morton sort) are not errors.  Inputs that crash the reference's k-means
 *    (non-finite points) return ST_ERR_NONFINITE.
 */
#ifndef ST_ABI_H
#define ST_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 1

enum st_status {
    ST_OK = 0,
    ST_ERR_ARG = -1,
    ST_ERR_HIP = -2,
    ST_ERR_NONFINITE = -3,
    ST_ERR_DRAWS = -4,
    ST_ERR_NOMEM = -5,
    ST_ERR_UNSUPPORTED = -6,
    ST_ERR_INTERNAL = -7
};

typedef struct st_ctx st_ctx;

/* SoA table of float32 columns (borrowed for the duration of a call). */
typedef struct {
    uint64_t n;                 /* rows */
    int32_t ncol;               /* columns */
    const char *const *names;   /* PLY property names: x y z f_dc_0 f_rest_k opacity scale_i rot_i ... */
    float *const *cols;         /* column base pointers (host or device, per entry point) */
} st_table;

/* Host-side constants of one transform() call: Mat4.setTRS (f32 storage),
 * the quaternion r, the uniform scale s and the RotateSH band matrices
 * (row-major, f64) built from Mat3.setFromQuat(r). */
typedef struct {
    float m4[16];
    double r[4]; /* x, y, z, w */
    double s;
    double sh1[9];
    double sh2[25];
    double sh3[49];
} st_transform_params;

typedef struct {
    int32_t width, height;          /* means/quats/scales/sh0/shN_labels textures (RGBA8) */
    double means_min[3], means_max[3];
    float scales_codebook[256];
    float sh0_codebook[256];
    int32_t sh_bands;               /* 0..3 */
    int32_t palette_size;           /* shN.count */
    float shn_codebook[256];
    int32_t shn_width, shn_height;  /* shN_centroids texture */
} st_sog_meta;

/* PLY header (readers/read-ply.ts:7-26); property types of read-ply.ts:28-40 */
enum st_ply_type {
    ST_PLY_CHAR = 1, ST_PLY_UCHAR, ST_PLY_SHORT, ST_PLY_USHORT, ST_PLY_INT, ST_PLY_UINT, ST_PLY_FLOAT, ST_PLY_DOUBLE
};
#define ST_PLY_MAX_ELEMENTS 16
#define ST_PLY_MAX_PROPS 256
#define ST_PLY_NAME 64
typedef struct {
    char name[ST_PLY_NAME];
    int32_t type; /* st_ply_type */
} st_ply_property;
typedef struct {
    char name[ST_PLY_NAME];
    uint64_t count;
    int32_t nprops;
    st_ply_property props[ST_PLY_MAX_PROPS];
} st_ply_element;
typedef struct {
    uint64_t header_bytes;   /* bytes up to and including "\nend_header\n" */
    int32_t nelements;
    int32_t ncomments;
    char comments[8192];     /* the comment texts, '\n'-separated */
    st_ply_element elements[ST_PLY_MAX_ELEMENTS];
} st_ply_header;

/* Typed SoA table: the reference's eight column types (data-table.ts:1-27) as st_ply_type
 * codes (ST_PLY_CHAR = Int8Array ... ST_PLY_FLOAT = Float32Array, ST_PLY_DOUBLE =
 * Float64Array).  Used where the reference handles every type: filterNaN, permuteRows,
 * combine.  Column data must be aligned to its element size. */
typedef struct {
    uint64_t n;
    int32_t ncol;
    const char *const *names;
    const int32_t *types;       /* st_ply_type per column */
    void *const *cols;
} st_ttable;

typedef struct {
    uint8_t *means_l, *means_u, *quats, *scales, *sh0; /* width*height*4 each */
    uint8_t *shn_centroids;                           /* shn_width*shn_height*4 (NULL if sh_bands==0) */
    uint8_t *shn_labels;                              /* width*height*4 (NULL if sh_bands==0) */
} st_sog_textures;

/* ---- runtime ------------------------------------------------------------ */
int st_abi_version(void);
const char *st_last_error(void);
int st_device_count(int32_t *count);
int st_ctx_create(int32_t device, st_ctx **out);
void st_ctx_destroy(st_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream()); NULL restores the context's own stream. */
int st_ctx_set_stream(st_ctx *ctx, void *hip_stream);
int st_ctx_synchronize(st_ctx *ctx);
/* Per-stage device timing (hipEvents) of the last st_*sog / st_*kmeans call, JSON text. */
const char *st_ctx_last_timings(st_ctx *ctx);
/* the last N-D k-means' assign classification on ctx, summed over its iterations, as JSON:
 * {"assigns", "points", "pairs" (two tile-halves settled by the exact fix-up), "ambiguous"
 * (the second sweep's candidate lists), "overflow" (first lists past 64 rows, collected again),
 * "walked_overflow" (past 2,048 rows too: the KdTree walk), "ties" (exact ties walked)}; "{}"
 * before the first.  Owned by ctx, valid until its next N-D k-means.  (No reference counterpart:
 * diagnostics of this build's exact assign.) */
const char *st_ctx_last_kmeans_stats(st_ctx *ctx);
/* The writeSog host forms (st_sog, st_sog_bundle, st_sog_file) run on the device columns the
 * last st_ply_read left resident when the caller's table is that read's host columns, unchanged:
 * the step starts at once on them while host threads compare every byte of the host columns
 * with the read's pinned copy; the first changed byte abandons the run (nothing has left the
 * device), and the call uploads the columns and runs again.  This reports, for the last such
 * call on ctx, how many columns / bytes ran from the resident copy (0 / 0: uploaded).
 * ST_HOST_MIRROR=0 disables the reuse.  (No reference counterpart: the reference's readPly ->
 * writeSog keeps the table in JS memory, index.ts:433-510.) */
int st_ctx_last_host_reuse(st_ctx *ctx, uint64_t *columns, uint64_t *bytes);
/* Kernel profiling: when enabled, the library brackets its named hot kernels
 * ("kn.sweep", "mo.sort", ...) with hipEvents on the context stream; stats
 * accumulate until st_ctx_reset_kernel_stats.  Query after a synchronize. */
int st_ctx_set_profiling(st_ctx *ctx, int32_t enable);
int st_ctx_reset_kernel_stats(st_ctx *ctx);
int st_ctx_kernel_stats(st_ctx *ctx, const char *name, double *total_ms, uint64_t *launches);
/* Output verification (bench.py, tests): when enabled, every N-D k-means (d > 1) keeps a
 * device copy of the centroids its LAST assign used, its final centroids and its labels
 * (k-means.ts:164-192: the returned labels come from the last assign, the centroids from the
 * update after it).  st_ctx_verify_snapshot writes d, k, n and, where the pointers are not
 * NULL, copies them into caller DEVICE buffers on the context stream: centroids [d][k]
 * float32, labels uint32[n].  Costs three device copies per k-means call while enabled. */
int st_ctx_set_verify(st_ctx *ctx, int32_t enable);
int st_ctx_verify_snapshot(st_ctx *ctx, float *prev_centroids, float *centroids, uint32_t *labels,
                           int32_t *d, int32_t *k, uint64_t *n);

/* ---- host constants ------------------------------------------------------ */
int st_quat_from_euler(double ex_deg, double ey_deg, double ez_deg, double q_xyzw[4]);
int st_transform_params_make(const double t[3], const double r_xyzw[4], double s, st_transform_params *out);
/* SOG texture geometry (write-sog.ts:117-118, :310, :319) */
int st_sog_geometry(uint64_t n, int32_t sh_coeffs, int32_t *width, int32_t *height,
                    int32_t *palette_size, int32_t *shn_width, int32_t *shn_height);

/* ---- host-memory entry points ---------------------------------------------- */
int st_transform(st_ctx *ctx, const st_table *table, const st_transform_params *p);
int st_filter_finite(st_ctx *ctx, const st_table *table, uint32_t *out_idx, uint64_t *out_n);
/* filterNaN on host columns in one call (process.ts:84-95 -> filter -> permuteRows): the table
 * is uploaded once, the surviving rows are compacted on the device and the first *out_m rows of
 * each dst column (host, src's types, capacity n rows) receive them */
int st_filter_nan(st_ctx *ctx, const st_ttable *src, const st_ttable *dst, uint64_t *out_m);
int st_morton_order(st_ctx *ctx, const float *x, const float *y, const float *z, uint32_t *indices, uint64_t n);
int st_pack_compressed(st_ctx *ctx, const st_table *table, const uint32_t *order,
                       float *chunk, uint32_t *vertex, uint8_t *sh);
int st_kmeans(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n, int32_t k, int32_t iters,
              const double *draws, uint64_t ndraws, uint64_t *used, float *centroids, uint32_t *labels);
int st_cluster1d(st_ctx *ctx, const float *const *cols, int32_t ncols, uint64_t n, int32_t iters,
                 const double *draws, uint64_t ndraws, uint64_t *used, float *centroids256, uint8_t *labels);
int st_sog(st_ctx *ctx, const st_table *table, int32_t iters, const double *draws, uint64_t ndraws,
           uint64_t *used, st_sog_meta *meta, const st_sog_textures *out);

/* ---- device-memory entry points (device pointers, context stream) ---------- */
int st_dev_transform(st_ctx *ctx, const st_table *table, const st_transform_params *p);
int st_dev_filter_finite(st_ctx *ctx, const st_table *table, uint32_t *out_idx, uint64_t *out_n);
int st_dev_permute_rows(st_ctx *ctx, const st_table *src, const uint32_t *idx, uint64_t m, const st_table *dst);
int st_dev_concat_rows(st_ctx *ctx, const st_table *const *srcs, int32_t nsrc, const st_table *dst);
/* typed forms (every column type, as the reference):
 *   filterNaN's indices: float32 and float64 columns are tested with isFinite, integer
 *     columns are always finite (process.ts:84-95)
 *   permuteRows: dst[c][j] = src[c][idx[j]], dst columns of src's types (data-table.ts:135-149)
 *   combine: st_combine_layout lists the result columns -- (table, column) of each, the
 *     first table's columns then every later column without a (name, type) match
 *     (index.ts:164-178); st_dev_combine fills a dst of that layout with sum(n) rows: zeros,
 *     then each source column at its table's row offset in its first (name, type) match */
int st_dev_filter_finite_t(st_ctx *ctx, const st_ttable *table, uint32_t *out_idx, uint64_t *out_n);
int st_dev_permute_rows_t(st_ctx *ctx, const st_ttable *src, const uint32_t *idx, uint64_t m, const st_ttable *dst);
/* host only (no device); col_table / col_index may be NULL to query the count */
int st_combine_layout(const st_ttable *const *srcs, int32_t nsrc, int32_t *col_table, int32_t *col_index,
                      int32_t *ncol);
int st_dev_combine(st_ctx *ctx, const st_ttable *const *srcs, int32_t nsrc, const st_ttable *dst);
int st_dev_morton_order(st_ctx *ctx, const float *x, const float *y, const float *z, uint32_t *indices, uint64_t n);
int st_dev_pack_compressed(st_ctx *ctx, const st_table *table, const uint32_t *order,
                           float *chunk, uint32_t *vertex, uint8_t *sh);
/* draws stay on the host (the reference's Math.random lives there) */
int st_dev_kmeans(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n, int32_t k, int32_t iters,
                  const double *draws, uint64_t ndraws, uint64_t *used, float *centroids, uint32_t *labels);
int st_dev_cluster1d(st_ctx *ctx, const float *const *cols, int32_t ncols, uint64_t n, int32_t iters,
                     const double *draws, uint64_t ndraws, uint64_t *used, float *centroids256, uint8_t *labels);
int st_dev_sog(st_ctx *ctx, const st_table *table, int32_t iters, const double *draws, uint64_t ndraws,
               uint64_t *used, st_sog_meta *meta, const st_sog_textures *out);

/* ---- processDataTable + writeCompressedPly in one upload (BASELINE config 3) -----
 * The reference's action list (process.ts:64-145) applied to a typed table in order:
 *   ST_ACTION_TRANSFORM     one transform() pass (translate / rotate / scale, process.ts:72-83),
 *                           params from st_transform_params_make; columns of any type (as
 *                           st_transform_t)
 *   ST_ACTION_FILTER_NAN    filterNaN (process.ts:84-95)
 *   ST_ACTION_FILTER_VALUE  filterByValue (process.ts:97-109): row[column] <compare> value;
 *                           compare outside ST_CMP_LT..ST_CMP_NEQ keeps every row (:108)
 *   ST_ACTION_FILTER_BANDS  filterBands (process.ts:110-134): f_rest columns renamed / dropped
 *                           (the input band is read from the ORIGINAL table, as :111 does)
 *   ST_ACTION_PARAM         no-op (:135-138)
 * st_process: the processed table's columns are matched by (name, type) into dst (host, capacity
 * src->n rows); *out_m = its rows.  st_compressed_ply: the processed table goes on through
 * writeCompressedPly's ordering and chunk loop (write-compressed-ply.ts:31-115): chunk
 * ceil(m/256)*18 f32, vertex m*4 u32, sh m*3C u8 (host, sized for src->n rows and src's band);
 * *out_m = m, *out_sh_coeffs = C.  st_dev_compressed_ply: the same over device columns
 * (transformed in place, like the reference's table) into device outputs. */
enum st_action_kind {
    ST_ACTION_TRANSFORM = 1, ST_ACTION_FILTER_NAN, ST_ACTION_FILTER_VALUE, ST_ACTION_FILTER_BANDS, ST_ACTION_PARAM,
    /* this project's own kinds: "importance, decimation and crops" below */
    ST_ACTION_ORDER_IMPORTANCE, ST_ACTION_DECIMATE, ST_ACTION_FILTER_BOX, ST_ACTION_FILTER_SPHERE,
    /* "neighbour distances and outliers" below */
    ST_ACTION_FILTER_OUTLIERS,
    /* "clusters" below */
    ST_ACTION_FILTER_CLUSTERS
};
enum st_compare { ST_CMP_LT = 0, ST_CMP_LTE, ST_CMP_GT, ST_CMP_GTE, ST_CMP_EQ, ST_CMP_NEQ };
enum st_decimate_mode { ST_DECIMATE_COUNT = 0, ST_DECIMATE_FRACTION = 1 };
enum st_outlier_mode { ST_OUTLIER_SIGMA = 0, ST_OUTLIER_DISTANCE = 1 };
enum st_cluster_mode { ST_CLUSTER_MIN_SIZE = 0, ST_CLUSTER_LARGEST = 1 };
typedef struct {
    int32_t kind;                    /* st_action_kind */
    int32_t compare;                 /* ST_ACTION_FILTER_VALUE: st_compare */
    const char *column;              /* ST_ACTION_FILTER_VALUE */
    double value;                    /* ST_ACTION_FILTER_VALUE */
    int32_t bands;                   /* ST_ACTION_FILTER_BANDS: output bands 0..3 */
    st_transform_params transform;   /* ST_ACTION_TRANSFORM */
    /* appended for the kinds after ST_ACTION_PARAM; a zero-filled st_action stays valid for the old ones */
    double box_min[3], box_max[3];   /* ST_ACTION_FILTER_BOX: the corners */
    double center[3];                /* ST_ACTION_FILTER_SPHERE */
    double radius;                   /* ST_ACTION_FILTER_SPHERE */
    double amount;                   /* ST_ACTION_DECIMATE: the row count or the fraction */
    int32_t amount_mode;             /* ST_ACTION_DECIMATE: st_decimate_mode */
    int32_t neighbors;               /* ST_ACTION_FILTER_OUTLIERS: k, 1..32 */
    int32_t outlier_mode;            /* ST_ACTION_FILTER_OUTLIERS: st_outlier_mode */
    double outlier_value;            /* ST_ACTION_FILTER_OUTLIERS: sigma, or the distance */
    double cluster_radius;           /* ST_ACTION_FILTER_CLUSTERS: the link radius, >= 0 (+Infinity allowed) */
    int32_t cluster_mode;            /* ST_ACTION_FILTER_CLUSTERS: st_cluster_mode */
    double cluster_min;              /* ST_ACTION_FILTER_CLUSTERS, ST_CLUSTER_MIN_SIZE: the smallest size kept */
} st_action;
int st_process(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, const st_ttable *dst,
               uint64_t *out_m);
int st_compressed_ply(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, float *chunk,
                      uint32_t *vertex, uint8_t *sh, uint64_t *out_m, int32_t *out_sh_coeffs);
int st_dev_compressed_ply(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                          float *chunk, uint32_t *vertex, uint8_t *sh, uint64_t *out_m, int32_t *out_sh_coeffs);
/* The same straight from the PLY file (`in.ply [actions] out.compressed.ply` / `in.ply [actions]
 * out.sog`, index.ts:463-496): the element's rows stream page cache -> pinned -> HBM
 * (st_dev_ply_read, read-ply.ts:139-188) and stay resident through the actions and the writer;
 * only the outputs cross back.  element < 0 selects the element named "vertex".
 * st_ply_compressed_ply: outputs sized for the element's row count and band.
 * st_ply_sog_bundle: st_sog_bundle of the processed table (malloc'd archive, st_free); with
 * st_set_devices(n > 1) the processed columns are sharded over the group from the host. */
int st_ply_compressed_ply(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                          int32_t nactions, float *chunk, uint32_t *vertex, uint8_t *sh, uint64_t *out_m,
                          int32_t *out_sh_coeffs);
/* writeCompressedPly into a file (write-compressed-ply.ts:31-115 and the CLI's write of the
 * output, index.ts:101-154): st_ply_compressed_ply / st_compressed_ply's chain, then the header
 * (the reference's text, "comment Generated by splat-transform <version>"; version NULL =
 * "0.10.1") and the chunk / vertex / sh arrays written to out_fd at offsets from its current
 * position (where the reference's FileHandle.write calls would go; the CLI's fresh output: 0)
 * as they come down from HBM through pinned slots (a host thread writes one slot while the next
 * one copies); the descriptor's position ends after the output and a longer file is cut there,
 * so a reused output needs no O_TRUNC.  out_fd must be a seekable descriptor open for writing
 * and not O_APPEND (ST_ERR_ARG before any work).  *size = the bytes written.
 * st_compressed_ply_file takes a host table (uploaded once). */
int st_ply_compressed_ply_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element,
                               const st_action *actions, int32_t nactions, int32_t out_fd, const char *version,
                               uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size);
int st_compressed_ply_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                           int32_t out_fd, const char *version, uint64_t *out_m, int32_t *out_sh_coeffs,
                           uint64_t *size);
int st_ply_sog_bundle(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                      int32_t nactions, int32_t iters, const double *draws, uint64_t ndraws, uint64_t *used,
                      uint16_t dos_time, uint16_t dos_date, uint8_t **out, uint64_t *out_size);

/* ---- every column type on the writers' path ---------------------------------
 * The reference reads its columns through getRow (data-table.ts:63-68: each element as a JS
 * number, whatever the TypedArray) and writes through setRow (:70-76: a TypedArray store), so
 * a PLY with double (or integer) x / y / z / rot / scale / f_rest properties transforms, orders
 * and compresses.  These forms take typed tables (st_ttable, ST_PLY_* types):
 *   st_transform_t / st_dev_transform_t   transform() in place (transform.ts:12-65): f64
 *       arithmetic on the numbers, TypedArray stores (Float32 rounds, Float64 keeps, integers
 *       take ToInt32 cut to their width); SH through the Float32Array shCoeffs (transform.ts:21)
 *   st_morton_order_t / st_dev_morton_order_t   generateOrdering (ordering.ts:4-110) of x / y / z
 *       of any types (keys from the JS numbers)
 *   st_sog_process / st_sog_bundle_process   processDataTable (the actions, as st_process) then
 *       writeSog (write-sog.ts:110-370) of a typed host table: the textures + meta (as st_sog)
 *       or the .sog archive (as st_sog_bundle, malloc'd, st_free).  Positions, rotations and
 *       opacity are read as numbers; cluster1d and the k-means points through Float32Arrays;
 *       calcAverage (k-means.ts:41-63) sums the numbers.  With st_set_devices(n > 1) the
 *       processed columns must be float32 (the sharded path moves float32 columns)
 *   st_dev_sog_t   writeSog's device part over a typed device table
 * st_process / st_compressed_ply / st_dev_compressed_ply / st_ply_* take every type too
 * (transform actions, the writer's Morton order, chunk members and SH bytes). */
int st_transform_t(st_ctx *ctx, const st_ttable *table, const st_transform_params *p);
int st_dev_transform_t(st_ctx *ctx, const st_ttable *table, const st_transform_params *p);
int st_morton_order_t(st_ctx *ctx, const void *const xyz[3], const int32_t types[3], uint32_t *indices, uint64_t n);
int st_dev_morton_order_t(st_ctx *ctx, const void *const xyz[3], const int32_t types[3], uint32_t *indices,
                          uint64_t n);
int st_sog_process(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t iters,
                   const double *draws, uint64_t ndraws, uint64_t *used, st_sog_meta *meta,
                   const st_sog_textures *out);
int st_sog_bundle_process(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                          int32_t iters, const double *draws, uint64_t ndraws, uint64_t *used, uint16_t dos_time,
                          uint16_t dos_date, uint8_t **out, uint64_t *out_size);
int st_dev_sog_t(st_ctx *ctx, const st_ttable *table, int32_t iters, const double *draws, uint64_t ndraws,
                 uint64_t *used, st_sog_meta *meta, const st_sog_textures *out);

/* ---- multi-GPU building blocks -----------------------------------
 * One process per GPU; rows are sharded in contiguous ranges in rank order; the
 * caller runs the collectives between calls (splat-transform_amd/py/splat_dist.py
 * composes them into kmeans / cluster1d / writeSog over the whole table).
 * k-means iteration = assign -> partials -> [allreduce sum/sum/min/sum] -> finish
 * -> [segment-ordered chain of seqsum for the pending pairs] -> average -> re-seed
 * empties from the draws (host).  Sums are [nseg][d][k] f64, counts [nseg][k];
 * a segment is a part of the shard that is contiguous in the global point order
 * (the shard for d > 1; one column of cluster1d's concatenation for d == 1). */
/* NaN-ignoring per-column min/max (+inf/-inf for a column without numbers) */
int st_dev_minmax(st_ctx *ctx, const float *const *cols, int32_t ncols, uint64_t n, double *lo, double *hi);
/* validates (ST_ERR_NONFINITE) and prepares the local point set for assign/partials */
int st_dev_kmeans_prepare(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n);
/* initializeCentroids (k-means.ts:8-20) over the global table of n rows, identical on every rank:
 * rows (device, k entries) = the first k distinct floor(draw * n) in draw order; *used = draws
 * consumed (replaces splat_dist's host selection; the owners then supply the rows) */
int st_dev_kmeans_init_rows(st_ctx *ctx, const double *draws, uint64_t ndraws, uint64_t n, int32_t k,
                            uint32_t *rows, uint64_t *used);
/* out[c * k + i] (device) = cols[c][rows[i] - offset] for the rows this rank holds
 * (offset <= rows[i] < offset + n_local), bit pattern 0 elsewhere: an integer SUM of the bit
 * patterns over the ranks assembles the global rows exactly (-0 and NaN payloads included) */
int st_dev_gather_rows(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n_local, uint64_t offset,
                       const uint32_t *rows, int32_t k, float *out);
/* exact nearest centroid (KdTree.findNearest semantics) of each local point */
int st_dev_kmeans_assign(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n, int32_t k,
                         const float *centroids, uint32_t *labels);
/* per (segment, dim, cluster): f64 sum in ascending point order, sum|x|, smallest ulp exponent; counts */
int st_dev_kmeans_partials(st_ctx *ctx, const float *const *cols, int32_t d, uint64_t n, int32_t nseg, int32_t k,
                           const uint32_t *labels, double *sums, double *sabs, int32_t *emin, uint32_t *counts);
/* continue running[i] (pair = cluster*d + dim) over this rank's members of segment seg, exactly as the
 * sequential f64 sum; emin / sabs are the global (reduced) partials [d][k] */
int st_dev_kmeans_seqsum(st_ctx *ctx, int32_t d, int32_t k, int32_t seg, const uint32_t *pairs, uint32_t npairs,
                         double *running, const int32_t *emin, const double *sabs);
/* global (reduced) partials -> centroids where the sum is certified exact; the rest listed in pending
 * (ascending pair order, *npending on the host); clusters with count 0 are left untouched */
int st_dev_kmeans_finish(st_ctx *ctx, int32_t d, int32_t k, const double *sums, const double *sabs,
                         const int32_t *emin, const uint32_t *counts, float *centroids, uint32_t *pending,
                         uint32_t *npending);
int st_dev_kmeans_average(st_ctx *ctx, int32_t d, int32_t k, const uint32_t *pairs, uint32_t npairs,
                          const double *running, const uint32_t *counts, float *centroids);
int st_dev_cluster1d_codebook(st_ctx *ctx, const float *centroids, const uint32_t *labels, uint64_t total,
                              float *codebook256, uint8_t *labels8);
/* writeSog texels of the local rows at their global sorted positions pos[i] (other texels untouched);
 * lo/hi: global NaN-ignoring x/y/z extents; label arrays per local row (NULL skips that texture);
 * fills meta->means_min/max */
int st_dev_sog_scatter(st_ctx *ctx, const st_table *local, const uint32_t *pos, const double lo[3], const double hi[3],
                       const uint8_t *scale_labels, const uint8_t *color_labels, const uint32_t *shn_labels,
                       st_sog_meta *meta, const st_sog_textures *out);
int st_dev_sog_shn_centroids(st_ctx *ctx, const uint8_t *codebook_labels, int32_t sh_coeffs, int32_t palette,
                             uint8_t *out);

/* ---- multi-GPU writeSog, native (SURVEY 8b st_set_devices, 8e) ----------------
 * The reference picks one device for its clusterer (write-sog.ts:241-243, :313); here the
 * splat rows are sharded across GPUs and the library runs the whole writeSog: k-means
 * centroid sums all-reduced over RCCL every iteration (exact: DESIGN.md (e)), rank 0 orders
 * the global table (Morton) and gathers the texels.  Results equal st_sog on the global table.
 * Rows of the global table = the input tables concatenated in order (combine(), index.ts:
 * 158-210: float32 columns by name, absent columns zero, band from the union of names). */
typedef struct st_comm st_comm;
typedef struct st_group st_group;
/* process-wide: st_sog / st_sog_bundle shard their rows over GPUs 0..ngpu-1 (one host thread
 * and stream per GPU, RCCL communicators from ncclCommInitAll); 1 (default) = one device */
int st_set_devices(int32_t ngpu);
int st_get_devices(int32_t *ngpu);
/* one process per GPU: rank 0 creates the id, the launcher distributes it, every rank joins */
int st_comm_unique_id(uint8_t id[128]);
int st_comm_init_rank(st_ctx *ctx, int32_t world, int32_t rank, const uint8_t id[128], st_comm **out);
/* the same job of one-rank processes with the bytes exchanged through host shared memory
 * instead of RCCL (several ranks on one GPU, which RCCL refuses: the process layout of the
 * N-GPU job rehearsed on one card).  Every rank passes the same `name` ([A-Za-z0-9_.-], unique
 * per job; rank 0 creates /dev/shm/st_<name>, which is unlinked once every rank has attached),
 * slot_bytes (per-rank staging slot, multiple of 4096; 0 = 32 MiB) and timeout_s (longest wait
 * for a peer before the job is aborted; <= 0 = 600 s).  The ranks must all attach within
 * timeout_s when it is set (> 0), within 120 s when it is not; the environment variable
 * ST_SHM_ATTACH_S overrides the attach wait.  A peer process that exits, or a rank that fails,
 * makes every rank's next exchange fail. */
int st_comm_init_host(st_ctx *ctx, int32_t world, int32_t rank, const char *name, uint64_t slot_bytes,
                      double timeout_s, st_comm **out);
void st_comm_destroy(st_comm *comm);
/* ranks in the communicator (ncclCommCount for RCCL): the bench reports it as `rccl_ranks` */
int st_comm_count(const st_comm *comm, int32_t *count);
/* the RCCL the library's collectives run on (loaded on first use, no GPU needed): its
 * ncclGetVersion (e.g. 22707 = 2.27.7) and the real path of the file.  Both hosts load the same
 * file by path -- /opt/rocm/lib/librccl.so.1 unless ST_RCCL names another, or ST_RCCL=process
 * (the copy of soname librccl.so.1 already in the process: torch's under Python) -- under a
 * handle of its own (RTLD_LOCAL).  path may be NULL.  ST_ERR_INTERNAL if it cannot be loaded. */
int st_rccl_info(int32_t *version, char *path, uint64_t path_len);
/* one rank's part of a sharded writeSog: `locals` are this rank's tables (device columns; its
 * files or file parts, in global order); every rank calls it with the same iters and draws.
 * meta / out (device textures) are written on rank 0 only. */
int st_dev_sog_sharded(st_ctx *ctx, st_comm *comm, const st_table *const *locals, int32_t nlocal, int32_t iters,
                       const double *draws, uint64_t ndraws, uint64_t *used, st_sog_meta *meta,
                       const st_sog_textures *out);
/* a set of ranks in this process: devices[r] is rank r's GPU (repeats allowed with
 * host_staged != 0: the exchange then goes through host memory -- several ranks on one GPU) */
int st_group_create(const int32_t *devices, int32_t n, int32_t host_staged, st_group **out);
void st_group_destroy(st_group *g);
/* writeSog of the concatenation of host tables; rank r takes global rows [splits[r], splits[r+1])
 * (splits: n + 1 ascending bounds from 0 to the row count; NULL = an even split); textures to
 * host memory (as st_sog) or the .sog archive (as st_sog_bundle) */
int st_group_sog(st_group *g, const st_table *const *tables, int32_t ntables, const uint64_t *splits, int32_t iters,
                 const double *draws, uint64_t ndraws, uint64_t *used, st_sog_meta *meta,
                 const st_sog_textures *out);
int st_group_sog_bundle(st_group *g, const st_table *const *tables, int32_t ntables, const uint64_t *splits,
                        int32_t iters, const double *draws, uint64_t ndraws, uint64_t *used, uint16_t dos_time,
                        uint16_t dos_date, uint8_t **out, uint64_t *out_size);
/* the same with each input table's processDataTable actions (process.ts:64-145: the CLI's
 * `a.ply [actions] b.ply [actions] out.sog`) applied on the GPUs to each rank's part of that
 * input before writeSog: transform and the filters are row-local (the filtered
 * parts concatenate to the filtered input; the shard offsets come from the all-gathered survivor
 * counts); nactions[t] == 0 leaves table t as it is.  With one input its list may also carry the
 * output's actions (combine of one table is the table, index.ts:158-160). */
int st_group_sog_bundle_process(st_group *g, const st_table *const *tables, int32_t ntables, const uint64_t *splits,
                                const st_action *const *actions, const int32_t *nactions, int32_t iters,
                                const double *draws, uint64_t ndraws, uint64_t *used, uint16_t dos_time,
                                uint16_t dos_date, uint8_t **out, uint64_t *out_size);

/* ---- WebP lossless, CRC-32, the .sog container ---------------
 * WebP: a valid lossless VP8L stream (predictor transform + canonical prefix
 * codes) that decodes to exactly the input RGBA; parity is at the decoded-pixel
 * level, the bytes differ from libwebp's.  Images are 1..16384 on each side. */
/* worst-case .webp size for a width x height image (0 if out of range) */
uint64_t st_webp_max_size(int32_t width, int32_t height);
/* device RGBA8 (stride bytes per row, multiple of 4) -> device .webp bytes (cap >= st_webp_max_size) */
int st_dev_webp_lossless(st_ctx *ctx, const uint8_t *rgba, int32_t width, int32_t height, int32_t stride,
                         uint8_t *out, uint64_t cap, uint64_t *size);
/* host form of WebPEncodeLosslessRGBA: *out is malloc'd, release with st_free */
int st_webp_lossless(st_ctx *ctx, const uint8_t *rgba, int32_t width, int32_t height, int32_t stride,
                     uint8_t **out, uint64_t *size);
/* zlib-compatible CRC-32 of n device bytes, continuing from crc_in (0 = fresh; crc.ts value()) */
int st_dev_crc32(st_ctx *ctx, const uint8_t *data, uint64_t n, uint32_t crc_in, uint32_t *out);
/* host: the store-only ZIP of zip-writer.ts (entries in order, CRCs given); *out malloc'd */
int st_zip_store(const char *const *names, const uint8_t *const *data, const uint64_t *sizes,
                 const uint32_t *crcs, int32_t count, uint16_t dos_time, uint16_t dos_date,
                 uint8_t **out, uint64_t *out_size);
/* host: meta.json text of writeSog (JS number formatting); *out malloc'd, NUL-terminated */
int st_sog_meta_json(const st_sog_meta *meta, uint64_t count, char **out, uint64_t *out_size);
/* the .sog archive of textures resident on the device (st_dev_sog's outputs):
 * WebP encode + CRC on the device, ZIP layout on the host.  dos_time/dos_date are
 * the ZipWriter's clock fields (zip-writer.ts:39-41).  *out malloc'd (st_free). */
int st_dev_sog_bundle(st_ctx *ctx, const st_sog_meta *meta, uint64_t count, const st_sog_textures *tex,
                      uint16_t dos_time, uint16_t dos_date, uint8_t **out, uint64_t *size);
/* as st_dev_sog_bundle, but *out borrows the context's pinned archive buffer (valid
 * until the next bundle call on ctx; no copy) -- what a writer hands to write(2) */
int st_dev_sog_bundle_view(st_ctx *ctx, const st_sog_meta *meta, uint64_t count, const st_sog_textures *tex,
                           uint16_t dos_time, uint16_t dos_date, const uint8_t **out, uint64_t *size);
/* writeSog into a file (write-sog.ts:110-370 and the CLI's write of the .sog, index.ts:101-154):
 * st_dev_sog with its archive streamed to the open file descriptor fd (written from offset 0) --
 * the five textures that are final before the SH palette k-means (means_l/u, quats, scales,
 * sh0) are WebP-encoded on a side context and written while the k-means runs, the shN
 * textures, meta.json and the central directory after it.  The file holds the same bytes as
 * st_dev_sog_bundle's archive and is cut to its length; *size = that length.  fd must be
 * seekable (a regular file opened for writing; the archive goes out with pwrite at absolute
 * offsets): a pipe or socket fails with ST_ERR_ARG before any work.  The caller opens and
 * closes fd; open it without O_TRUNC (the call cuts the file itself: on ext4 a file truncated to
 * zero and rewritten is flushed at close, and its old pages are freed at the open). */
int st_dev_sog_file(st_ctx *ctx, const st_table *table, int32_t iters, const double *draws, uint64_t ndraws,
                    uint64_t *used, st_sog_meta *meta, const st_sog_textures *out, int32_t fd, uint16_t dos_time,
                    uint16_t dos_date, uint64_t *size);
/* the same from a host table (uploaded; st_set_devices > 1: the group's archive written whole,
 * from offset 0, the file cut to its length; the same fd requirement) */
int st_sog_file(st_ctx *ctx, const st_table *table, int32_t iters, const double *draws, uint64_t ndraws,
                uint64_t *used, int32_t fd, uint16_t dos_time, uint16_t dos_date, uint64_t *size);
/* the whole writeSog(.sog) from a host table: st_sog + st_dev_sog_bundle */
int st_sog_bundle(st_ctx *ctx, const st_table *table, int32_t iters, const double *draws, uint64_t ndraws,
                  uint64_t *used, uint16_t dos_time, uint16_t dos_date, uint8_t **out, uint64_t *size);
void st_free(void *p);

/* ---- PLY ingest and the compressed-PLY reader ----------------
 * Same header grammar and errors as readPly (binary little-endian bodies; the
 * "format" line is not checked, as in the reference).  A body shorter than the
 * header declares is an error here (the reference silently keeps stale bytes). */
int st_ply_parse_header(const uint8_t *data, uint64_t len, st_ply_header *out);
int st_ply_read_header(int32_t fd, st_ply_header *out);   /* pread of the first <= 128 KiB */
uint64_t st_ply_row_bytes(const st_ply_header *h, int32_t element);
/* element rows (row_bytes each, 4-byte aligned, device) -> per-property device columns */
int st_dev_ply_transpose(st_ctx *ctx, const st_ply_header *h, int32_t element, const uint8_t *rows,
                         uint64_t nrows, void *const *cols);
/* element `element` of the file fd -> device columns (pinned double-buffered chunks, H2D, transpose) */
int st_dev_ply_read(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, void *const *cols);
/* the same into host columns (readPly's TypedArrays) */
int st_ply_read(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, void *const *host_cols);
/* readPly with the values left in HBM (replaces read-ply.ts:111-191 for a host that defers the
 * host copy): element `element` goes to the device columns only, and host_cols are registered
 * as that element's lazy columns -- their memory is NOT written until st_ply_materialize.  The
 * writeSog host forms (st_sog, st_sog_bundle, st_sog_file) given a lazy column run on its device
 * copy directly; every other host form copies it down first.  Each lazy column holds a device
 * block of its own until it is materialized or st_ply_forget-ten (later reads do not touch it);
 * the caller keeps the host column alive until then.
 * A lazy column belongs to the context that read it.  Any other context, and an explicit group
 * (st_group_sog*), refuses a table that holds one, or a view of one, with ST_ERR_ARG and writes
 * nothing: st_ply_materialize it on its own context first.  The default group (st_set_devices,
 * ST_NUM_GPUS) is given host bytes, so st_sog / st_sog_bundle / st_sog_file copy the caller
 * context's lazy columns down before its ranks upload them (st_ctx_last_host_reuse: 0, 0).
 * A host form that overwrites a lazy column whole drops its device copy without copying; one that
 * overwrites only part of it (a view) copies the column down first, so the other rows keep the
 * read's values. */
int st_ply_read_resident(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, void *const *host_cols);
/* a lazy column's values copied into its host memory (then an ordinary host column: the caller
 * may change it); no-op for any other pointer */
int st_ply_materialize(st_ctx *ctx, const void *host_col);
/* drop the lazy or mirrored column at host_col without copying (its memory is being released) */
int st_ply_forget(st_ctx *ctx, const void *host_col);
/* decompressPly: chunk = the 18 float columns min_x..max_b in decompress-ply.ts:14-33 order,
 * vertex = packed_position, packed_rotation, packed_scale, packed_color; sh = nsh (0/9/24/45)
 * uint8 f_rest columns; out = x y z f_dc_0..2 opacity rot_0..3 scale_0..2 then f_rest_0.. */
int st_dev_decompress_ply(st_ctx *ctx, uint64_t n, const float *const *chunk, const uint32_t *const *vertex,
                          const uint8_t *const *sh, int32_t nsh, float *const *out);
int st_decompress_ply(st_ctx *ctx, uint64_t n, const float *const *chunk, const uint32_t *const *vertex,
                      const uint8_t *const *sh, int32_t nsh, float *const *out);

/* ---- the PLY writer (writers/write-ply.ts, the 'ply' case of index.ts:126-133) ----
 * st_ply_header_text (host only, no context): the header text of write-ply.ts:19-35 for one
 * element -- "ply", "format binary_little_endian 1.0", a "comment <c>" line per comment, "element
 * <element> <t->n>" (element NULL = "vertex"), a "property <type> <name>" line per column with
 * the type names of write-ply.ts:5-16 (char uchar short ushort int uint float double),
 * "end_header"; every line ends in '\n'.  Only t's n, names and types are read.
 * st_ply_element_text: the "element ..." and "property ..." lines alone, for a host that composes
 * a header of several elements.  Both results are malloc'd (st_free); *size excludes the NUL.
 * st_dev_ply_rows: the kernel alone, the inverse of st_dev_ply_transpose -- rows [row0, row0 +
 * nrows) of a device table of any column types as nrows x R row-major bytes (write-ply.ts:54-62:
 * the columns' elements back to back in column order, no padding) at dev_rows (device, 4-byte
 * aligned), on the context stream.  Columns are aligned to their type.  R > 12 KiB returns
 * ST_ERR_UNSUPPORTED; zero rows or zero columns is a no-op.
 * st_dev_ply_rows_file / st_ply_rows_file: all rows of a device / host table (uploaded once)
 * written to out_fd at its current position, the rows only.  They are interleaved a piece at a
 * time into a small device staging buffer and come down through st_compressed_ply_file's pinned
 * slots while a host thread writes the slot before; the n x R bytes never exist in HBM at once.
 * out_fd as for st_compressed_ply_file: seekable, open for writing, not O_APPEND (ST_ERR_ARG
 * before any work); its position ends after the output and a longer file is cut there.
 * st_ply_file: processDataTable on a host table, then header + rows (one element named "vertex",
 * the CLI's shape); the columns and their order are the processed table's.  *out_m = its rows,
 * *size = the bytes written.
 * st_ply_ply_file: the CLI's `in.ply [actions] out.ply` -- the element's rows go from the file
 * into HBM (st_dev_ply_read), stay resident through the actions and the interleave, and only the
 * output's bytes cross back.  element < 0 selects the element named "vertex".
 * One device writes: the st_set_devices group is not used by these calls.
 * One divergence from the reference: write-ply.ts:40 wraps a column's whole ArrayBuffer, so a
 * column that is an offset view would be written from its buffer's start; here a column's own
 * elements are written. */
int st_ply_header_text(const st_ttable *t, const char *element, const char *const *comments, int32_t ncomments,
                       char **out, uint64_t *size);
int st_ply_element_text(const st_ttable *t, const char *element, char **out, uint64_t *size);
int st_dev_ply_rows(st_ctx *ctx, const st_ttable *dev_table, uint64_t row0, uint64_t nrows, uint8_t *dev_rows);
int st_dev_ply_rows_file(st_ctx *ctx, const st_ttable *dev_table, int32_t out_fd, uint64_t *size);
int st_ply_rows_file(st_ctx *ctx, const st_ttable *host_table, int32_t out_fd, uint64_t *size);
int st_ply_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                const char *const *comments, int32_t ncomments, int32_t out_fd, uint64_t *out_m, uint64_t *size);
int st_ply_ply_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, const char *const *comments, int32_t ncomments, int32_t out_fd,
                    uint64_t *out_m, uint64_t *size);

/* ---- the CSV writer (writers/write-csv.ts, the 'csv' case of index.ts:117-118) ----
 * The file is the header line -- the column names joined by ',' and a '\n', written raw (no
 * quoting: write-csv.ts:9-10) -- and per row the cells '' + column[i] joined by ',' and a '\n'
 * (write-csv.ts:15-22).  A cell is ECMA-262 Number::toString of the element as a JS number: an
 * integer column's plain decimal; a float32 widened exactly to a double first (0.1f is
 * 0.10000000149011612); the shortest digits that round back to the double, the closest among
 * those, fixed up to 21 digits and down to 1e-6, exponent form outside (1e+21, 1e-7); NaN,
 * Infinity, -Infinity, 0 for both zeros.  At most 25 bytes.
 * st_csv_max_row_bytes (host only, no context): the longest row the table's types admit -- per
 * column the longest cell of its type (4 3 6 5 11 10 25 25 in st_ply_type order) plus one
 * separator; 0 for a bad table.  Rows above 48 KiB by this bound (more than 1,890 float64
 * columns) are ST_ERR_UNSUPPORTED in every call below.
 * st_csv_header_text (host only): the header line; malloc'd (st_free), *size excludes the NUL.
 * A table without columns is ST_ERR_ARG here and below (the reference's DataTable refuses it).
 * st_dev_csv_rows: the kernels alone -- the text of rows [row0, row0 + nrows) of a device table of
 * any column types, contiguous at dev_out (device, 4-byte aligned).  *size = the bytes the rows
 * need; above cap the call returns ST_ERR_ARG and writes nothing.  No byte outside
 * [dev_out, dev_out + *size) is written.  The call returns once the size is known; the text is
 * complete in stream order.
 * st_dev_csv_file: header + all rows of a device table written to out_fd from its position.  The
 * rows become text a piece at a time (as many rows as fit one pinned slot by the worst-case
 * width) in two device staging buffers and come down through st_compressed_ply_file's pinned
 * slots while a host thread writes the slot before; the whole text never exists in HBM.
 * out_fd as for st_compressed_ply_file: seekable, open for writing, not O_APPEND (ST_ERR_ARG
 * before any work); its position ends after the output and a longer file is cut there.
 * st_csv_file: processDataTable on a host table (uploaded once), then header + rows.  *out_m =
 * the processed table's rows, *size = the bytes written.
 * st_ply_csv_file: the CLI's `in.ply [actions] out.csv` -- the element's rows stay resident from
 * the file to the text; element < 0 selects the element named "vertex".
 * One device writes: the st_set_devices group is not used by these calls. */
uint64_t st_csv_max_row_bytes(const st_ttable *t);
int st_csv_header_text(const st_ttable *t, char **out, uint64_t *size);
int st_dev_csv_rows(st_ctx *ctx, const st_ttable *dev_table, uint64_t row0, uint64_t nrows, uint8_t *dev_out,
                    uint64_t cap, uint64_t *size);
int st_dev_csv_file(st_ctx *ctx, const st_ttable *dev_table, int32_t out_fd, uint64_t *size);
int st_csv_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t out_fd,
                uint64_t *out_m, uint64_t *size);
int st_ply_csv_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, int32_t out_fd, uint64_t *out_m, uint64_t *size);

/* ---- the HTML viewer writer (writers/write-html.ts, the 'html' case of index.ts:135-143) ----
 * The file is the viewer's page with its style link, its script tag and its settings fetch
 * replaced by the inlined css, js and JSON.stringify(experienceSettings), and fetch(contentUrl)
 * by fetch("data:application/ply;base64,<text>") where <text> is the RFC 4648 base64 (A-Z a-z 0-9
 * + /, '=' padding: Buffer.toString('base64')) of the .compressed.ply file of the table.  The
 * viewer template (html, css, js: @playcanvas/supersplat-viewer's exports) is the caller's; all
 * text is UTF-8, NUL-terminated.
 * st_base64_size (host only, no context): 4 * ceil(nbytes / 3).
 * st_dev_base64: the kernel alone.  segs (at most 4, device pointers, any alignment, a length may
 * be 0) make one byte stream back to back; the text of its bytes [byte0, byte0 + nbytes) is
 * written contiguously at dev_out (device, 4-byte aligned) on the context stream.  byte0 is a
 * multiple of 3; nbytes is a multiple of 3 unless the range ends the stream, where the padding
 * goes.  *size = st_base64_size(nbytes); above cap, for a misaligned dev_out and for a range
 * outside these rules the call returns ST_ERR_ARG and writes nothing.  No byte outside
 * [dev_out, dev_out + *size) is written.
 * st_html_parts (host only): write-html.ts:11-14,24-36,46-55.  pad(text, 12) puts 12 spaces
 * before every '\n'-separated line, empty ones too.  The settings are JSON.stringify's text in
 * the reference's key order: {"camera":{"fov":50,"position":[..],"target":[..],"startAnim":"none"},
 * "background":{"color":[0.4,0.4,0.4]},"animTracks":[]}; a number is Number::toString (the CSV
 * writer's digits), null when not finite, 0 for -0.  The replaces run in order, each on the result
 * of the one before, as String.prototype.replace with a string pattern: the first occurrence
 * only, a missing pattern changes nothing, and in the inserted text $$ is '$', $& the pattern, $`
 * the text before the match and $' the text after it; every other '$' stays.  The page is
 * returned split around the payload: *prefix ends with fetch("data:application/ply;base64, and
 * *suffix begins with ").  Without a fetch(contentUrl) *embeds = 0, *prefix is the whole page and
 * *suffix is empty.  Both are malloc'd (st_free); the sizes exclude the NUL.  camera / target: 3
 * doubles each.
 * st_html_file / st_ply_html_file: the chain of st_compressed_ply_file /
 * st_ply_compressed_ply_file (the actions, the Morton order, the chunk pack; the same errors, the
 * same *out_m / *out_sh_coeffs), then prefix + base64(header | chunk | vertex | sh) + suffix
 * written from out_fd's position.  The compressed file never exists on the host: the arrays stay
 * in HBM, the text is made a piece at a time (one pinned slot of text from slot / 4 * 3 stream
 * bytes) in two device staging buffers and comes down through st_compressed_ply_file's pinned
 * slots while a host thread writes the slot before.  Without a fetch(contentUrl) the chain still
 * runs (its errors surface, as the reference still runs writeCompressedPly) and the page alone is
 * written.  out_fd as for st_compressed_ply_file: seekable, open for writing, not O_APPEND
 * (ST_ERR_ARG before any work); its position ends after the output and a longer file is cut
 * there.  *size = the bytes written.  version as for st_compressed_ply_file.
 * One device writes: the st_set_devices group is not used by these calls. */
typedef struct st_bytes_seg {
    const uint8_t *ptr;
    uint64_t len;
} st_bytes_seg;
uint64_t st_base64_size(uint64_t nbytes);
int st_dev_base64(st_ctx *ctx, const st_bytes_seg *segs, int32_t nseg, uint64_t byte0, uint64_t nbytes,
                  uint8_t *dev_out, uint64_t cap, uint64_t *size);
int st_html_parts(const char *html, const char *css, const char *js, const double *camera, const double *target,
                  char **prefix, uint64_t *prefix_size, char **suffix, uint64_t *suffix_size, int32_t *embeds);
int st_html_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, const char *html,
                 const char *css, const char *js, const double *camera, const double *target, int32_t out_fd,
                 const char *version, uint64_t *out_m, int32_t *out_sh_coeffs, uint64_t *size);
int st_ply_html_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                     int32_t nactions, const char *html, const char *css, const char *js, const double *camera,
                     const double *target, int32_t out_fd, const char *version, uint64_t *out_m,
                     int32_t *out_sh_coeffs, uint64_t *size);

/* ---- the other input formats: .splat, .ksplat, .spz (index.ts:52-76) ----------
 * Each reader decodes packed per-splat records into 14 + nsh float32 columns in its own order:
 * x y z scale_0..2 f_dc_0..2 opacity rot_0..3 f_rest_0..nsh-1 (nsh = 0, 9, 24 or 45).
 *
 * st_*_layout are host-only (no context, no GPU).  They check what the reference checks, in its
 * order, and return the row count and nsh; an input the reference throws on returns ST_ERR_ARG
 * (ST_ERR_UNSUPPORTED for a version or compression mode it does not know) with the reference's
 * message in st_last_error() -- for the RangeErrors of its typed-array views, V8's text.  They
 * are the only gate before a launch: every decode and read call runs them first, and after ST_OK
 * no kernel reads a byte outside the `len` bytes it was given, whatever the file says.
 *   .splat   needs the file size only (a multiple of 32, not 0).
 *   .ksplat  data = the file (at least its main header and section headers).  One deviation: a
 *            section whose harmonics degree is above 3 is refused (the reference fails on the
 *            first record of a non-empty one and loses track of its offsets after an empty one).
 *   .spz     data = the INFLATED stream ("NGSP"...): gunzip is the caller's (the reference hands
 *            it to the platform's DecompressionStream, read-spz.ts:16-28).  A degree above 3 gives
 *            nsh = 0, as the reference's table lookup does.
 * st_dev_*_decode: record bytes already in HBM -> device columns, on the context stream.
 *   splat    rows: nrows 32-byte rows, 16-byte aligned.
 *   ksplat   file: the whole file in HBM (4-byte aligned), len bytes; headers: a HOST copy of its
 *            first headers_len bytes, covering at least the main and section headers -- the
 *            section walk and the partial-bucket walk (read-ksplat.ts:196-269) run on the host.
 *            When headers_len does not reach a section's partial bucket sizes they are copied
 *            down from HBM (one small synchronous copy per such section).
 *   spz      file: the inflated stream in HBM (4-byte aligned); its 16-byte header is read back.
 * st_*_read write host columns, st_dev_*_read device columns (both return when the columns are
 * complete).  .splat comes from a file descriptor: its rows stream page cache -> pinned double
 * buffer -> HBM -> decode in st_dev_ply_read's chunks.  .ksplat / .spz come from a host buffer
 * (the file, the inflated stream), uploaded once. */
int st_splat_layout(uint64_t file_size, uint64_t *n, int32_t *nsh);
int st_ksplat_layout(const uint8_t *data, uint64_t len, uint64_t *n, int32_t *nsh);
int st_spz_layout(const uint8_t *data, uint64_t len, uint64_t *n, int32_t *nsh);
int st_dev_splat_decode(st_ctx *ctx, const uint8_t *rows, uint64_t nrows, float *const *cols);
int st_dev_ksplat_decode(st_ctx *ctx, const uint8_t *headers, uint64_t headers_len, const uint8_t *file, uint64_t len,
                         float *const *cols);
int st_dev_spz_decode(st_ctx *ctx, const uint8_t *file, uint64_t len, float *const *cols);
int st_splat_read(st_ctx *ctx, int32_t fd, float *const *host_cols);
int st_dev_splat_read(st_ctx *ctx, int32_t fd, float *const *cols);
int st_ksplat_read(st_ctx *ctx, const uint8_t *data, uint64_t len, float *const *host_cols);
int st_dev_ksplat_read(st_ctx *ctx, const uint8_t *data, uint64_t len, float *const *cols);
int st_spz_read(st_ctx *ctx, const uint8_t *data, uint64_t len, float *const *host_cols);
int st_dev_spz_read(st_ctx *ctx, const uint8_t *data, uint64_t len, float *const *cols);

/* ---- the .sog reader (no reference counterpart: the reference writes SOG, write-sog.ts:110-370,
 * and its CLI at this version cannot read it back) -------------------------------------------
 * A .sog is a store-only ZIP of meta.json and five (seven with SH bands) lossless WebP textures;
 * the unbundled form is the same files in a directory (index.ts:88 treats both as SOG).  The
 * reader gives 14 + nsh float32 columns in the other readers' order: x y z scale_0..2 f_dc_0..2
 * opacity rot_0..3 f_rest_0..nsh-1 (nsh = 0, 9, 24 or 45).
 *
 * The decode rules are this project's own: the exact inverses of the writer's quantisers
 * (write-sog.ts:162-268, :319-348) in JS-number (f64) arithmetic, one Float32Array store per
 * value, Math.exp / Math.log as V8 has them.  Texel i (row-major in the width x height textures)
 * is splat i, bytes R G B A:
 *   x y z      q = means_l[a] | means_u[a] << 8;  v = mins[a] + (maxs[a] - mins[a]) * (q / 65535);
 *              out = Math.sign(v) * (Math.exp(Math.abs(v)) - 1)   (NaN / Inf in mins / maxs propagate)
 *   rot_0..3   t = quats.A & 3 (the writer stores 252 + maxComp; any other alpha byte is read the
 *              same way); c_k = (byte_k / 255 - 0.5) * Math.sqrt(2) for k = R, G, B;
 *              rot_t = Math.sqrt(Math.max(0, 1 - (c0*c0 + c1*c1 + c2*c2))), the other three in
 *              ascending index take c0, c1, c2; no renormalisation
 *   scale_k    scales_codebook[scales.k];  f_dc_k = sh0_codebook[sh0.k]   (float32 copies)
 *   opacity    p = sh0.A / 255;  e = Math.min(1 - 1e-6, Math.max(1e-6, p));  Math.log(e / (1 - e))
 *   f_rest_{j + ch * C}  (C = 3 / 8 / 15 coefficients of bands 1 / 2 / 3, ch = 0..2)
 *              label = shN_labels.R | shN_labels.G << 8; the texel at row label >> 6, column
 *              (label & 63) * C + j of shN_centroids (width 64 * C) gives shn_codebook[texel[ch]].
 *              A label >= palette_size writes zeros for its row and is counted.
 *
 * st_zip_index (host only): the entries of a ZIP archive in memory, from its central directory:
 * name (name_len bytes at data + name_offset, not NUL-terminated), CRC-32, and where the entry's
 * `size` bytes lie (data + offset).  entries may be NULL to query *count; cap < *count is
 * ST_ERR_ARG.  Stored entries only: a compressed entry or a zip64 archive is ST_ERR_UNSUPPORTED;
 * a malformed archive is ST_ERR_ARG.  Every offset and length is checked against len first.
 * st_webp_info / st_webp_decode_lossless (host only): a WebP-lossless file (RIFF container with
 * a VP8L chunk, alone or in a VP8X file; all of RFC 9649) -> its size / its pixels as RGBA8 rows
 * of `stride` bytes (>= 4 * width).  A lossy file is ST_ERR_UNSUPPORTED, a truncated or corrupt
 * one ST_ERR_ARG; nothing is read past len.
 * st_sog_read_layout (host only, no context): the only gate before a launch.  tex_wh: the
 * (width, height) of means_l, means_u, quats, scales, sh0, shN_centroids, shN_labels (the last
 * two ignored for bands 0).  Checks count >= 1; the per-splat textures all width x height with
 * width * height >= count (meta's width / height must agree); bands in 0..3; for bands > 0,
 * 1 <= palette_size <= 65536, the centroid texture 64 * C wide and 64 * its height >= palette_size
 * (meta's shn_width / shn_height must agree).  *n = count, *nsh = 3 * C.
 * st_dev_sog_decode: device textures (RGBA8, 4-byte aligned) -> device columns, one kernel on the
 * context stream; it waits for the kernel and returns ST_ERR_ARG "N shN labels outside the
 * palette" when any label was (the columns are complete, those rows zero).  Only rows
 * [0, count) of the columns are written.
 * st_sog_read / st_dev_sog_read: a whole .sog in a host buffer plus the caller-parsed meta
 * (parsing meta.json's text is the caller's job, as gunzip is for .spz; width / height /
 * shn_width / shn_height of meta are filled from the textures here and need not be set).  The
 * archive is indexed, the textures looked up under the writer's names (means_l.webp
 * means_u.webp quats.webp scales.webp sh0.webp shN_centroids.webp shN_labels.webp), sized
 * (st_webp_info), checked (st_sog_read_layout), decoded on up to 7 host threads, each uploaded as
 * it finishes, and one kernel makes the columns (host_cols / device cols, capacity count rows). */
typedef struct {
    uint64_t name_offset;
    uint32_t name_len;
    uint32_t crc;
    uint64_t offset;
    uint64_t size;
} st_zip_entry;
int st_zip_index(const uint8_t *data, uint64_t len, st_zip_entry *entries, int32_t cap, int32_t *count);
int st_webp_info(const uint8_t *data, uint64_t len, int32_t *width, int32_t *height);
int st_webp_decode_lossless(const uint8_t *data, uint64_t len, uint8_t *rgba_out, int32_t stride);
int st_sog_read_layout(const st_sog_meta *meta, uint64_t count, const int32_t tex_wh[7][2], uint64_t *n,
                       int32_t *nsh);
int st_dev_sog_decode(st_ctx *ctx, const st_sog_meta *meta, uint64_t count, const st_sog_textures *dev_tex,
                      float *const *cols);
int st_sog_read(st_ctx *ctx, const uint8_t *data, uint64_t len, const st_sog_meta *meta, uint64_t count,
                float *const *host_cols);
int st_dev_sog_read(st_ctx *ctx, const uint8_t *data, uint64_t len, const st_sog_meta *meta, uint64_t count,
                    float *const *cols);

/* ---- the .splat and .spz writers (no reference counterpart: the reference reads both formats,
 * readers/read-splat.ts and readers/read-spz.ts, and writes neither) ---------------------------
 * The encode rules are this project's own, anchored on the reference: each field gets the code
 * that the reference's own reader decodes to the nearest value, so writing the columns the
 * reference decoded from a file gives the file's bytes back (tests/golden/readers.*; where a
 * decode loses information -- a signalling NaN, a float32 scale through log, a rotation whose
 * stored part exceeds unit length -- it cannot).
 *
 * v is the column's element as a JS number (float32 / float64 widened exactly, integers taken
 * exactly; any of the eight column types).  All arithmetic is IEEE double, one rounding per
 * operation in the order written, no fused multiply-add.  exp is V8's Math.exp;
 * sigmoid(v) = 1 / (1 + exp(-v)).
 *   Q8(t)  = 0 if t is NaN, else min(255, max(0, floor(t + 0.5)))
 *   u      the unit quaternion: L = sqrt(((r0*r0 + r1*r1) + r2*r2) + r3*r3) with r_k = rot_k;
 *          u_k = r_k / L if L > 0 and L < Infinity, else u = (1, 0, 0, 0)
 * Required columns: x y z scale_0..2 f_dc_0..2 opacity rot_0..3.  A missing one is ST_ERR_ARG and
 * the message names it; the first column of a name wins; other columns (nx, ...) are ignored.
 * The band C (0, 3, 8 or 15 coefficients per channel) follows the first-missing-f_rest_i rule
 * (transform.ts:20).  Columns must be aligned to their type.
 *
 * .splat: 32 bytes per row, little endian, in row order (no importance sort: a caller who wants
 * one permutes first).  f_rest columns are ignored.  n = 0 is ST_ERR_ARG (the reference's reader
 * refuses an empty file).
 *   bytes  0-11  x, y, z as float32: a float32 column's bits unchanged (NaN payloads included),
 *                other types Math.fround(v)
 *         12-23  Math.fround(exp(scale_k))
 *         24-26  Q8((f_dc_k * 0.28209479177387814 + 0.5) * 255)
 *         27     Q8(sigmoid(opacity) * 255)
 *         28-31  Q8((u_k + 1) * 127.5), k = 0..3
 *
 * .spz: version 2 only.  The raw image (what the reference's reader takes after its gunzip) is a
 * 16-byte header and six planes, 16 + n * (19 + 3C) bytes:
 *   header  0-3 4E 47 53 50;  4-7 u32 2;  8-11 u32 n;  12 degree 0..3;  13 fractional_bits;  14-15 0
 *   positions  9 B per splat: x, y, z as the little-endian low 24 bits of k;  k = 0 if v is NaN,
 *              else min(2^23 - 1, max(-2^23, floor(v * 2^fractional_bits + 0.5)))
 *   alphas     Q8(sigmoid(opacity) * 255)
 *   colours    Q8((f_dc_k * 0.15 + 0.5) * 255)
 *   scales     Q8((scale_k + 10) * 16)
 *   rotations  u as above; if u_0 < 0 all four are negated; then Q8((u_k + 1) * 127.5), k = 1, 2, 3
 *   harmonics  for i = 0..3C-1: Q8(f_rest_{(i mod 3) * C + floor(i / 3)} * 128 + 128)
 * fractional_bits is 0..23 (outside: ST_ERR_ARG).  *out_clamped (nullable) counts the position
 * values that were NaN or fell outside [-2^23, 2^23 - 1] before the clamp -- whether or not the
 * positions plane is asked for; the caller decides whether to retry with fewer bits.
 * n >= 2^32 is ST_ERR_UNSUPPORTED; n = 0 writes the header alone.
 *
 * st_spz_image_size (host only): 16 + n * (19 + 3 * sh_coeffs); 0 for an sh_coeffs that is no
 * band or n >= 2^32.
 * st_dev_splat_rows: rows [row0, row0 + nrows) of a device table as nrows x 32 bytes at dev_rows
 * (device, 4-byte aligned), queued on the context stream.
 * st_dev_spz_planes: the same rows' bytes of each plane at planes[0..5] (positions, alphas,
 * colours, scales, rotations, harmonics; device, ANY alignment: where row0's bytes of that plane
 * go; NULL skips one).  Waits for the kernel (the count).
 * st_dev_spz_image: header + planes of the whole table at dev_out (device, any alignment).
 * *size = the bytes the image needs; above cap the call returns ST_ERR_ARG and writes nothing.
 * No byte outside the stated output ranges is ever written by any of them.
 * The file forms follow st_dev_csv_file / st_csv_file / st_ply_csv_file: processDataTable through
 * the same chain, out_fd seekable, open for writing and not O_APPEND (ST_ERR_ARG before any
 * work), written from its position, which ends after the output; a longer file is cut there;
 * *out_m = the row count, *size = the bytes written; one device (the st_set_devices group is not
 * consulted).  The .splat rows are encoded a pinned slot at a time and never exist in HBM at
 * once; the .spz forms write the RAW image, built whole in HBM: what readSpz decodes after its
 * gunzip (st_spz_layout / st_spz_read take it as is).  The gzip member around it, which readSpz
 * itself (read-spz.ts:56-75 stops on a file without the gzip magic) and other .spz consumers
 * expect, is the caller's here; the st_*_spz_gz_file forms below write it. */
uint64_t st_spz_image_size(uint64_t n, int32_t sh_coeffs);
int st_dev_splat_rows(st_ctx *ctx, const st_ttable *dev_table, uint64_t row0, uint64_t nrows, uint8_t *dev_rows);
int st_dev_spz_planes(st_ctx *ctx, const st_ttable *dev_table, int32_t fractional_bits, uint64_t row0,
                      uint64_t nrows, uint8_t *const planes[6], uint64_t *out_clamped);
int st_dev_spz_image(st_ctx *ctx, const st_ttable *dev_table, int32_t fractional_bits, uint8_t *dev_out,
                     uint64_t cap, uint64_t *size, uint64_t *out_clamped);
int st_dev_splat_file(st_ctx *ctx, const st_ttable *dev_table, int32_t out_fd, uint64_t *size);
int st_splat_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t out_fd,
                  uint64_t *out_m, uint64_t *size);
int st_ply_splat_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                      int32_t nactions, int32_t out_fd, uint64_t *out_m, uint64_t *size);
int st_dev_spz_file(st_ctx *ctx, const st_ttable *dev_table, int32_t fractional_bits, int32_t out_fd,
                    uint64_t *size, uint64_t *out_clamped);
int st_spz_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped);
int st_ply_spz_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                    int32_t nactions, int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size,
                    uint64_t *out_clamped);

/* ---- the gzip member around a .spz image: DEFLATE (RFC 1951) on the device ---------------------
 * readSpz takes a gzip member (read-spz.ts:56-75 stops on a file without the gzip magic); the raw
 * forms above leave it to the caller.  These make it on the device.  The stream is this project's
 * own choice among the valid ones, fixed by the rules below, so a host program that follows them
 * (csrc/st_deflate.h's serial encoder) gives the same bytes.
 *
 * Segments.  The input is cut into segments of ST_DEFLATE_SEG bytes, each coded alone: no token
 * refers to bytes before its segment.  Every segment's code ends on a byte boundary: a segment
 * that is not the last and is not stored is followed by an empty stored block (bits 000, zero
 * padding to the byte, then 00 00 FF FF); the last block of the last segment has BFINAL = 1 and is
 * padded with zeros.  n = 0 is the one fixed block 03 00.
 * Tokens are literals and matches of distance 1.  Of a maximal run of L equal bytes inside a
 * segment the first byte is a literal; the other L - 1 are cut greedily into matches of 258; a
 * remainder of at least 3 is one match, a remainder of 1 or 2 is literals.
 * Block type.  A segment is the smallest, in bytes with its byte-boundary trailer, of: stored
 * blocks (LEN at most 65,535, so a full segment takes two); one fixed-code block; one
 * dynamic-code block.  Ties go to the simpler coding, in that order.
 * Dynamic blocks.  Literal/length code: Huffman's tree over the used symbols and one end-of-block,
 * merged from the symbols in (count, symbol) order, of two equal weights the internal node first;
 * if it is deeper than 15, counts are raised to a floor that doubles from
 * max(2, total >> 17) until it is not.  Distance symbols 0 and 1 both get length 1 (HDIST = 2).
 * The lengths of both codes form one sequence, coded with 16 / 17 / 18: a run of zeros is cut
 * greedily into 18s (11..138), a 17 (3..10), then single zeros; a run of another length is that
 * length once, 16s (3..6), then the length again for the rest.  The code-length code is built the
 * same way with the limit 7 and the floor from max(2, total >> 9).  Codes are canonical, written
 * MSB-first into the LSB-first stream; extra bits go LSB-first.
 *
 * st_deflate_bound(n): the all-stored size, which is also the stream's worst case; 2 for n = 0.
 * st_gzip_bound(n) = st_deflate_bound(n) + 18.
 * st_dev_deflate: the stream of dev_in[0..n) at dev_out, *size = its bytes.  dev_in and dev_out are
 * device pointers of ANY alignment; no byte outside [dev_out, dev_out + *size) is written; if the
 * stream does not fit cap, nothing is written and the call returns ST_ERR_ARG (against the bound
 * that never happens).  All offsets are 64-bit.  Waits for the kernels (the size).
 * st_dev_gzip: one gzip member: 1f 8b 08 00 00 00 00 00 00 ff, the stream, the CRC-32 of the
 * input, n mod 2^32.
 * st_dev_spz_gz_file / st_spz_gz_file / st_ply_spz_gz_file: st_dev_spz_file / st_spz_file /
 * st_ply_spz_file with the member around the image: the same arguments, descriptor rules and ring;
 * the raw image and the member are both built in HBM; *size = the file's bytes. */
#define ST_DEFLATE_SEG 65536
uint64_t st_deflate_bound(uint64_t n);
uint64_t st_gzip_bound(uint64_t n);
int st_dev_deflate(st_ctx *ctx, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap, uint64_t *size);
int st_dev_gzip(st_ctx *ctx, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t cap, uint64_t *size);
int st_dev_spz_gz_file(st_ctx *ctx, const st_ttable *dev_table, int32_t fractional_bits, int32_t out_fd,
                       uint64_t *size, uint64_t *out_clamped);
int st_spz_gz_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions,
                   int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped);
int st_ply_spz_gz_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                       int32_t nactions, int32_t fractional_bits, int32_t out_fd, uint64_t *out_m, uint64_t *size,
                       uint64_t *out_clamped);

/* ---- the .ksplat writer (no reference counterpart: the reference reads the format,
 * readers/read-ksplat.ts:103-384, and has no writer for it) ---------------------------------------
 * The rules are this project's own, anchored on the reference's reader as "the .splat and .spz
 * writers" above are: each field gets the code that readKsplat decodes to the nearest value.  v,
 * the arithmetic (IEEE double, one rounding per operation in the order written, no fused
 * multiply-add, V8's exp), Q8(t), sigmoid, the unit quaternion u, the required columns, the band
 * rule and the any-of-eight-column-types rule are those of that section.
 *
 * Parameters
 *   mode        0, 1 or 2, the compression mode (else ST_ERR_ARG)
 *   degree      -1..3; -1: the table's own by the band rule.  A degree below the table's drops the
 *               higher bands with filterBands' column mapping (process.ts:110-136: coefficient j
 *               of channel ch stays f_rest_{ch * C_table + j}); above the table's: ST_ERR_ARG
 *   block_size  a float32 B (a caller holding a double rounds it to float32 first), finite and
 *               > 0 (else ST_ERR_ARG); 5.0 is the usual choice
 *   sh_min, sh_max  float32, mode 2 only: both finite and non-zero with sh_min < sh_max (else
 *               ST_ERR_ARG: the reader substitutes -1.5 / 1.5 for a zero header field,
 *               read-ksplat.ts:135-136, so a zero would not be read back).  Modes 0 and 1 ignore
 *               them and write -1.5 and 1.5
 *   n = 0 is ST_ERR_ARG (the reader refuses an empty file, :138); n >= 2^32 is ST_ERR_UNSUPPORTED
 *
 * Grid and buckets (all modes; ONE section; bucket capacity 256)
 *   lo_a      the least finite v on axis a over all rows; 0 if the axis has no finite value
 *   cell_a(v) 0 if v is NaN or v < lo_a, else min(2^21 - 1, floor((v - lo_a) / B)): +Inf lands in
 *             the last cell
 *   key       cell_z * 2^42 + cell_y * 2^21 + cell_x
 *   Rows are stably sorted by key (on equal keys the lower row index first).  A cell holding m
 *   rows gives floor(m / 256) full buckets from its first rows and, if m mod 256 != 0, one partial
 *   bucket of the rest.  In the file all full buckets come first, in key order, rows in sorted
 *   order inside each; then all partial buckets, in key order.  No bucket has size 0.  This is the
 *   layout the reader's walk assumes (:251-269: it advances at most one partial bucket per splat).
 *   The bucket centre is Math.fround(lo_a + (cell_a + 0.5) * B) per axis.
 *   *out_clamped (nullable) counts the position values that are not finite or whose unclamped cell
 *   is >= 2^21; the caller decides whether to write again with a larger block.
 *
 * File (little endian; every byte not listed is 0), F / P the full / partial bucket counts:
 *   main header, 4096 bytes: byte 0 = 0, byte 1 = 1 (version 0.1); u32 at 4 = 1 (maxSections);
 *     u32 at 8 = 1 and u32 at 12 = n (the reference's reader reads neither; the original format's
 *     section count and maximum splat count are believed to sit there -- nothing available when
 *     this was written pins them); u32 at 16 = n; u16 at 20 = mode; f32 at 36 / 40 = sh_min /
 *     sh_max (-1.5 / 1.5 in modes 0 and 1)
 *   section header, 1024 bytes at 4096: u32 at 0 and 4 = n; u32 at 8 = 256; u32 at 12 = F + P;
 *     f32 at 16 = B; u16 at 20 = 12; u32 at 24 = 32767; u32 at 32 / 36 = F / P; u16 at 40 = degree
 *   then the partial bucket sizes (u32 each), the bucket centres (3 x f32 per bucket, full buckets
 *   then partial buckets) and the records; each of these offsets is a multiple of 4.
 *   size = 5120 + 4 P + 12 (F + P) + n * stride; stride = 44 + 4 * 3C, 24 + 2 * 3C or 24 + 3C for
 *   modes 0, 1, 2 (C the file's coefficients per channel)
 *
 * Records (the offsets of COMPRESSION_MODES, :62-99).  H(t) is IEEE round-to-nearest-even from the
 * double to binary16: |t| >= 65520 gives +-Inf, NaN gives 0x7E00, subnormals are produced.
 *   centre, mode 0       float32: a float32 column's bits unchanged, other types Math.fround(v)
 *   centre, modes 1, 2   ps = B / 2 / 32767, c = the row's bucket centre widened to double,
 *                        dec(k) = Math.fround((k - 32767) * ps + c) (the reader's decode, :278).
 *                        f = floor((v - c) / ps + 0.5) + 32767; the code is 0 if f is NaN (v is
 *                        NaN), else k0 = min(65535, max(0, f)) corrected by the reader's own
 *                        decode: of k0 - 1, k0, k0 + 1 inside 0..65535 the one with the least
 *                        |dec(k) - v|; k0 wins a tie, k0 - 1 a tie between the neighbours.  (The
 *                        bare closed form is not always the nearest code: dec's float32 store
 *                        moves values by up to half a float32 step of |c|, which is not small
 *                        beside ps for buckets far from the origin.)  Stored as a u16
 *   scale                t = exp(scale_k); mode 0 Math.fround(t), modes 1 and 2 H(t).  A t that
 *                        rounds to 0 reads back as -10 (:321), not as scale_k
 *   rotation             u in the order rot_0..3 the reader stores back (:296-307), no sign
 *                        change; mode 0 Math.fround(u_k), modes 1 and 2 H(u_k)
 *   colour, opacity      Q8((f_dc_k * 0.28209479177387814 + 0.5) * 255), Q8(sigmoid(opacity) * 255)
 *   harmonics            file component i takes the column the reader's mapping sends it to
 *                        (:343-362: band by band, channel-major inside a band).  Mode 0: float32 as
 *                        for the centre; mode 1: H(v); mode 2: with lo = sh_min and span = sh_max -
 *                        sh_min (the header's float32 values widened, the subtraction in double),
 *                        dec(b) = Math.fround(lo + (b / 255) * span) (:242-243); the byte is 0 if v
 *                        is NaN, else k0 = Q8((v - lo) / span * 255) corrected among k0 - 1, k0,
 *                        k0 + 1 inside 0..255 as the centre code is
 *
 * st_ksplat_image_size (host only): the size above for sh_coeffs = C of the FILE; 0 for a C that
 * is no band, a mode outside 0..2, n = 0, n >= 2^32 or a bucket count above n.
 * st_dev_ksplat_plan: the plan of a device table (x, y, z of any types) on the device: dev_order[r]
 * = the source row of record r, dev_bucket[r] = its bucket, dev_centres = 3 float32 per bucket,
 * dev_partial_sizes = one u32 per partial bucket (all device, 4-byte aligned; order and bucket
 * hold n entries, the bucket tables bucket_cap buckets: n is always enough).  *full, *partial and
 * *out_clamped (nullable) come back; with more buckets than bucket_cap the call sets them, returns
 * ST_ERR_ARG and writes no table.  Waits for the stream.
 * st_dev_ksplat_records: records [rec0, rec0 + nrec) of the file at dev_out (device, ANY
 * alignment), queued on the context stream.  The grid is the CALLER's here, so that a file's own
 * bucket table can be handed in: dev_order (NULL: record r is row r), dev_bucket and dev_centres
 * (modes 1 and 2; nbuckets entries; 4-byte aligned), any float32 block_size and any quant_range
 * > 0 in place of B and 32767 (ps = block_size / 2 / quant_range; the public writer always uses B
 * and 32767).  An order or bucket entry outside its table is the caller's error; it is read as the
 * last row / bucket.
 * st_dev_ksplat_image: the whole image at dev_out (device, any alignment).  *size = the bytes the
 * image needs; above cap the call returns ST_ERR_ARG and writes nothing.
 * No byte outside the stated output ranges is ever written by any of them.
 * The file forms follow st_dev_spz_file / st_spz_file / st_ply_spz_file: the same descriptor checks
 * before any work, the same processDataTable chain, the image built whole in HBM and copied down
 * through the pinned ring, one device.
 * Not written: more than one section, bucket capacities other than 256, an importance order of
 * the rows, sharded output. */
uint64_t st_ksplat_image_size(uint64_t n, int32_t sh_coeffs, int32_t mode, uint64_t full, uint64_t partial);
int st_dev_ksplat_plan(st_ctx *ctx, const st_ttable *dev_table, float block_size, uint64_t bucket_cap,
                       uint32_t *dev_order, uint32_t *dev_bucket, float *dev_centres, uint32_t *dev_partial_sizes,
                       uint64_t *full, uint64_t *partial, uint64_t *out_clamped);
int st_dev_ksplat_records(st_ctx *ctx, const st_ttable *dev_table, int32_t mode, int32_t degree, float sh_min,
                          float sh_max, float block_size, uint32_t quant_range, const uint32_t *dev_order,
                          const uint32_t *dev_bucket, const float *dev_centres, uint64_t nbuckets, uint64_t rec0,
                          uint64_t nrec, uint8_t *dev_out);
int st_dev_ksplat_image(st_ctx *ctx, const st_ttable *dev_table, int32_t mode, int32_t degree, float block_size,
                        float sh_min, float sh_max, uint8_t *dev_out, uint64_t cap, uint64_t *size,
                        uint64_t *out_clamped);
int st_dev_ksplat_file(st_ctx *ctx, const st_ttable *dev_table, int32_t mode, int32_t degree, float block_size,
                       float sh_min, float sh_max, int32_t out_fd, uint64_t *size, uint64_t *out_clamped);
int st_ksplat_file(st_ctx *ctx, const st_ttable *src, const st_action *actions, int32_t nactions, int32_t mode,
                   int32_t degree, float block_size, float sh_min, float sh_max, int32_t out_fd, uint64_t *out_m,
                   uint64_t *size, uint64_t *out_clamped);
int st_ply_ksplat_file(st_ctx *ctx, int32_t fd, const st_ply_header *h, int32_t element, const st_action *actions,
                       int32_t nactions, int32_t mode, int32_t degree, float block_size, float sh_min, float sh_max,
                       int32_t out_fd, uint64_t *out_m, uint64_t *size, uint64_t *out_clamped);

/* ---- inflating a gzip member on the device: INFLATE (RFC 1951) for the .spz reader --------------
 * readSpz gunzips its file first (read-spz.ts:50-75).  These calls do that on the device for ANY
 * deflate stream -- one zlib stream of many dynamic-code blocks with back-references through the
 * 32 KiB window, not only the segments st_dev_gzip writes -- by a method whose result never rests
 * on a guess (csrc/st_inflate.h holds every rule as a host/device function, and a serial host form
 * of the same steps):
 *   find     the compressed bytes are cut into chunks of chunk_bytes.  For every chunk but the
 *            first: the first bit position in the chunk at which a NON-FINAL dynamic-code block
 *            header parses completely (BTYPE 2, HLIT and HDIST at most 29, a complete code-length
 *            code, a valid length sequence, a length for symbol 256, both codes complete or zlib's
 *            one-code case).  A chunk may have none.  Stored and fixed blocks are not looked for.
 *   size     one decoder per candidate, and one at bit 0, decodes block after block and counts
 *            bytes.  After a block that ends at bit p it stops if the block was final (FINAL) or
 *            if p is the candidate of a later chunk (JOINED); candidates below p are passed.
 *   chain    from chunk 0 along the JOINED links to FINAL.  Only these decoders are kept: each
 *            started where the true decode has a block boundary, so the result is the sequential
 *            inflate whatever the finder returned.  A running sum gives each its output offset.
 *   write    the kept decoders decode again into 16-bit symbols: a byte, or 256 + i for a
 *            reference to byte i of the 32 KiB before the decoder's first byte (copies carry such
 *            markers along).
 *   windows  kept chunk after kept chunk, the last 32 KiB of each become bytes; then every other
 *            symbol does, all at once.
 * A decoder gives up after ST_INFLATE_BUDGET * chunk_bytes coded symbols (stored blocks cost none).
 *
 * DECLINED.  These calls return ST_OK, a negative st_status (a bad argument, a HIP error), or
 * ST_DECLINED (1, no message): the device path does not take this input, and the caller inflates it
 * some other way.  Declined: any parse error zlib would report, a decoder over its budget, a chain
 * that breaks, bytes after the final block, an output that is not `expect` bytes, a CRC-32 or ISIZE
 * that does not match, a second member, reserved FLG bits, a method other than 8, a header longer
 * than 4,096 bytes (st_dev_gunzip).  After ST_DECLINED nothing is promised about the output bytes.
 *
 * st_gzip_member_layout (host only): RFC 1952's header with FEXTRA, FNAME, FCOMMENT and FHCRC
 * stepped over -> where the deflate stream lies in the member and the trailer's CRC-32 and ISIZE.
 * st_inflate_head (host only): the first `want` bytes of a raw deflate stream, serially; *got = how
 * many there are.  The .spz reader takes the image's 16-byte header this way, so the rows and the
 * image size are known before anything is allocated.
 * st_dev_inflate: the raw deflate stream dev_in[0..n) into dev_out[0..expect).  st_dev_gunzip: the
 * same for one gzip member, with the trailer checked.  chunk_bytes: 0 = ST_INFLATE_CHUNK; any value
 * from 256 up is taken (below: ST_ERR_ARG).  Device pointers of ANY alignment; no byte outside
 * [dev_out, dev_out + expect) is written.  stats (nullable) is filled as far as the call got.
 * Both wait for the kernels.
 * st_spz_gz_layout (host only): row count and f_rest count of a gzipped .spz FILE from its member
 * layout and its first 16 inflated bytes (st_spz_layout's checks on them, the image size being the
 * trailer's ISIZE); *image_bytes = that size.  Whatever st_spz_layout would refuse is ST_DECLINED
 * here: the caller's host path then reports it in its own words.
 * st_spz_gz_read / st_dev_spz_gz_read: st_spz_read / st_dev_spz_read from the FILE's bytes (host):
 * layout, head, upload, st_dev_gunzip's steps into HBM, then the same decode kernel. */
#define ST_DECLINED 1
#define ST_INFLATE_CHUNK 65536
#define ST_INFLATE_BUDGET 512
typedef struct st_inflate_stats {
    uint64_t chunks;         /* chunks of compressed bytes */
    uint64_t candidates;     /* chunks (after the first) in which the finder found a start */
    uint64_t kept;           /* decoders on the chain */
    uint64_t discarded;      /* decoders run and not kept: 1 + candidates - kept */
    uint64_t markers;        /* symbols of the write pass that refer to the previous window */
    uint64_t stored_blocks;  /* blocks the kept decoders read, by BTYPE */
    uint64_t fixed_blocks;
    uint64_t dynamic_blocks;
} st_inflate_stats;
int st_gzip_member_layout(const uint8_t *host, uint64_t n, uint64_t *stream_off, uint64_t *stream_len, uint32_t *crc,
                          uint32_t *isize);
int st_inflate_head(const uint8_t *host_stream, uint64_t n, uint8_t *out, uint64_t want, uint64_t *got);
int st_dev_inflate(st_ctx *ctx, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect,
                   uint64_t chunk_bytes, st_inflate_stats *stats);
int st_dev_gunzip(st_ctx *ctx, const uint8_t *dev_in, uint64_t n, uint8_t *dev_out, uint64_t expect,
                  uint64_t chunk_bytes, st_inflate_stats *stats);
int st_spz_gz_layout(const uint8_t *file, uint64_t len, uint64_t *n, int32_t *nsh, uint64_t *image_bytes);
int st_spz_gz_read(st_ctx *ctx, const uint8_t *file, uint64_t len, float *const *host_cols, uint64_t chunk_bytes,
                   st_inflate_stats *stats);
int st_dev_spz_gz_read(st_ctx *ctx, const uint8_t *file, uint64_t len, float *const *cols, uint64_t chunk_bytes,
                       st_inflate_stats *stats);

/* ---- column summary --------------------------------------------------------------------------
 * What is in a table, column by column: counts, extremes, mean, deviation, median.  The reference
 * at this version has no such command, so the rules are this project's own, and they are written
 * so that no result depends on the order of the rows (every writer here reorders them) or on the
 * shape of a launch: the sum is the real-number sum rounded once, the median is the true order
 * statistic.  csrc/st_summary.h holds every rule as a host/device function and a serial host form.
 *
 * For one column of any st_ply_type, v_i is the element as a JS number (widened exactly).  All
 * arithmetic is IEEE double, each operation rounds once in the order written, nothing is fused.
 *   rows       n.  nan_count: the NaN elements, any sign or payload.  inf_count: the +-Infinity
 *              elements.  m = n - nan_count - inf_count; everything below is over the m finite ones.
 *   min, max   in the total order in which -0 precedes +0 (Math.min / Math.max).
 *   sum        the exact real sum, rounded once to double, nearest-even: +-Infinity when its
 *              magnitude is 2^1024 - 2^970 or more.  No partial sum exists that could leave the
 *              double range on the way: [1.7e308, 1.7e308, -1.7e308] sums to 1.7e308.
 *   mean       sum / m, one division, m as a double.  n >= 2^53 is ST_ERR_UNSUPPORTED.
 *   ssd        d_i = v_i - mean, t_i = d_i * d_i; the exact real sum of the t_i, rounded once;
 *              +Infinity if any t_i is +Infinity.
 *   std_dev    sqrt(ssd / m): the population deviation.
 *   median     the finite elements sorted in the total order above: element (m - 1) / 2 for odd m,
 *              (a + b) / 2 of elements m / 2 - 1 and m / 2 for even m, computed as written: it may
 *              overflow, and (-0 + +0) / 2 is +0.
 *   m = 0      (n = 0 included): min, max, mean, std_dev, median are NaN; sum and ssd are +0.
 * A table without columns is ST_ERR_ARG.  Columns must be aligned to their type (ST_ERR_ARG, the
 * message names the column).  Duplicate names are allowed and summarised independently.
 *
 * st_dev_summary reads the device columns in place: no column data goes to the host, and the device
 * scratch is a fixed record per column (the columns go through in batches of 128, one grid
 * dimension over a batch).  It works on the context stream and waits for it.  st_summary uploads a
 * host table through the staged copies, about 1 GiB of columns at a time, and runs the same steps.
 * st_ctx_last_summary_stats: the last call's sum paths as JSON -- {"columns", "fast" (int128 in
 * units of the column's lowest set bit), "general" (the superaccumulator), "normalisations" (carry
 * propagations inside a loop), "flush"}.  Switches, read per call: ST_SUM_EXACT=1 sends every
 * column down the general path; ST_SUM_FLUSH=<n> (1 .. 2^30, the default) is the additions a wave's
 * accumulator takes between normalisations.
 * st_summary_text (host only): "column,rows,nanCount,infCount,min,max,mean,stdDev,median\n", then a
 * line per column: the name as it is (not quoted, as in the CSV writer), the counts as decimal
 * integers, the doubles as JavaScript prints them (NaN, Infinity, -0 as 0).  malloc'd (st_free);
 * *size excludes the NUL. */
typedef struct {
    uint64_t rows, nan_count, inf_count;
    double min, max, sum, mean, ssd, std_dev, median;
} st_col_summary;
int st_dev_summary(st_ctx *ctx, const st_ttable *dev_table, st_col_summary *out);
int st_summary(st_ctx *ctx, const st_ttable *host_table, st_col_summary *out);
int st_summary_text(const st_ttable *t, const st_col_summary *s, char **out, uint64_t *size);
const char *st_ctx_last_summary_stats(st_ctx *ctx);

/* ---- importance, decimation and crops -----------------------------------------------------------
 * Making a scene smaller on purpose: the rows that matter most, the rows inside a box or a sphere,
 * the rows in the order a progressive viewer should draw them.  The reference at this version has
 * none of these, so the rules are this project's own.  csrc/st_importance.h holds every rule as a
 * host/device function and a serial host form of the three selections.
 *
 * Every value is the column's element as a JS number (any st_ply_type, widened exactly); all
 * arithmetic is IEEE double, each operation rounds once in the order written, nothing is fused.
 *   score      s = (scale_0 + scale_1) + scale_2; score = exp(s) * sigmoid(opacity), exp and sigmoid
 *              those of csrc/st_jsmath.h (V8's).  The convention of the original .splat converter.
 *              A score is in [+0, +Infinity] or NaN: Infinity * 0 is NaN, and a NaN in any of the four
 *              values gives NaN.  A table without one of the four columns is ST_ERR_ARG (for
 *              ST_ACTION_ORDER_IMPORTANCE and ST_ACTION_DECIMATE too); nothing is launched.
 *   key        NaN ? 0 : bits(score) + 1 as uint64: larger is more important, every NaN is 0.
 *   importance order   descending key; equal keys (NaN among NaN included) by ascending row index: a
 *              total order that depends only on the data.  rank(i) = row i's position in it.
 *   ST_ACTION_ORDER_IMPORTANCE (orderByImportance)   permuteRows by that order; n <= 1 does nothing.
 *   ST_ACTION_DECIMATE (decimate)   keeps the m rows of rank < m in their original row order (a
 *              stable selection, like the filters).  amount_mode ST_DECIMATE_COUNT: amount must be a
 *              finite, non-negative, integer-valued double below 2^53 (else ST_ERR_ARG), m =
 *              min(amount, n).  ST_DECIMATE_FRACTION: 0 <= amount <= 1 (else ST_ERR_ARG, NaN included),
 *              m = min(n, floor(amount * (double)n)), the product in f64.  Another mode is ST_ERR_ARG.
 *              m == n keeps the table as it is (permuteRows by the identity); m == 0 leaves no row.
 *   ST_ACTION_FILTER_BOX (filterBox)   keep iff x >= box_min[0] && x <= box_max[0] && y >= box_min[1]
 *              && y <= box_max[1] && z >= box_min[2] && z <= box_max[2]: faces inclusive, any NaN
 *              (coordinate or bound) false, infinite bounds open a side (Infinity <= Infinity holds),
 *              min > max keeps nothing.  A missing x, y or z column reads as NaN: every row is dropped,
 *              as for filterByValue's missing column.
 *   ST_ACTION_FILTER_SPHERE (filterSphere)   dx = x - center[0], dy, dz alike; keep iff
 *              ((dx*dx + dy*dy) + dz*dz) < radius*radius.  Strict: radius 0 keeps nothing; a negative
 *              radius behaves as its square does; a NaN anywhere keeps nothing; missing columns as
 *              for the box.
 * All four copy the table the way a filter does.  In st_group_sog_bundle_process the box and the
 * sphere are row-local and run in the per-rank slices; ST_ACTION_DECIMATE and
 * ST_ACTION_ORDER_IMPORTANCE are global and are refused there with ST_ERR_UNSUPPORTED before any rank
 * uploads.  (The st_set_devices group of the one-call forms runs the actions on one device before
 * the rows are sharded: every kind works.)
 *
 * The stand-alone calls take a device table of n < 2^32 rows (ST_ERR_UNSUPPORTED above), columns
 * aligned to their types, work on the context stream and wait for it:
 *   st_dev_importance        dev_scores[i] = row i's score (n doubles)
 *   st_dev_importance_order  dev_order[j] = the row of rank j (n uint32)
 *   st_dev_importance_top    the rows of rank < min(m, n), ascending, into dev_rows (capacity
 *                            min(m, n) uint32); *out_m = their count.  The key of rank m - 1 is found
 *                            by a radix select over the keys (8-bit digits from the top, LDS block
 *                            histograms merged with integer atomics, digits picked on the device,
 *                            the rounds queued without a host round trip); rows above it are kept,
 *                            rows equal to it in row order until m are.  All integer: the result
 *                            does not depend on the launch shape. */
int st_dev_importance(st_ctx *ctx, const st_ttable *dev_table, double *dev_scores);
int st_dev_importance_order(st_ctx *ctx, const st_ttable *dev_table, uint32_t *dev_order);
int st_dev_importance_top(st_ctx *ctx, const st_ttable *dev_table, uint64_t m, uint32_t *dev_rows, uint64_t *out_m);

/* ---- neighbour distances and outliers ---------------------------------------------------------------
 * Cleaning a scene: trained Gaussian scenes carry "floaters", isolated rows far from any surface, that
 * stretch the extents every writer quantises over.  The reference at this version has no such
 * command, so the rules are this project's own, in the style of the two sections above: a result
 * depends only on the data -- not on the order of the rows, the shape of a launch or the search
 * structure -- and is checked bit for bit.  csrc/st_neighbors.h holds every rule as a host/device
 * function and a plain serial host form.
 *
 * Every value is the column's element as a JS number (any st_ply_type, widened exactly); all
 * arithmetic is IEEE double, each operation rounds once in the order written, nothing is fused.
 *   placed     row i is placed iff its x, y and z are all finite.  A table without an x, y or z column
 *              is ST_ERR_ARG (the message names the column); nothing is launched.
 *   d2(i, j)   for placed i != j: dx = x_i - x_j, dy, dz alike; d2 = (dx*dx + dy*dy) + dz*dz.  It may
 *              be +Infinity and is never NaN.  Rows that coincide are still distinct rows: only j = i
 *              is excluded.
 *   dist_k(i)  i not placed: NaN, the one quiet NaN 0x7ff8000000000000.  Fewer than k other rows
 *              placed: +Infinity.  Otherwise sqrt of the k-th smallest element, with multiplicity, of
 *              the multiset { d2(i, j) : j placed, j != i }.  A property of a multiset: no tie rule
 *              is needed, and any correct search gives the same bits.
 *   k          an integer in 1..32; anything else is ST_ERR_ARG before any launch.
 *   ST_ACTION_FILTER_OUTLIERS (filterOutliers)   neighbors = k; keep iff dist_k(i) <= t.
 *              outlier_mode ST_OUTLIER_SIGMA: t = mean + outlier_value * std_dev, one multiplication
 *              and one addition, mean and std_dev those of the column summary over the finite dist_k
 *              values of the table as it is at that point of the chain; outlier_value may be any
 *              double but NaN (ST_ERR_ARG).  ST_OUTLIER_DISTANCE: t = outlier_value; NaN is
 *              ST_ERR_ARG.  Another mode is ST_ERR_ARG.  Rows that are not placed go; rows with a
 *              dist_k of +Infinity go unless t is +Infinity; with no finite dist_k the sigma mode has
 *              t = NaN and keeps nothing.  A stable selection through permuteRows, like the filters;
 *              all rows kept: the table stays as it is; n = 0 does nothing.
 * The action is global: st_group_sog_bundle_process refuses it with ST_ERR_UNSUPPORTED before any
 * rank uploads, as it does ST_ACTION_DECIMATE.  (The st_set_devices group of the one-call forms runs
 * the actions on one device first: it works there.)
 *
 * st_dev_neighbor_dist: dev_dist[i] = dist_k(i) for a device table of n < 2^32 rows
 * (ST_ERR_UNSUPPORTED above), columns aligned to their types; it works on the context stream and
 * waits for it.  The search: the placed rows sorted by a 30-bit Morton key of their own (locality
 * only: no result depends on it), leaves of L consecutive sorted rows with exact boxes, an implicit
 * 8-ary tree of boxes above them; one wave takes a leaf as its queries and prunes a node when, for
 * every one of them, a lower bound of d2 -- computed with d2's own operations in d2's order, so that
 * IEEE rounding's monotonicity makes it a bound on the COMPUTED d2 and no tolerance exists anywhere --
 * is >= that query's k-th best so far.  ST_KNN_LEAF=<4..64>, read per call, sets L (default 64; an invalid value falls
 * back to it).
 * st_ctx_last_neighbor_stats: the last call's JSON -- {"rows", "placed", "leaves", "levels" (box
 * levels, leaves to root), "pairs" (d2 evaluations), "nodes" (box tests)}. */
int st_dev_neighbor_dist(st_ctx *ctx, const st_ttable *dev_table, int32_t k, double *dev_dist);
const char *st_ctx_last_neighbor_stats(st_ctx *ctx);

/* ---- clusters -----------------------------------------------------------------------------------------
 * Cleaning a scene, second tool: floaters rarely come alone, and a clump of them has an ordinary
 * dist_k, because every member's neighbours are inside the clump.  Connectivity finds it: link every
 * two rows closer than a radius, keep the connected components that are large, or only the largest.
 * The reference has no such command (its kd-tree answers nearest-one queries only), so the rules are
 * this project's own, in the style of the two sections above: a result depends only on the data --
 * not on the order of the rows, the shape of a launch, the search tree or the order in which atomics
 * arrive -- and is checked bit for bit against a brute-force serial form.  csrc/st_clusters.h holds
 * every rule as a host/device function and that serial form.
 *
 * Every value is the column's element as a JS number (any st_ply_type, widened exactly); all
 * arithmetic is IEEE double, each operation rounds once in the order written, nothing is fused.
 *   placed, d2  those of "neighbour distances and outliers", unchanged.  A table without an x, y or z
 *              column is ST_ERR_ARG (the message names the column); nothing is launched.
 *   radius     any double >= 0, +Infinity included; NaN or a negative value is ST_ERR_ARG before any
 *              launch.  r2 = radius * radius, one multiplication; it may be +Infinity.
 *   link(i, j) iff i != j, both rows are placed and d2(i, j) <= r2.  Inclusive: a pair at exactly the
 *              radius links.  Symmetric bit for bit: x_i - x_j and x_j - x_i are exact negations, so
 *              their squares are equal.  r2 = +Infinity links every two placed rows, pairs whose d2
 *              overflowed included; radius = 0 links exactly the rows that coincide.
 *   component  the connected components of the link graph over the placed rows.  label(i) is the
 *              smallest row index in row i's component, 0xFFFFFFFF for a row that is not placed;
 *              size(i) is the number of rows of the component, 0 for a row that is not placed.  The
 *              partition is a property of the data; the labels additionally depend on the numbering
 *              of the rows, by definition.
 *   ST_ACTION_FILTER_CLUSTERS (filterClusters)   cluster_radius = radius.  cluster_mode
 *              ST_CLUSTER_MIN_SIZE keeps row i iff it is placed and size(i) >= cluster_min;
 *              cluster_min must be a finite, non-negative, integer-valued double below 2^53, as
 *              decimate's count (ST_ERR_ARG otherwise).  ST_CLUSTER_LARGEST keeps every row whose
 *              component has the maximal size; several components may tie for it and all of them are
 *              kept, so the kept set never depends on the numbering of the rows (cluster_min is not
 *              read).  Another mode is ST_ERR_ARG.  Rows that are not placed go.  A stable selection
 *              through permuteRows, like the filters; all rows kept: the table stays as it is; n = 0
 *              does nothing; no placed row: nothing is kept.
 * The action is global: st_group_sog_bundle_process refuses it with ST_ERR_UNSUPPORTED before any
 * rank uploads, as it does ST_ACTION_FILTER_OUTLIERS.  (The st_set_devices group of the one-call forms
 * runs the actions on one device first: it works there.)
 *
 * st_dev_clusters: dev_label[i] = label(i) and dev_size[i] = size(i) for a device table of n < 2^32
 * rows (ST_ERR_UNSUPPORTED above), columns aligned to their types, the outputs to 4 bytes; either
 * output may be NULL.  It works on the context stream and waits for it.  The search runs over the
 * tree of st_dev_neighbor_dist (ST_KNN_LEAF sets L for both): one wave takes a leaf as its queries,
 * prunes a node when the lower bound of d2 is > r2 for every one of them, and takes a whole node at
 * once, without one d2, where the node is a clique (the upper bound of d2 between two rows of its
 * own box is <= r2) and the upper bound of d2 between the query and its box is <= r2 -- both bounds
 * computed with d2's own operations in d2's order, so that no tolerance exists anywhere.  Linked rows
 * are joined in a lock-free union-find that hooks the larger root under the smaller.
 * st_ctx_last_cluster_stats: the last call's JSON -- {"rows", "placed", "components", "largest",
 * "leaves", "levels" (box levels, leaves to root), "pairs" (d2 evaluations), "nodes" (box tests),
 * "unions" (successful hooks)}. */
int st_dev_clusters(st_ctx *ctx, const st_ttable *dev_table, double radius, uint32_t *dev_label, uint32_t *dev_size);
const char *st_ctx_last_cluster_stats(st_ctx *ctx);

/* ---- st_dev_probe: a test hook ----------------------------------------------------------------
 * The two layers under every bit-exact result, called directly so that tests can compare them
 * with a reference on inputs of their own choosing: the scalar rules of csrc/st_jsmath.h as
 * compiled for the device, and the primitives of csrc/st_prims.hip.  No production path calls it
 * and it adds no kernel to one; the Node addon does not bind it.
 *
 * Every pointer in st_probe_args is a device pointer (cols: a host array of device pointers).  The
 * call works on the context stream and waits for it.  Before any launch it answers ST_ERR_ARG for:
 * an unknown op; n >= 2^32; a pointer the op needs that is NULL while n > 0, or that is not aligned
 * to its element type; a bit range outside 0 <= begin_bit <= end_bit <= the key width; ncols
 * outside 1 .. 64.  Its workspace slots are "probe.*".
 *
 * Scalar ops, elementwise over n elements (csrc/st_probe_ops.h holds the expression of each; the
 * kernel and tests/native/jsmath_cpu_check.cpp both evaluate that one text).  in0 (and in1 for the
 * two-input ops): float64.  out0: float64, except F32_STORE and F32_CAST (float32), TO_INT32
 * (int32) and TO_UINT8 (uint8).
 *   EXP, LOG, SIGMOID, LOG_TRANSFORM   js::exp, js::log, js::sigmoid, js::log_transform
 *   LOG1ABS                            js::log(|v| + 1)
 *   LOGEXP                             js::log(js::x86_nan(js::exp(v) * s, v != v || s != s)): the
 *                                      scale column of transform(), s = args.s
 *   SQRT, ROUND                        __builtin_sqrt(v), floor(v + 0.5)
 *   TO_INT32, TO_UINT8, F32_STORE      js::to_int32, js::to_uint8, js::f32_store
 *   F32_CAST, SIGN                     (float)v, js::sign_
 *   DIV, MIN, MAX                      in0 / in1, js::min_, js::max_
 *
 * Primitive ops: thin calls of the internal functions with the caller's buffers (keys and values
 * uint32, ST_PROBE_SORT_U64's keys uint64; bits [begin_bit, end_bit) of a key are sorted on).
 *   SCAN            scan_u32: exclusive scan of in0[0..n) into out0 (may be in0); aux (nullable)
 *                   receives the total and may be out0 + n
 *   SORT_U32        radix_sort_u32: out0 (keys) and out1 (values) in place
 *   SORT_FROM       radix_sort_u32_from: keys in0 (left unchanged), values in1 (NULL: the identity)
 *                   into out0 / out1, without the fused first histogram.  out0 == in0 or
 *                   out1 == in1 needs an even pass count: ST_ERR_INTERNAL, nothing written
 *   SORT_IOTA       radix_sort_u32_iota: in0 -> out0 / out1
 *   SORT_SWAP       radix_sort_u32_inplace_or_swap on the pair in0 / in1 (overwritten); the pair
 *                   its returned pointers name is copied to out0 / out1; result = 1 when that pair
 *                   was in0 / in1, 0 when it was the workspace's
 *   SORT_U64        radix_sort_u64: out0 (uint64 keys) and out1 in place
 *   MINMAX          minmax_keys_dev over the ncols float columns cols[0..ncols) of n elements:
 *                   out0[2a] = min, out0[2a + 1] = max of column a as order-preserving keys
 *   IOTA            iota_u32: out0[i] = i */
#define ST_PROBE_EXP 1
#define ST_PROBE_LOG 2
#define ST_PROBE_SIGMOID 3
#define ST_PROBE_LOG_TRANSFORM 4
#define ST_PROBE_LOG1ABS 5
#define ST_PROBE_LOGEXP 6
#define ST_PROBE_SQRT 7
#define ST_PROBE_ROUND 8
#define ST_PROBE_TO_INT32 9
#define ST_PROBE_TO_UINT8 10
#define ST_PROBE_F32_STORE 11
#define ST_PROBE_F32_CAST 12
#define ST_PROBE_SIGN 13
#define ST_PROBE_DIV 14
#define ST_PROBE_MIN 15
#define ST_PROBE_MAX 16
#define ST_PROBE_SCAN 32
#define ST_PROBE_SORT_U32 33
#define ST_PROBE_SORT_FROM 34
#define ST_PROBE_SORT_IOTA 35
#define ST_PROBE_SORT_SWAP 36
#define ST_PROBE_SORT_U64 37
#define ST_PROBE_MINMAX 38
#define ST_PROBE_IOTA 39
typedef struct st_probe_args {
    void *in0, *in1;
    void *out0, *out1;
    void *aux;
    const float *const *cols;
    uint64_t n;
    double s;
    int32_t begin_bit, end_bit, ncols;
    int32_t result; /* written by ST_PROBE_SORT_SWAP */
} st_probe_args;
int st_dev_probe(st_ctx *ctx, int32_t op, st_probe_args *args);

#ifdef __cplusplus
}
#endif
#endif /* ST_ABI_H */
