"""ctypes binding of libsplat_hip.so (the C-ABI in include/st_abi.h).

Used by the tests, bench.py and __graft_entry__.  Host-array entry points take
numpy arrays; ``dev_*`` entry points take torch CUDA (HIP) tensors and pass
their device pointers, running on torch's current stream.  There is no CPU
fallback: constructing a Context without a gfx950 device raises.
"""
import collections
import contextlib
import ctypes
import weakref
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
# ST_LIB overrides the library path (kernel-variant experiments under tools/)
LIB_PATH = os.environ.get('ST_LIB') or os.path.join(PKG, 'lib', 'libsplat_hip.so')

ST_OK = 0
ST_ERR_ARG, ST_ERR_HIP, ST_ERR_NONFINITE, ST_ERR_DRAWS = -1, -2, -3, -4
ST_ERR_UNSUPPORTED = -6
_lib = None


class StError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'st error {code}: {msg}')
        self.code = code


class Table(ctypes.Structure):
    _fields_ = [('n', ctypes.c_uint64), ('ncol', ctypes.c_int32),
                ('names', ctypes.POINTER(ctypes.c_char_p)), ('cols', ctypes.POINTER(ctypes.c_void_p))]


class TTable(ctypes.Structure):
    _fields_ = [('n', ctypes.c_uint64), ('ncol', ctypes.c_int32), ('names', ctypes.POINTER(ctypes.c_char_p)),
                ('types', ctypes.POINTER(ctypes.c_int32)), ('cols', ctypes.POINTER(ctypes.c_void_p))]


class TransformParams(ctypes.Structure):
    _fields_ = [('m4', ctypes.c_float * 16), ('r', ctypes.c_double * 4), ('s', ctypes.c_double),
                ('sh1', ctypes.c_double * 9), ('sh2', ctypes.c_double * 25), ('sh3', ctypes.c_double * 49)]


class SogMeta(ctypes.Structure):
    _fields_ = [('width', ctypes.c_int32), ('height', ctypes.c_int32),
                ('means_min', ctypes.c_double * 3), ('means_max', ctypes.c_double * 3),
                ('scales_codebook', ctypes.c_float * 256), ('sh0_codebook', ctypes.c_float * 256),
                ('sh_bands', ctypes.c_int32), ('palette_size', ctypes.c_int32),
                ('shn_codebook', ctypes.c_float * 256), ('shn_width', ctypes.c_int32), ('shn_height', ctypes.c_int32)]


class SogTextures(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in
                ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shn_centroids', 'shn_labels')]


class Action(ctypes.Structure):
    _fields_ = [('kind', ctypes.c_int32), ('compare', ctypes.c_int32), ('column', ctypes.c_char_p),
                ('value', ctypes.c_double), ('bands', ctypes.c_int32), ('transform', TransformParams),
                ('box_min', ctypes.c_double * 3), ('box_max', ctypes.c_double * 3), ('center', ctypes.c_double * 3),
                ('radius', ctypes.c_double), ('amount', ctypes.c_double), ('amount_mode', ctypes.c_int32),
                ('neighbors', ctypes.c_int32), ('outlier_mode', ctypes.c_int32), ('outlier_value', ctypes.c_double),
                ('cluster_radius', ctypes.c_double), ('cluster_mode', ctypes.c_int32), ('cluster_min', ctypes.c_double)]


ACTION_TRANSFORM, ACTION_FILTER_NAN, ACTION_FILTER_VALUE, ACTION_FILTER_BANDS, ACTION_PARAM = 1, 2, 3, 4, 5
ACTION_ORDER_IMPORTANCE, ACTION_DECIMATE, ACTION_FILTER_BOX, ACTION_FILTER_SPHERE = 6, 7, 8, 9
ACTION_FILTER_OUTLIERS = 10
ACTION_FILTER_CLUSTERS = 11
DECIMATE_COUNT, DECIMATE_FRACTION = 0, 1
OUTLIER_SIGMA, OUTLIER_DISTANCE = 0, 1
CLUSTER_MIN_SIZE, CLUSTER_LARGEST = 0, 1
COMPARE = {'lt': 0, 'lte': 1, 'gt': 2, 'gte': 3, 'eq': 4, 'neq': 5}


PLY_TYPES = {1: ('char', np.int8), 2: ('uchar', np.uint8), 3: ('short', np.int16), 4: ('ushort', np.uint16),
             5: ('int', np.int32), 6: ('uint', np.uint32), 7: ('float', np.float32), 8: ('double', np.float64)}


class PlyProperty(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 64), ('type', ctypes.c_int32)]


class PlyElement(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char * 64), ('count', ctypes.c_uint64), ('nprops', ctypes.c_int32),
                ('props', PlyProperty * 256)]


class PlyHeader(ctypes.Structure):
    _fields_ = [('header_bytes', ctypes.c_uint64), ('nelements', ctypes.c_int32), ('ncomments', ctypes.c_int32),
                ('comments', ctypes.c_char * 8192), ('elements', PlyElement * 16)]

    def layout(self):
        """[(element name, count, [(prop name, numpy dtype)])]"""
        out = []
        for e in self.elements[:self.nelements]:
            out.append((e.name.decode(), e.count,
                        [(p.name.decode(), PLY_TYPES[p.type][1]) for p in e.props[:e.nprops]]))
        return out

    def comment_list(self):
        return self.comments.decode().split('\n') if self.ncomments else []


EXPORTS = [
    'st_abi_version', 'st_last_error', 'st_device_count', 'st_ctx_create', 'st_ctx_destroy', 'st_ctx_set_stream',
    'st_ctx_synchronize', 'st_ctx_last_timings', 'st_ctx_last_kmeans_stats', 'st_ctx_set_profiling', 'st_ctx_reset_kernel_stats',
    'st_ctx_kernel_stats', 'st_ctx_set_verify', 'st_ctx_verify_snapshot', 'st_quat_from_euler', 'st_transform_params_make', 'st_sog_geometry',
    'st_transform', 'st_filter_finite', 'st_morton_order', 'st_pack_compressed', 'st_kmeans', 'st_cluster1d', 'st_sog',
    'st_dev_transform', 'st_dev_filter_finite', 'st_dev_permute_rows', 'st_dev_concat_rows', 'st_dev_morton_order',
    'st_dev_pack_compressed', 'st_dev_kmeans', 'st_dev_cluster1d', 'st_dev_sog',
    'st_set_devices', 'st_get_devices', 'st_comm_unique_id', 'st_comm_init_rank', 'st_comm_init_host', 'st_comm_destroy',
    'st_comm_count', 'st_rccl_info', 'st_ctx_last_host_reuse', 'st_ply_compressed_ply_file',
    'st_compressed_ply_file',
    'st_dev_sog_sharded', 'st_group_create', 'st_group_destroy', 'st_group_sog', 'st_group_sog_bundle',
    'st_filter_nan', 'st_dev_filter_finite_t', 'st_dev_permute_rows_t', 'st_combine_layout', 'st_dev_combine',
    'st_dev_minmax', 'st_dev_kmeans_init_rows', 'st_dev_gather_rows', 'st_dev_kmeans_prepare',
    'st_dev_kmeans_assign', 'st_dev_kmeans_partials',
    'st_dev_kmeans_seqsum', 'st_dev_kmeans_finish', 'st_dev_kmeans_average', 'st_dev_cluster1d_codebook',
    'st_dev_sog_scatter', 'st_dev_sog_shn_centroids',
    'st_webp_max_size', 'st_dev_webp_lossless', 'st_webp_lossless', 'st_dev_crc32', 'st_zip_store',
    'st_sog_meta_json', 'st_dev_sog_bundle', 'st_dev_sog_bundle_view', 'st_dev_sog_file', 'st_sog_file', 'st_sog_bundle',
    'st_free',
    'st_ply_parse_header', 'st_ply_read_header', 'st_ply_row_bytes', 'st_dev_ply_transpose', 'st_dev_ply_read',
    'st_ply_read', 'st_ply_read_resident', 'st_ply_materialize', 'st_ply_forget', 'st_dev_decompress_ply', 'st_decompress_ply',
    'st_process', 'st_compressed_ply', 'st_dev_compressed_ply', 'st_ply_compressed_ply', 'st_ply_sog_bundle',
    'st_group_sog_bundle_process',
    'st_transform_t', 'st_dev_transform_t', 'st_morton_order_t', 'st_dev_morton_order_t', 'st_sog_process',
    'st_sog_bundle_process', 'st_dev_sog_t',
    'st_splat_layout', 'st_ksplat_layout', 'st_spz_layout', 'st_dev_splat_decode', 'st_dev_ksplat_decode',
    'st_dev_spz_decode', 'st_splat_read', 'st_dev_splat_read', 'st_ksplat_read', 'st_dev_ksplat_read', 'st_spz_read',
    'st_dev_spz_read',
    'st_ply_header_text', 'st_ply_element_text', 'st_dev_ply_rows', 'st_dev_ply_rows_file', 'st_ply_rows_file',
    'st_ply_file', 'st_ply_ply_file',
    'st_csv_max_row_bytes', 'st_csv_header_text', 'st_dev_csv_rows', 'st_dev_csv_file', 'st_csv_file',
    'st_ply_csv_file',
    'st_base64_size', 'st_dev_base64', 'st_html_parts', 'st_html_file', 'st_ply_html_file',
    'st_zip_index', 'st_webp_info', 'st_webp_decode_lossless', 'st_sog_read_layout', 'st_dev_sog_decode', 'st_sog_read',
    'st_dev_sog_read',
    'st_spz_image_size', 'st_dev_splat_rows', 'st_dev_spz_planes', 'st_dev_spz_image', 'st_dev_splat_file',
    'st_splat_file', 'st_ply_splat_file', 'st_dev_spz_file', 'st_spz_file', 'st_ply_spz_file',
    'st_ksplat_image_size', 'st_dev_ksplat_plan', 'st_dev_ksplat_records', 'st_dev_ksplat_image', 'st_dev_ksplat_file',
    'st_ksplat_file', 'st_ply_ksplat_file',
    'st_deflate_bound', 'st_gzip_bound', 'st_dev_deflate', 'st_dev_gzip', 'st_dev_spz_gz_file', 'st_spz_gz_file',
    'st_ply_spz_gz_file',
    'st_gzip_member_layout', 'st_inflate_head', 'st_dev_inflate', 'st_dev_gunzip', 'st_spz_gz_layout', 'st_spz_gz_read',
    'st_dev_spz_gz_read',
    'st_dev_summary', 'st_summary', 'st_summary_text', 'st_ctx_last_summary_stats',
    'st_dev_importance', 'st_dev_importance_order', 'st_dev_importance_top',
    'st_dev_neighbor_dist', 'st_ctx_last_neighbor_stats',
    'st_dev_clusters', 'st_ctx_last_cluster_stats',
    'st_dev_probe',
]


def _forget_column(ctx_ref, ptr):
    """a resident read's column is being freed: the context (if still open) drops it (st_ply_forget)"""
    c = ctx_ref()
    if c is not None and c.h:
        lib().st_ply_forget(c.h, ctypes.c_void_p(ptr))


def build(jobs=8):
    subprocess.check_call(['make', '-s', '-C', PKG, f'-j{jobs}'])


def lib():
    """Load libsplat_hip.so (fails loudly if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} missing: build it with `make -C {PKG}` (hipcc, gfx950)')
        L = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(L, name)
        L.st_last_error.restype = ctypes.c_char_p
        L.st_ctx_last_timings.restype = ctypes.c_char_p
        L.st_ctx_last_kmeans_stats.restype = ctypes.c_char_p
        L.st_ctx_last_summary_stats.restype = ctypes.c_char_p
        L.st_ctx_last_neighbor_stats.restype = ctypes.c_char_p
        L.st_ctx_last_cluster_stats.restype = ctypes.c_char_p
        L.st_ctx_destroy.restype = None
        L.st_comm_destroy.restype = None
        L.st_group_destroy.restype = None
        L.st_free.restype = None
        L.st_webp_max_size.restype = ctypes.c_uint64
        L.st_ply_row_bytes.restype = ctypes.c_uint64
        L.st_csv_max_row_bytes.restype = ctypes.c_uint64
        L.st_base64_size.restype = ctypes.c_uint64
        L.st_base64_size.argtypes = [ctypes.c_uint64]
        L.st_spz_image_size.restype = ctypes.c_uint64
        L.st_spz_image_size.argtypes = [ctypes.c_uint64, ctypes.c_int32]
        L.st_ksplat_image_size.restype = ctypes.c_uint64
        L.st_ksplat_image_size.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64]
        for name in ('st_deflate_bound', 'st_gzip_bound'):
            getattr(L, name).restype = ctypes.c_uint64
            getattr(L, name).argtypes = [ctypes.c_uint64]
        for name in EXPORTS:
            if name not in ('st_last_error', 'st_ctx_last_timings', 'st_ctx_last_kmeans_stats',
                            'st_ctx_last_summary_stats', 'st_ctx_last_neighbor_stats', 'st_ctx_last_cluster_stats', 'st_ctx_destroy', 'st_free', 'st_webp_max_size',
                            'st_ply_row_bytes', 'st_csv_max_row_bytes', 'st_base64_size', 'st_comm_destroy',
                            'st_group_destroy', 'st_spz_image_size', 'st_ksplat_image_size', 'st_deflate_bound',
                            'st_gzip_bound'):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
    return _lib


def check(rc):
    if rc != ST_OK:
        raise StError(rc, lib().st_last_error().decode())


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _ptr(t):
    """device pointer of a torch tensor or numpy host array"""
    if t is None:
        return None
    if hasattr(t, 'data_ptr'):
        return ctypes.c_void_p(t.data_ptr())
    return ctypes.c_void_p(t.ctypes.data)


def make_table(cols):
    """st_table over a dict name -> float32 array (numpy host or torch device); keeps refs alive"""
    names = list(cols.keys())
    n = len(cols[names[0]]) if names else 0
    c_names = (ctypes.c_char_p * len(names))(*[s.encode() for s in names])
    c_cols = (ctypes.c_void_p * len(names))(*[_ptr(cols[k]).value for k in names])
    t = Table(n, len(names), ctypes.cast(c_names, ctypes.POINTER(ctypes.c_char_p)),
              ctypes.cast(c_cols, ctypes.POINTER(ctypes.c_void_p)))
    t._keep = (c_names, c_cols, cols)
    return t


_NP_TO_PLY = {np.dtype(v[1]): k for k, v in PLY_TYPES.items()}


def ply_type_of(a):
    """st_ply_type code of a numpy array or torch tensor's element type"""
    if hasattr(a, 'data_ptr'):
        import torch
        tmap = {torch.int8: 1, torch.uint8: 2, torch.int16: 3, torch.uint16: 4, torch.int32: 5, torch.uint32: 6,
                torch.float32: 7, torch.float64: 8}
        return tmap[a.dtype]
    return _NP_TO_PLY[np.dtype(a.dtype)]


def _torch_type(dtype):
    import torch
    return {np.dtype(n): t for n, t in (
        (np.int8, torch.int8), (np.uint8, torch.uint8), (np.int16, torch.int16), (np.uint16, torch.uint16),
        (np.int32, torch.int32), (np.uint32, torch.uint32), (np.float32, torch.float32),
        (np.float64, torch.float64))}[np.dtype(dtype)]


def make_ttable(cols, n=None):
    """st_ttable over a list of (name, array) or a dict (numpy host or torch device, any of the eight
    types); keeps refs alive"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    names = [k for k, _ in items]
    if n is None:
        n = len(items[0][1]) if items else 0
    c_names = (ctypes.c_char_p * len(items))(*[k.encode() for k in names])
    c_types = (ctypes.c_int32 * len(items))(*[ply_type_of(a) for _, a in items])
    c_cols = (ctypes.c_void_p * len(items))(*[_ptr(a).value for _, a in items])
    t = TTable(n, len(items), ctypes.cast(c_names, ctypes.POINTER(ctypes.c_char_p)),
               ctypes.cast(c_types, ctypes.POINTER(ctypes.c_int32)), ctypes.cast(c_cols, ctypes.POINTER(ctypes.c_void_p)))
    t._keep = (c_names, c_types, c_cols, items)
    return t


def combine_layout(tables):
    """combine()'s result columns (index.ts:164-178): [(table index, column index)]; tables are lists
    of (name, array)"""
    tts = [make_ttable(t) for t in tables]
    arr = (ctypes.POINTER(TTable) * len(tts))(*[ctypes.pointer(t) for t in tts])
    ncol = ctypes.c_int32()
    check(lib().st_combine_layout(arr, ctypes.c_int32(len(tts)), None, None, ctypes.byref(ncol)))
    ct = (ctypes.c_int32 * max(ncol.value, 1))()
    ci = (ctypes.c_int32 * max(ncol.value, 1))()
    check(lib().st_combine_layout(arr, ctypes.c_int32(len(tts)), ct, ci, ctypes.byref(ncol)))
    return [(ct[i], ci[i]) for i in range(ncol.value)]


def set_devices(n):
    """st_set_devices: st_sog / st_sog_bundle shard their rows over GPUs 0..n-1 (RCCL)"""
    check(lib().st_set_devices(ctypes.c_int32(n)))


def get_devices():
    n = ctypes.c_int32()
    check(lib().st_get_devices(ctypes.byref(n)))
    return n.value


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it; the launcher hands it to every rank)"""
    buf = (ctypes.c_uint8 * 128)()
    check(lib().st_comm_unique_id(buf))
    return bytes(buf)


def _tables_arg(tables):
    ts = [make_table(t) for t in tables]
    arr = (ctypes.POINTER(Table) * len(ts))(*[ctypes.pointer(t) for t in ts])
    return ts, arr


def _sog_out(N, C, host=True, device=None):
    W, H, pal, cw, ch = sog_geometry(N, C)
    names = ['means_l', 'means_u', 'quats', 'scales', 'sh0'] + (['shN_labels'] if C else [])
    if host:
        tex = {k: np.zeros(W * H * 4, np.uint8) for k in names}
        if C:
            tex['shN_centroids'] = np.zeros(cw * ch * 4, np.uint8)
    else:
        import torch
        tex = {k: torch.empty(W * H * 4, dtype=torch.uint8, device=device) for k in names}
        if C:
            tex['shN_centroids'] = torch.empty(cw * ch * 4, dtype=torch.uint8, device=device)
    out = SogTextures(*[(_ptr(tex[k]).value if k in tex else None) for k in
                        ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
    return tex, out, (W, H, cw, ch)


def _union_coeffs(tables):
    names = set()
    for t in tables:
        names.update(t.keys())
    miss = next((i for i in range(45) if f'f_rest_{i}' not in names), -1)
    return [0, 3, 8, 15][{9: 1, 24: 2, -1: 3}.get(miss, 0)]


class Group:
    """st_group: several ranks in this process (one context + host thread each).  host_staged: the
    exchange goes through host memory, so ranks may share a GPU (the multi-rank tests)"""

    def __init__(self, devices, host_staged=False):
        self.h = ctypes.c_void_p()
        arr = (ctypes.c_int32 * len(devices))(*devices)
        check(lib().st_group_create(arr, ctypes.c_int32(len(devices)), ctypes.c_int32(1 if host_staged else 0),
                                    ctypes.byref(self.h)))
        self.world = len(devices)

    def close(self):
        if self.h:
            lib().st_group_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sog(self, tables, iters, draws, splits=None):
        """writeSog of the concatenated host tables (dicts name -> float32 array)"""
        N = sum(len(next(iter(t.values()))) for t in tables)
        C = _union_coeffs(tables)
        tex, out, (W, H, cw, ch) = _sog_out(N, C)
        ts, arr = _tables_arg(tables)
        sp = (ctypes.c_uint64 * (self.world + 1))(*splits) if splits is not None else None
        meta = SogMeta()
        used = ctypes.c_uint64()
        check(lib().st_group_sog(self.h, arr, ctypes.c_int32(len(ts)), sp, ctypes.c_int32(iters), _vp(draws),
                                 ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.byref(meta),
                                 ctypes.byref(out)))
        res = {k: v.reshape(H, W, 4) for k, v in tex.items() if k != 'shN_centroids'}
        if C:
            res['shN_centroids'] = tex['shN_centroids'].reshape(ch, cw, 4)
        return res, meta, used.value

    def sog_bundle(self, tables, iters, draws, dos_time, dos_date, splits=None):
        ts, arr = _tables_arg(tables)
        sp = (ctypes.c_uint64 * (self.world + 1))(*splits) if splits is not None else None
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        used = ctypes.c_uint64()
        check(lib().st_group_sog_bundle(self.h, arr, ctypes.c_int32(len(ts)), sp, ctypes.c_int32(iters),
                                        _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used),
                                        ctypes.c_uint16(dos_time), ctypes.c_uint16(dos_date), ctypes.byref(out),
                                        ctypes.byref(size)))
        return _take(out, size), used.value


    def sog_bundle_process(self, tables, actions, iters, draws, dos_time, dos_date, splits=None):
        """writeSog -> .sog bytes of the combine of `tables` after each table's processDataTable
        `actions` (one list per table) ran on the ranks' parts (st_group_sog_bundle_process)"""
        ts, arr = _tables_arg(tables)
        acts = [make_actions(a) for a in actions]
        aptr = (ctypes.POINTER(Action) * len(ts))(*[ctypes.cast(a, ctypes.POINTER(Action)) for a in acts])
        nact = (ctypes.c_int32 * len(ts))(*[len(a) for a in actions])
        sp = (ctypes.c_uint64 * (self.world + 1))(*splits) if splits is not None else None
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        used = ctypes.c_uint64()
        check(lib().st_group_sog_bundle_process(self.h, arr, ctypes.c_int32(len(ts)), sp, aptr, nact,
                                                ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)),
                                                ctypes.byref(used), ctypes.c_uint16(dos_time),
                                                ctypes.c_uint16(dos_date), ctypes.byref(out), ctypes.byref(size)))
        return _take(out, size), used.value


class Comm:
    """st_comm: this process's rank of a one-rank-per-process job: over RCCL (one GPU per rank,
    `uid` from comm_unique_id on rank 0) or, with Comm.host, over host shared memory (any number
    of ranks on one GPU)"""

    def __init__(self, ctx, world, rank, uid=None, _host=None):
        self.h = ctypes.c_void_p()
        self.world, self.rank = world, rank
        if _host is not None:
            name, slot_bytes, timeout_s = _host
            check(lib().st_comm_init_host(ctx.h, ctypes.c_int32(world), ctypes.c_int32(rank), name.encode(),
                                          ctypes.c_uint64(slot_bytes), ctypes.c_double(timeout_s),
                                          ctypes.byref(self.h)))
            self.transport = 'host-shm'
            return
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(lib().st_comm_init_rank(ctx.h, ctypes.c_int32(world), ctypes.c_int32(rank), buf, ctypes.byref(self.h)))
        self.transport = 'rccl'

    @classmethod
    def host(cls, ctx, world, rank, name, slot_bytes=0, timeout_s=600.0):
        """st_comm_init_host: every rank passes the same job `name` (unique per job)"""
        return cls(ctx, world, rank, _host=(name, slot_bytes, timeout_s))

    def count(self):
        """ranks in the communicator (ncclCommCount for RCCL)"""
        n = ctypes.c_int32()
        check(lib().st_comm_count(self.h, ctypes.byref(n)))
        return n.value

    def close(self):
        if self.h:
            lib().st_comm_destroy(self.h)
            self.h = ctypes.c_void_p()


def quat_from_euler(ex, ey, ez):
    q = (ctypes.c_double * 4)()
    check(lib().st_quat_from_euler(ctypes.c_double(ex), ctypes.c_double(ey), ctypes.c_double(ez), q))
    return np.array(q[:])


def transform_params(t=(0.0, 0.0, 0.0), r=(0.0, 0.0, 0.0, 1.0), s=1.0):
    p = TransformParams()
    check(lib().st_transform_params_make((ctypes.c_double * 3)(*t), (ctypes.c_double * 4)(*r), ctypes.c_double(s),
                                         ctypes.byref(p)))
    return p


def action_params(kind, value):
    """process.ts:71-83: translate / rotate (Euler degrees) / scale"""
    if kind == 'translate':
        return transform_params(t=value)
    if kind == 'rotate':
        return transform_params(r=quat_from_euler(*value))
    if kind == 'scale':
        return transform_params(s=float(value))
    raise ValueError(kind)


def make_actions(actions):
    """processDataTable's ProcessAction list (process.ts:6-42) as st_action[]: dicts with 'kind' in
    translate / rotate / scale (value as in action_params), filterNaN, filterByValue (columnName,
    comparator, value), filterBands (value), param; and this project's own (st_abi.h, "importance,
    decimation and crops"): filterBox (min, max: three numbers each), filterSphere (center, radius),
    decimate (count or fraction), orderByImportance; and ("neighbour distances and outliers")
    filterOutliers (k, default 8, and either sigma or distance); and ("clusters") filterClusters (radius,
    and either minSize or keep='largest')"""
    arr = (Action * max(1, len(actions)))()
    keep = []
    for a, act in zip(arr, actions):
        k = act['kind']
        if k in ('translate', 'rotate', 'scale'):
            a.kind, a.transform = ACTION_TRANSFORM, action_params(k, act['value'])
        elif k == 'filterNaN':
            a.kind = ACTION_FILTER_NAN
        elif k == 'filterByValue':
            col = act['columnName'].encode()
            keep.append(col)
            a.kind, a.column, a.value = ACTION_FILTER_VALUE, col, float(act['value'])
            a.compare = COMPARE.get(act['comparator'], -1)
        elif k == 'filterBands':
            a.kind, a.bands = ACTION_FILTER_BANDS, int(act['value'])
        elif k == 'param':
            a.kind = ACTION_PARAM
        elif k == 'filterBox':
            a.kind, a.box_min, a.box_max = ACTION_FILTER_BOX, _vec3(act['min']), _vec3(act['max'])
        elif k == 'filterSphere':
            a.kind, a.center, a.radius = ACTION_FILTER_SPHERE, _vec3(act['center']), float(act['radius'])
        elif k == 'decimate':
            if ('count' in act) == ('fraction' in act):
                raise ValueError('decimate takes either count or fraction')
            a.kind = ACTION_DECIMATE
            a.amount_mode = DECIMATE_COUNT if 'count' in act else DECIMATE_FRACTION
            a.amount = float(act['count'] if 'count' in act else act['fraction'])
        elif k == 'orderByImportance':
            a.kind = ACTION_ORDER_IMPORTANCE
        elif k == 'filterOutliers':
            if ('sigma' in act) == ('distance' in act):
                raise ValueError('filterOutliers takes either sigma or distance')
            kk = act.get('k', 8)
            a.kind, a.neighbors = ACTION_FILTER_OUTLIERS, (int(kk) if int(kk) == kk and abs(kk) < 2 ** 31 else 0)  # 0: refused
            a.outlier_mode = OUTLIER_SIGMA if 'sigma' in act else OUTLIER_DISTANCE
            a.outlier_value = float(act['sigma'] if 'sigma' in act else act['distance'])
        elif k == 'filterClusters':
            if 'radius' not in act or ('minSize' in act) == ('keep' in act) or act.get('keep', 'largest') != 'largest':
                raise ValueError("filterClusters takes radius and either minSize or keep='largest'")
            a.kind, a.cluster_radius = ACTION_FILTER_CLUSTERS, float(act['radius'])
            a.cluster_mode = CLUSTER_LARGEST if 'keep' in act else CLUSTER_MIN_SIZE
            a.cluster_min = float(act.get('minSize', 0))
        else:
            raise ValueError(k)
    arr._keep = keep
    return arr


def process_schema(items, actions, with_source=False):
    """the (name, dtype) columns processDataTable leaves (filterBands renames / drops f_rest
    columns against the ORIGINAL table's band, process.ts:110-134); with_source: (name, dtype,
    index of the input column it is)"""
    names = [k for k, _ in items]
    first_missing = next((i for i in range(45) if f'f_rest_{i}' not in names), -1)
    in_coeffs = {9: 3, 24: 8, -1: 15}.get(first_missing, 0)
    cols = [(k, np.dtype(a.dtype), i) for i, (k, a) in enumerate(items)]
    for act in actions:
        if act['kind'] != 'filterBands':
            continue
        out_coeffs = [0, 3, 8, 15][act['value']]
        if out_coeffs >= in_coeffs:
            continue
        mp = {}
        for i in range(in_coeffs):
            for j in range(3):
                mp[f'f_rest_{i + j * in_coeffs}'] = f'f_rest_{i + j * out_coeffs}' if i < out_coeffs else None
        cols = [(mp[k], t, i) if k in mp else (k, t, i) for k, t, i in cols if k not in mp or mp[k] is not None]
    return cols if with_source else [(k, t) for k, t, _ in cols]


TRANSFORM_KINDS = ('translate', 'rotate', 'scale')
# the kinds that copy the table (those after filterByValue are this project's own)
FILTER_KINDS = ('filterNaN', 'filterByValue', 'filterBox', 'filterSphere', 'decimate', 'orderByImportance',
                'filterOutliers', 'filterClusters')


def sog_geometry(n, sh_coeffs):
    v = [ctypes.c_int32() for _ in range(5)]
    check(lib().st_sog_geometry(ctypes.c_uint64(n), ctypes.c_int32(sh_coeffs), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _take(buf, size):
    """copy a malloc'd library buffer into bytes and release it"""
    try:
        return ctypes.string_at(buf, size.value)
    finally:
        lib().st_free(buf)


def webp_max_size(w, h):
    return lib().st_webp_max_size(ctypes.c_int32(w), ctypes.c_int32(h))


def zip_store(entries, dos_time, dos_date):
    """store-only ZIP of [(name, bytes, crc)] in the layout of serialize/zip-writer.ts (host)"""
    n = len(entries)
    names = (ctypes.c_char_p * n)(*[e[0].encode() for e in entries])
    bufs = [ctypes.create_string_buffer(bytes(e[1]), len(e[1]) or 1) for e in entries]
    data = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    sizes = (ctypes.c_uint64 * n)(*[len(e[1]) for e in entries])
    crcs = (ctypes.c_uint32 * n)(*[e[2] for e in entries])
    out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
    check(lib().st_zip_store(names, data, sizes, crcs, ctypes.c_int32(n), ctypes.c_uint16(dos_time),
                             ctypes.c_uint16(dos_date), ctypes.byref(out), ctypes.byref(size)))
    return _take(out, size)


def sog_meta_json(meta, count):
    """meta.json text of writeSog for an SogMeta (host)"""
    out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
    check(lib().st_sog_meta_json(ctypes.byref(meta), ctypes.c_uint64(count), ctypes.byref(out), ctypes.byref(size)))
    return _take(out, size)


CHUNK_COLS = ['min_x', 'min_y', 'min_z', 'max_x', 'max_y', 'max_z', 'min_scale_x', 'min_scale_y', 'min_scale_z',
              'max_scale_x', 'max_scale_y', 'max_scale_z', 'min_r', 'min_g', 'min_b', 'max_r', 'max_g', 'max_b']
VERTEX_COLS = ['packed_position', 'packed_rotation', 'packed_scale', 'packed_color']
DECOMP_COLS = ['x', 'y', 'z', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity', 'rot_0', 'rot_1', 'rot_2', 'rot_3',
               'scale_0', 'scale_1', 'scale_2']


def ply_parse_header(data):
    """readPly's header (read-ply.ts:54-137) from the first bytes of a file (host)"""
    h = PlyHeader()
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    check(lib().st_ply_parse_header(buf, ctypes.c_uint64(len(data)), ctypes.byref(h)))
    return h


def _schema_ttable(schema, n):
    """st_ttable of names and types only (st_ply_header_text reads nothing else): schema is a list of
    (name, numpy dtype or array)"""
    names = [k for k, _ in schema]
    c_names = (ctypes.c_char_p * max(len(names), 1))(*[k.encode() for k in names])
    c_types = (ctypes.c_int32 * max(len(names), 1))(
        *[ply_type_of(a) if hasattr(a, 'data_ptr') or isinstance(a, np.ndarray) else _NP_TO_PLY[np.dtype(a)]
          for _, a in schema])
    t = TTable(n, len(names), ctypes.cast(c_names, ctypes.POINTER(ctypes.c_char_p)),
               ctypes.cast(c_types, ctypes.POINTER(ctypes.c_int32)), None)
    t._keep = (c_names, c_types)
    return t


def _comments_arg(comments):
    keep = [c.encode() for c in comments]
    return (ctypes.c_char_p * max(len(keep), 1))(*keep), ctypes.c_int32(len(keep))


def ply_header_text(schema, n, element=None, comments=(), element_only=False):
    """writePly's header text (write-ply.ts:19-35) for one element of n rows: schema is a list of
    (name, numpy dtype or array); element None = 'vertex'.  element_only: the element / property
    lines alone (st_ply_element_text), for headers of several elements.  Host only -> bytes"""
    t = _schema_ttable(schema, n)
    out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
    el = element.encode() if element is not None else None
    if element_only:
        check(lib().st_ply_element_text(ctypes.byref(t), el, ctypes.byref(out), ctypes.byref(size)))
    else:
        cs, nc = _comments_arg(comments)
        check(lib().st_ply_header_text(ctypes.byref(t), el, cs, nc, ctypes.byref(out), ctypes.byref(size)))
    return _take(out, size)


def csv_header_text(cols):
    """writeCsv's header line (write-csv.ts:9-10): the column names joined by ',' and a newline, raw.
    cols: a list of (name, numpy dtype or array) or a dict.  Host only -> bytes"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    t = _schema_ttable(items, 0)
    out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
    check(lib().st_csv_header_text(ctypes.byref(t), ctypes.byref(out), ctypes.byref(size)))
    return _take(out, size)


def csv_max_row_bytes(cols):
    """the longest row of text the columns' types admit (st_csv_max_row_bytes): per column its type's
    longest cell plus one separator.  Host only"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    return lib().st_csv_max_row_bytes(ctypes.byref(_schema_ttable(items, 0)))


class ColSummaryC(ctypes.Structure):
    _fields_ = [('rows', ctypes.c_uint64), ('nan_count', ctypes.c_uint64), ('inf_count', ctypes.c_uint64),
                ('min', ctypes.c_double), ('max', ctypes.c_double), ('sum', ctypes.c_double),
                ('mean', ctypes.c_double), ('ssd', ctypes.c_double), ('std_dev', ctypes.c_double),
                ('median', ctypes.c_double)]


ColSummary = collections.namedtuple('ColSummary', [f for f, _ in ColSummaryC._fields_])


class ProbeArgs(ctypes.Structure):
    _fields_ = [('in0', ctypes.c_void_p), ('in1', ctypes.c_void_p), ('out0', ctypes.c_void_p), ('out1', ctypes.c_void_p),
                ('aux', ctypes.c_void_p), ('cols', ctypes.c_void_p), ('n', ctypes.c_uint64), ('s', ctypes.c_double),
                ('begin_bit', ctypes.c_int32), ('end_bit', ctypes.c_int32), ('ncols', ctypes.c_int32),
                ('result', ctypes.c_int32)]


# st_abi.h's ST_PROBE_* codes
PROBE_OPS = {'exp': 1, 'log': 2, 'sigmoid': 3, 'log_transform': 4, 'log1abs': 5, 'logexp': 6, 'sqrt': 7, 'round': 8,
             'to_int32': 9, 'to_uint8': 10, 'f32_store': 11, 'f32_cast': 12, 'sign': 13, 'div': 14, 'min': 15, 'max': 16,
             'scan': 32, 'sort_u32': 33, 'sort_from': 34, 'sort_iota': 35, 'sort_swap': 36, 'sort_u64': 37,
             'minmax': 38, 'iota': 39}


def _summaries_out(names, raw):
    """{name: ColSummary}, or a list in column order when a name occurs twice"""
    vals = [ColSummary(*(getattr(r, f) for f in ColSummary._fields)) for r in raw]
    return dict(zip(names, vals)) if len(set(names)) == len(names) else vals


def summary_text(cols, summaries):
    """st_summary_text: the header line and one line per column -- name, counts, then min, max, mean,
    stdDev and median as JavaScript prints them.  cols: a list of (name, anything) or a dict, for the
    names; summaries: what Context.summary / dev_summary returned (or a list of ColSummary in column
    order).  Host only -> bytes"""
    names = [k for k, _ in (cols.items() if isinstance(cols, dict) else cols)]
    vals = [summaries[k] for k in names] if isinstance(summaries, dict) else list(summaries)
    assert len(vals) == len(names)
    raw = (ColSummaryC * max(1, len(names)))(*[ColSummaryC(*v) for v in vals])
    t = _schema_ttable([(k, np.float32) for k in names], 0)
    out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
    check(lib().st_summary_text(ctypes.byref(t), raw, ctypes.byref(out), ctypes.byref(size)))
    return _take(out, size)


def base64_size(nbytes):
    """the bytes of the base64 text of nbytes bytes (st_base64_size): 4 * ceil(nbytes / 3).  Host only"""
    return lib().st_base64_size(nbytes)


def _vec3(v):
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def html_parts(html, css, js, camera=(2, 2, -2), target=(0, 0, 0)):
    """writeHtml's page text (write-html.ts:11-14,24-36,46-55; st_html_parts) around the payload:
    html / css / js are the viewer template's three strings (str or UTF-8 bytes).  Host only ->
    (prefix bytes, suffix bytes, embeds): the file is prefix + base64 + suffix; a page without
    fetch(contentUrl) has embeds 0, the whole page as prefix and an empty suffix"""
    enc = [t.encode('utf-8') if isinstance(t, str) else bytes(t) for t in (html, css, js)]
    pre, suf = ctypes.c_void_p(), ctypes.c_void_p()
    npre, nsuf, embeds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_int32(0)
    check(lib().st_html_parts(enc[0], enc[1], enc[2], _vec3(camera), _vec3(target), ctypes.byref(pre),
                              ctypes.byref(npre), ctypes.byref(suf), ctypes.byref(nsuf), ctypes.byref(embeds)))
    return _take(pre, npre), _take(suf, nsuf), embeds.value


class BytesSeg(ctypes.Structure):
    _fields_ = [('ptr', ctypes.c_void_p), ('len', ctypes.c_uint64)]


class _OutFd:
    """a path (opened for writing without O_TRUNC: the library cuts the file) or a descriptor of the
    caller's"""

    def __init__(self, out):
        self.own = not isinstance(out, int)
        self.fd = os.open(out, os.O_WRONLY | os.O_CREAT, 0o644) if self.own else out

    def __enter__(self):
        return ctypes.c_int32(self.fd)

    def __exit__(self, *exc):
        if self.own:
            os.close(self.fd)


@contextlib.contextmanager
def _ply_in(path):
    """a .ply file opened read-only, its header read: (descriptor, PlyHeader) while the block runs"""
    fd = os.open(path, os.O_RDONLY)
    try:
        h = PlyHeader()
        check(lib().st_ply_read_header(ctypes.c_int32(fd), ctypes.byref(h)))
        yield fd, h
    finally:
        os.close(fd)


def _host_table(cols):
    """host columns (a dict or a list of (name, numpy array)) -> (the list, its st_ttable)"""
    items = list(cols.items()) if isinstance(cols, dict) else list(cols)
    return items, make_ttable(items, len(items[0][1]) if items else 0)


READER_COLS = ['x', 'y', 'z', 'scale_0', 'scale_1', 'scale_2', 'f_dc_0', 'f_dc_1', 'f_dc_2', 'opacity',
               'rot_0', 'rot_1', 'rot_2', 'rot_3']


def reader_columns(nsh):
    """the column names of the .splat / .ksplat / .spz readers, in their order"""
    return READER_COLS + [f'f_rest_{i}' for i in range(nsh)]


def _layout(fn, *args):
    n, nsh = ctypes.c_uint64(0), ctypes.c_int32(0)
    check(fn(*args, ctypes.byref(n), ctypes.byref(nsh)))
    return n.value, nsh.value


def splat_layout(size):
    """(rows, f_rest columns) of a .splat file of `size` bytes (read-splat.ts:21-29; host only)"""
    return _layout(lib().st_splat_layout, ctypes.c_uint64(size))


def ksplat_layout(data):
    """(rows, f_rest columns) of a .ksplat file's bytes, checked as readKsplat checks them (host only)"""
    data = bytes(data)
    return _layout(lib().st_ksplat_layout, data, ctypes.c_uint64(len(data)))


def spz_layout(data):
    """(rows, f_rest columns) of an inflated .spz stream, checked as readSpz checks it (host only)"""
    data = bytes(data)
    return _layout(lib().st_spz_layout, data, ctypes.c_uint64(len(data)))


def _is_compressed_ply(elements):
    """isCompressedPly (decompress-ply.ts:7-78) over read_ply's [(element, {prop: column})]"""
    if len(elements) not in (2, 3):
        return False
    el = {}
    for name, cols in elements:  # Array.find: the first element of a name
        el.setdefault(name, cols)

    def shaped(cols, names, dt):
        return all(k in cols and cols[k].dtype == dt for k in names)

    chunk, vertex = el.get('chunk'), el.get('vertex')
    if chunk is None or not shaped(chunk, CHUNK_COLS, np.float32):
        return False
    if vertex is None or not shaped(vertex, VERTEX_COLS, np.uint32):
        return False
    rows = lambda cols: len(next(iter(cols.values()))) if cols else 0
    if (rows(vertex) + 255) // 256 != rows(chunk):
        return False
    if len(elements) == 3:
        sh = el.get('sh')
        if sh is None or len(sh) not in (9, 24, 45):
            return False
        if not shaped(sh, [f'f_rest_{i}' for i in range(len(sh))], np.uint8):
            return False
        if rows(sh) != rows(vertex):
            return False
    return True


def spz_inflate(data):
    """the gunzip of readSpz (read-spz.ts:50-75).  A file without the gzip magic is not inflated, and
    the reference then sizes itself from its 4-byte magic buffer: whatever follows, it stops with
    'invalid file header' or 'File too small to be valid .spz format'."""
    data = bytes(data)
    if data[:2] != b'\x1f\x8b':
        if data[:4].ljust(4, b'\0') != b'NGSP':
            raise StError(ST_ERR_ARG, 'invalid file header')
        raise StError(ST_ERR_ARG, 'File too small to be valid .spz format')
    import gzip
    return gzip.decompress(data)


ST_DECLINED = 1
INFLATE_CHUNK = 65536
INFLATE_BUDGET = 512


class InflateStats(ctypes.Structure):
    """st_inflate_stats"""
    _fields_ = [(k, ctypes.c_uint64) for k in ('chunks', 'candidates', 'kept', 'discarded', 'markers', 'stored_blocks',
                                               'fixed_blocks', 'dynamic_blocks')]

    def dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def _declined(rc):
    """True for ST_DECLINED, False for ST_OK; an error raises"""
    if rc == ST_DECLINED:
        return True
    check(rc)
    return False


def gzip_member_layout(data):
    """st_gzip_member_layout: (stream offset, stream bytes, CRC-32, ISIZE) of one gzip member, or None
    when the device path does not take its header (host only)"""
    data = bytes(data)
    off, length, crc, isize = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    if _declined(lib().st_gzip_member_layout(data, ctypes.c_uint64(len(data)), ctypes.byref(off), ctypes.byref(length),
                                             ctypes.byref(crc), ctypes.byref(isize))):
        return None
    return off.value, length.value, crc.value, isize.value


def inflate_head(stream, want):
    """st_inflate_head: the first `want` bytes of a raw deflate stream (fewer when it ends first), or
    None when the stream is broken before them (host only, serial)"""
    stream = bytes(stream)
    out, got = ctypes.create_string_buffer(max(want, 1)), ctypes.c_uint64(0)
    if _declined(lib().st_inflate_head(stream, ctypes.c_uint64(len(stream)), out, ctypes.c_uint64(want), ctypes.byref(got))):
        return None
    return out.raw[:got.value]


def spz_gz_layout(data):
    """st_spz_gz_layout: (rows, f_rest columns, image bytes) of a gzipped .spz file's bytes, or None
    when the device path declines it (host only)"""
    n, nsh, size = ctypes.c_uint64(0), ctypes.c_int32(0), ctypes.c_uint64(0)
    if _declined(lib().st_spz_gz_layout(data, ctypes.c_uint64(len(data)), ctypes.byref(n), ctypes.byref(nsh),
                                        ctypes.byref(size))):
        return None
    return n.value, nsh.value, size.value


def spz_image_size(n, sh_coeffs):
    """the bytes of a raw .spz image of n splats with sh_coeffs (0, 3, 8 or 15) coefficients per
    channel: 16 + n * (19 + 3 * sh_coeffs); 0 for a bad argument (st_spz_image_size; host only)"""
    return lib().st_spz_image_size(ctypes.c_uint64(n), ctypes.c_int32(sh_coeffs))


def ksplat_image_size(n, sh_coeffs, mode, full, partial):
    """the bytes of a .ksplat image of n splats in `full` + `partial` buckets with sh_coeffs (0, 3, 8 or
    15) coefficients per channel in the file: 5120 + 4 partial + 12 (full + partial) + n * stride; 0 for
    a bad argument (st_ksplat_image_size; host only)"""
    return lib().st_ksplat_image_size(n, sh_coeffs, mode, full, partial)


SPZ_DEFLATE_SEGMENT = 8 << 20


def spz_deflate(raw, level, threads=8, _segment=SPZ_DEFLATE_SEGMENT):
    """ONE gzip member (mtime 0, no name) whose inflation is `raw`: the form .spz consumers expect
    around the raw image.  Fixed segments of 8 MiB are raw-deflated independently on up to
    min(threads, 8) threads (zlib releases the GIL), every segment but the last ended with a sync
    flush -- a byte boundary, so the pieces concatenate into one deflate stream -- and the last with
    finish; one CRC-32 runs over the whole input.  The bytes do not depend on the thread count."""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    raw = memoryview(raw).cast('B')
    segs = [raw[o:o + _segment] for o in range(0, len(raw), _segment)] or [raw[:0]]

    def deflate(i):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return c.compress(segs[i]) + c.flush(zlib.Z_FINISH if i + 1 == len(segs) else zlib.Z_SYNC_FLUSH)

    nthreads = max(1, min(int(threads), 8, len(segs)))
    if nthreads == 1:
        parts = [deflate(i) for i in range(len(segs))]
    else:
        with ThreadPoolExecutor(nthreads) as pool:
            parts = list(pool.map(deflate, range(len(segs))))
    crc = 0
    for s in segs:
        crc = zlib.crc32(s, crc)
    # ID1 ID2 CM=8 FLG=0 MTIME=0 XFL=0 OS=255 (unknown)
    head = b'\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff'
    return head + b''.join(parts) + (crc & 0xffffffff).to_bytes(4, 'little') + (len(raw) & 0xffffffff).to_bytes(4, 'little')


DEFLATE_SEG = 65536  # ST_DEFLATE_SEG


def deflate_bound(n):
    """st_deflate_bound: the most bytes Context.dev_deflate writes for n input bytes"""
    return lib().st_deflate_bound(n)


def gzip_bound(n):
    """st_gzip_bound: the most bytes Context.dev_gzip writes for n input bytes"""
    return lib().st_gzip_bound(n)


# ---- the .sog reader's host pieces ------------------------------------------------------------
class ZipEntry(ctypes.Structure):
    _fields_ = [('name_offset', ctypes.c_uint64), ('name_len', ctypes.c_uint32), ('crc', ctypes.c_uint32),
                ('offset', ctypes.c_uint64), ('size', ctypes.c_uint64)]


SOG_TEXTURES = ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')
SOG_FILES = tuple(k + '.webp' for k in SOG_TEXTURES)


def zip_index(data):
    """[(name, data offset, size, crc)] of a ZIP archive's bytes from its central directory
    (st_zip_index: stored entries only; host only)"""
    data = bytes(data)
    n = ctypes.c_int32(0)
    check(lib().st_zip_index(data, ctypes.c_uint64(len(data)), None, ctypes.c_int32(0), ctypes.byref(n)))
    es = (ZipEntry * max(n.value, 1))()
    check(lib().st_zip_index(data, ctypes.c_uint64(len(data)), es, ctypes.c_int32(n.value), ctypes.byref(n)))
    return [(data[e.name_offset:e.name_offset + e.name_len].decode('utf-8', 'replace'), e.offset, e.size, e.crc)
            for e in es[:n.value]]


def webp_info(data):
    """(width, height) of a WebP-lossless file's bytes (host only)"""
    data = bytes(data)
    w, h = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().st_webp_info(data, ctypes.c_uint64(len(data)), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def webp_decode_lossless(data):
    """a WebP-lossless file's bytes -> (height, width, 4) uint8 RGBA (st_webp_decode_lossless: the
    host VP8L decoder, all of RFC 9649)"""
    data = bytes(data)
    w, h = webp_info(data)
    out = np.empty((h, w, 4), np.uint8)
    check(lib().st_webp_decode_lossless(data, ctypes.c_uint64(len(data)), _vp(out), ctypes.c_int32(w * 4)))
    return out


def sog_read_meta(text):
    """meta.json of a SOG (write-sog.ts:271-293, :350-361) -> (SogMeta, count, the texture file names
    in SOG_TEXTURES order: five without an shN entry).  version must be 2 and every `files` entry
    present; a JSON null (the writer's text of a non-finite number) reads as NaN.  The texture
    sizes (width, height, shn_width, shn_height) are left 0: the textures tell them."""
    import json
    if isinstance(text, (bytes, bytearray)):
        text = bytes(text).decode('utf-8')

    def bad(msg):
        return StError(ST_ERR_ARG, 'sog meta.json: ' + msg)

    try:
        m = json.loads(text)
    except ValueError as e:
        raise bad(str(e))
    if not isinstance(m, dict):
        raise bad('not an object')
    if m.get('version') != 2:
        raise StError(ST_ERR_UNSUPPORTED, f"sog meta.json: version {m.get('version')!r} (2 is supported)")
    count = m.get('count')
    if not isinstance(count, int) or isinstance(count, bool) or count < 1:
        raise bad('count must be a positive integer')

    def num(v):
        if v is None:
            return float('nan')
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise bad('a number expected')
        return float(v)

    def files(key, n):
        f = m.get(key, {}).get('files') if isinstance(m.get(key), dict) else None
        if not isinstance(f, list) or len(f) != n or not all(isinstance(x, str) for x in f):
            raise bad(f'{key}.files must list {n} file name' + ('s' if n > 1 else ''))
        return f

    def codebook(key):
        cb = m[key].get('codebook')
        if not isinstance(cb, list) or len(cb) != 256:
            raise bad(f'{key}.codebook must hold 256 numbers')
        return np.array([num(v) for v in cb], np.float64).astype(np.float32)

    names = files('means', 2) + files('quats', 1) + files('scales', 1) + files('sh0', 1)
    meta = SogMeta()
    for key, dst in (('mins', meta.means_min), ('maxs', meta.means_max)):
        v = m['means'].get(key)
        if not isinstance(v, list) or len(v) != 3:
            raise bad(f'means.{key} must hold 3 numbers')
        for a in range(3):
            dst[a] = num(v[a])
    meta.scales_codebook[:] = codebook('scales').tolist()
    meta.sh0_codebook[:] = codebook('sh0').tolist()
    if 'shN' in m:
        names += files('shN', 2)
        sn = m['shN']
        for key in ('count', 'bands'):
            if not isinstance(sn.get(key), int) or isinstance(sn.get(key), bool):
                raise bad(f'shN.{key} must be an integer')
        if not 1 <= sn['bands'] <= 3:
            raise bad('shN.bands must be 1..3')
        if not 1 <= sn['count'] <= 65536:
            raise bad('shN.count must be 1..65536')
        meta.sh_bands, meta.palette_size = sn['bands'], sn['count']
        meta.shn_codebook[:] = codebook('shN').tolist()
    return meta, count, names


def rccl_info():
    """(version, path) of the RCCL the library's collectives run on (st_rccl_info: loaded by path,
    /opt/rocm/lib/librccl.so.1 unless ST_RCCL says otherwise; no GPU needed)"""
    v = ctypes.c_int32(0)
    buf = ctypes.create_string_buffer(4096)
    check(lib().st_rccl_info(ctypes.byref(v), buf, ctypes.c_uint64(len(buf))))
    return v.value, buf.value.decode()


def device_count():
    n = ctypes.c_int32(0)
    check(lib().st_device_count(ctypes.byref(n)))
    return n.value


class Context:
    def __init__(self, device=0):
        # PyTorch-ROCm ships its own HIP runtime next to the one this library links; when both
        # live in one process, torch's must initialise first (the other order leaves torch
        # without a device).  Device tensors are still shared through plain pointers.
        if 'torch' in sys.modules:
            try:
                sys.modules['torch'].cuda.init()
            except RuntimeError:
                pass  # no device: st_ctx_create reports it
        self.h = ctypes.c_void_p()
        self.device = device
        self.last_inflate = None        # 'host' or 'device': the way the last read_spz / read_spz_dev went
        self.last_inflate_stats = None  # st_inflate_stats of the last device inflate, as far as it got
        check(lib().st_ctx_create(ctypes.c_int32(device), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            lib().st_ctx_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        """run on a caller-owned hipStream_t.  Handle 0 is refused: torch's legacy default stream
        has handle 0, which the C ABI reads as NULL = the context's own (non-blocking) stream, so
        the library would silently stop ordering against the caller's torch work."""
        if not stream_handle:
            raise ValueError('set_stream(0): handle 0 selects the context\'s own stream, not the legacy '
                             'default stream; use bind_torch_stream() or use_own_stream()')
        check(lib().st_ctx_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def use_own_stream(self):
        check(lib().st_ctx_set_stream(self.h, None))

    def bind_torch_stream(self, device):
        """one real stream for the library and the caller's torch work on `device`: torch's
        current stream when it is not the legacy default stream, else a new stream made
        current, ordered after what the default stream already holds.  Returns the torch stream."""
        import torch
        s = torch.cuda.current_stream(device)
        if s.cuda_stream == 0:
            prev, s = s, torch.cuda.Stream(device)
            s.wait_stream(prev)  # work already queued on the default stream comes first
            torch.cuda.set_stream(s)
        self.set_stream(s.cuda_stream)
        return s

    def synchronize(self):
        check(lib().st_ctx_synchronize(self.h))

    def timings(self):
        return lib().st_ctx_last_timings(self.h).decode()

    def host_reuse(self):
        """(columns, bytes) the last writeSog host form ran from st_ply_read's resident copy
        (st_ctx_last_host_reuse; (0, 0): it uploaded them)"""
        cols, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().st_ctx_last_host_reuse(self.h, ctypes.byref(cols), ctypes.byref(nb)))
        return cols.value, nb.value

    def sog_file(self, cols, iters, draws, path, dos_time=0, dos_date=0):
        """writeSog of a host table into a file (st_sog_file): (used, size).  The file is opened
        without O_TRUNC (st_sog_file cuts it to the archive's length)"""
        keep = {k: np.ascontiguousarray(v, np.float32) for k, v in cols.items()}
        t = make_table(keep)
        used, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
        fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)
        try:
            check(lib().st_sog_file(self.h, ctypes.byref(t), ctypes.c_int32(iters), _vp(draws),
                                    ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.c_int32(fd),
                                    ctypes.c_uint16(dos_time), ctypes.c_uint16(dos_date), ctypes.byref(size)))
        finally:
            os.close(fd)
        return used.value, size.value

    def kmeans_stats(self):
        """the last N-D k-means' assign classification (st_ctx_last_kmeans_stats) as a dict"""
        import json
        return json.loads(lib().st_ctx_last_kmeans_stats(self.h).decode())

    def _summary(self, fn, cols):
        t = make_ttable(cols)
        raw = (ColSummaryC * max(1, t.ncol))()
        check(fn(self.h, ctypes.byref(t), raw))
        names = [k for k, _ in (cols.items() if isinstance(cols, dict) else cols)]
        return _summaries_out(names, raw[:t.ncol])

    def dev_summary(self, cols):
        """st_dev_summary: the column summary (st_abi.h, "column summary") of device columns (list of
        (name, tensor) or a dict, any of the eight types) read in place -> {name: ColSummary}; a list
        in column order when a name occurs twice"""
        return self._summary(lib().st_dev_summary, cols)

    def summary(self, cols):
        """st_summary: the same of host columns (numpy arrays), uploaded through the staged copies"""
        return self._summary(lib().st_summary, cols)

    def dev_importance(self, cols):
        """st_dev_importance: exp((scale_0 + scale_1) + scale_2) * sigmoid(opacity) of every row of
        device columns (list of (name, tensor) or a dict, any of the eight types) -> float64 tensor"""
        import torch
        t = make_ttable(cols)
        out = torch.empty(t.n, dtype=torch.float64, device=f'cuda:{self.device}')
        check(lib().st_dev_importance(self.h, ctypes.byref(t), _ptr(out)))
        return out

    def dev_importance_order(self, cols):
        """st_dev_importance_order: the rows from the most important down (descending score, NaN
        last, ties by row index) -> torch.int32 tensor holding the uint32 row indices"""
        import torch
        t = make_ttable(cols)
        out = torch.empty(t.n, dtype=torch.int32, device=f'cuda:{self.device}')
        check(lib().st_dev_importance_order(self.h, ctypes.byref(t), _ptr(out)))
        return out

    def dev_importance_top(self, cols, m):
        """st_dev_importance_top: the min(m, n) most important rows' indices, ascending (decimate's
        selection) -> torch.int32 tensor holding the uint32 row indices"""
        import torch
        t = make_ttable(cols)
        k = min(int(m), t.n)
        out = torch.empty(k, dtype=torch.int32, device=f'cuda:{self.device}')
        got = ctypes.c_uint64()
        check(lib().st_dev_importance_top(self.h, ctypes.byref(t), ctypes.c_uint64(int(m)), _ptr(out), ctypes.byref(got)))
        assert got.value == k
        return out

    def _upload(self, cols):
        import torch
        items = list(cols.items()) if isinstance(cols, dict) else list(cols)
        out = []
        for k, a in items:  # as bytes: every one of the eight types, whatever torch converts
            a = np.ascontiguousarray(a)
            raw = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(f'cuda:{self.device}')
            out.append((k, raw.view(_torch_type(a.dtype))))
        return out

    def importance(self, cols):
        """the scores of host columns (numpy arrays), uploaded -> float64 array"""
        return self.dev_importance(self._upload(cols)).cpu().numpy()

    def importance_order(self, cols):
        """the importance order of host columns (numpy arrays), uploaded -> uint32 array"""
        return self.dev_importance_order(self._upload(cols)).cpu().numpy().view(np.uint32)

    def dev_neighbor_dist(self, cols, k):
        """st_dev_neighbor_dist: the distance from every row of device columns (list of (name, tensor)
        or a dict; x, y, z of any of the eight types) to its k-th nearest other placed row (st_abi.h,
        "neighbour distances and outliers") -> float64 tensor"""
        import torch
        t = make_ttable(cols)
        out = torch.empty(t.n, dtype=torch.float64, device=f'cuda:{self.device}')
        check(lib().st_dev_neighbor_dist(self.h, ctypes.byref(t), ctypes.c_int32(int(k)), _ptr(out)))
        return out

    def neighbor_dist(self, cols, k):
        """the same of host columns (numpy arrays), uploaded -> float64 array"""
        return self.dev_neighbor_dist(self._upload(cols), k).cpu().numpy()

    def last_neighbor_stats(self):
        """the last neighbour search's sizes and work (st_ctx_last_neighbor_stats) as a dict: rows,
        placed, leaves, levels, pairs (d2 evaluations), nodes (box tests)"""
        import json
        return json.loads(lib().st_ctx_last_neighbor_stats(self.h).decode())

    def dev_clusters(self, cols, radius):
        """st_dev_clusters: the connected components of device columns (list of (name, tensor) or a dict;
        x, y, z of any of the eight types) linked at `radius` (st_abi.h, "clusters") -> (label, size),
        uint32 tensors: the smallest row index of the row's component (0xFFFFFFFF: not placed) and the
        component's row count (0: not placed)"""
        import torch
        t = make_ttable(cols)
        label = torch.empty(t.n, dtype=torch.uint32, device=f'cuda:{self.device}')
        size = torch.empty(t.n, dtype=torch.uint32, device=f'cuda:{self.device}')
        check(lib().st_dev_clusters(self.h, ctypes.byref(t), ctypes.c_double(float(radius)), _ptr(label), _ptr(size)))
        return label, size

    def clusters(self, cols, radius):
        """the same of host columns (numpy arrays), uploaded -> (label, size) as uint32 arrays"""
        label, size = self.dev_clusters(self._upload(cols), radius)
        return label.cpu().numpy().view(np.uint32), size.cpu().numpy().view(np.uint32)

    def last_cluster_stats(self):
        """the last cluster search's sizes and work (st_ctx_last_cluster_stats) as a dict: rows, placed,
        components, largest, leaves, levels, pairs (d2 evaluations), nodes (box tests), unions"""
        import json
        return json.loads(lib().st_ctx_last_cluster_stats(self.h).decode())

    def summary_stats(self):
        """the last summary's sum paths (st_ctx_last_summary_stats) as a dict: columns, fast, general,
        normalisations, flush"""
        import json
        return json.loads(lib().st_ctx_last_summary_stats(self.h).decode())

    def dev_probe(self, op, in0=None, in1=None, out0=None, out1=None, aux=None, cols=None, n=0, s=0.0,
                  begin_bit=0, end_bit=0):
        """st_dev_probe, a test hook (st_abi.h): one of PROBE_OPS by name or code over device tensors
        (or raw device addresses); cols: the float32 column tensors of 'minmax'.  Returns args.result
        (1 when 'sort_swap' left the result in the caller's pair)"""
        def p(t):
            return ctypes.c_void_p(t) if isinstance(t, int) else _ptr(t)
        a = ProbeArgs(p(in0), p(in1), p(out0), p(out1), p(aux), None, n, s, begin_bit, end_bit, 0, 0)
        if cols is not None:
            a.ncols = len(cols)
            ptrs = (ctypes.c_void_p * max(1, len(cols)))(*[p(t) for t in cols])
            a.cols = ctypes.cast(ptrs, ctypes.c_void_p)
        check(lib().st_dev_probe(self.h, ctypes.c_int32(PROBE_OPS.get(op, op)), ctypes.byref(a)))
        return a.result

    def set_profiling(self, on=True):
        check(lib().st_ctx_set_profiling(self.h, ctypes.c_int32(1 if on else 0)))

    def reset_kernel_stats(self):
        check(lib().st_ctx_reset_kernel_stats(self.h))

    def kernel_stats(self, name):
        """(total_ms, launches) of a named library kernel since the last reset (HIP events, ctx stream)"""
        ms = ctypes.c_double(0)
        cnt = ctypes.c_uint64(0)
        check(lib().st_ctx_kernel_stats(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def set_verify(self, on=True):
        check(lib().st_ctx_set_verify(self.h, ctypes.c_int32(1 if on else 0)))

    def verify_snapshot(self, device='cuda'):
        """(prev_centroids [d, k], centroids [d, k], labels [n]) torch tensors of the last N-D
        k-means run while verification was on (st_ctx_verify_snapshot)"""
        import torch
        d, k, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
        check(lib().st_ctx_verify_snapshot(self.h, None, None, None, ctypes.byref(d), ctypes.byref(k),
                                           ctypes.byref(n)))
        prev = torch.empty((d.value, k.value), dtype=torch.float32, device=device)
        cen = torch.empty_like(prev)
        lab = torch.empty(n.value, dtype=torch.int32, device=device)
        check(lib().st_ctx_verify_snapshot(self.h, _ptr(prev), _ptr(cen), _ptr(lab), ctypes.byref(d),
                                           ctypes.byref(k), ctypes.byref(n)))
        self.synchronize()
        return prev, cen, lab

    # ---- host-memory seams ----------------------------------------------------
    def transform(self, cols, params):
        """transform() in place on host columns (dict name -> array); columns that are not float32
        take st_transform_t (the reference's getRow / setRow on any type)"""
        if any(np.dtype(a.dtype) != np.float32 for a in cols.values()):
            t = make_ttable(cols)
            check(lib().st_transform_t(self.h, ctypes.byref(t), ctypes.byref(params)))
            return
        t = make_table(cols)
        check(lib().st_transform(self.h, ctypes.byref(t), ctypes.byref(params)))

    def filter_finite(self, cols):
        t = make_table(cols)
        out = np.zeros(t.n, np.uint32)
        m = ctypes.c_uint64(0)
        check(lib().st_filter_finite(self.h, ctypes.byref(t), _vp(out), ctypes.byref(m)))
        return out[:m.value]

    def morton_order(self, x, y, z, indices=None):
        n = len(x)
        idx = np.arange(n, dtype=np.uint32) if indices is None else np.ascontiguousarray(indices, np.uint32).copy()
        if any(np.dtype(a.dtype) != np.float32 for a in (x, y, z)):  # ordering.ts reads any type's numbers
            xyz = [np.ascontiguousarray(a) for a in (x, y, z)]
            ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in xyz])
            types = (ctypes.c_int32 * 3)(*[ply_type_of(a) for a in xyz])
            check(lib().st_morton_order_t(self.h, ptrs, types, _vp(idx), ctypes.c_uint64(n)))
            return idx
        check(lib().st_morton_order(self.h, _vp(x), _vp(y), _vp(z), _vp(idx), ctypes.c_uint64(n)))
        return idx

    def pack_compressed(self, cols, order, nsh):
        t = make_table(cols)
        n = t.n
        chunk = np.zeros(((n + 255) // 256) * 18, np.float32)
        vertex = np.zeros(n * 4, np.uint32)
        sh = np.zeros(max(n * nsh, 1), np.uint8)
        check(lib().st_pack_compressed(self.h, ctypes.byref(t), _vp(np.ascontiguousarray(order, np.uint32)),
                                       _vp(chunk), _vp(vertex), _vp(sh)))
        return chunk, vertex, sh[:n * nsh]

    def kmeans(self, col_list, k, iters, draws):
        d, n = len(col_list), len(col_list[0])
        kk = min(k, n)
        cent = np.zeros(d * kk, np.float32)
        labels = np.zeros(n, np.uint32)
        used = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * d)(*[c.ctypes.data for c in col_list])
        check(lib().st_kmeans(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(n), ctypes.c_int32(k),
                              ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used),
                              _vp(cent), _vp(labels)))
        return cent.reshape(d, kk), labels, used.value

    def cluster1d(self, col_list, iters, draws):
        n = len(col_list[0])
        cent = np.zeros(256, np.float32)
        labels = np.zeros(n * len(col_list), np.uint8)
        used = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * len(col_list))(*[c.ctypes.data for c in col_list])
        check(lib().st_cluster1d(self.h, ptrs, ctypes.c_int32(len(col_list)), ctypes.c_uint64(n),
                                 ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used),
                                 _vp(cent), _vp(labels)))
        return cent, labels.reshape(len(col_list), n), used.value

    def sog(self, cols, iters, draws):
        t = make_table(cols)
        C = sum(1 for k in cols if k.startswith('f_rest_')) // 3
        C = {9: 3, 24: 8, 45: 15}.get(3 * C, 0) if C else 0
        W, H, pal, cw, ch = sog_geometry(t.n, C)
        tex = {k: np.zeros(W * H * 4, np.uint8) for k in ('means_l', 'means_u', 'quats', 'scales', 'sh0')}
        if C:
            tex['shN_labels'] = np.zeros(W * H * 4, np.uint8)
            tex['shN_centroids'] = np.zeros(cw * ch * 4, np.uint8)
        out = SogTextures(tex['means_l'].ctypes.data, tex['means_u'].ctypes.data, tex['quats'].ctypes.data,
                          tex['scales'].ctypes.data, tex['sh0'].ctypes.data,
                          tex['shN_centroids'].ctypes.data if C else None,
                          tex['shN_labels'].ctypes.data if C else None)
        meta = SogMeta()
        used = ctypes.c_uint64(0)
        check(lib().st_sog(self.h, ctypes.byref(t), ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)),
                           ctypes.byref(used), ctypes.byref(meta), ctypes.byref(out)))
        res = {k: v.reshape(H, W, 4) for k, v in tex.items() if k != 'shN_centroids'}
        if C:
            res['shN_centroids'] = tex['shN_centroids'].reshape(ch, cw, 4)
        return res, meta, used.value

    def sog_process(self, cols, actions, iters, draws):
        """processDataTable then writeSog's textures + meta on a host table of any column types
        (list of (name, array) or dict): (textures, meta, draws used) as sog()"""
        items, t = _host_table(cols)
        names = [k for k, _ in items]
        first_missing = next((i for i in range(45) if f'f_rest_{i}' not in names), -1)
        C = {9: 3, 24: 8, -1: 15}.get(first_missing, 0)
        tex, out, _ = _sog_out(t.n, C)
        meta = SogMeta()
        used = ctypes.c_uint64(0)
        acts = make_actions(actions)
        check(lib().st_sog_process(self.h, ctypes.byref(t), acts, ctypes.c_int32(len(actions)), ctypes.c_int32(iters),
                                   _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.byref(meta),
                                   ctypes.byref(out)))
        W, H, cw, ch = meta.width, meta.height, meta.shn_width, meta.shn_height
        res = {k: v[:W * H * 4].reshape(H, W, 4) for k, v in tex.items() if k != 'shN_centroids'}
        if meta.sh_bands:
            res['shN_centroids'] = tex['shN_centroids'][:cw * ch * 4].reshape(ch, cw, 4)
        else:
            res.pop('shN_labels', None)
        return res, meta, used.value

    def sog_bundle_process(self, cols, actions, iters, draws, dos_time, dos_date):
        """processDataTable then writeSog to a .sog bundle, any column types: (archive, draws used)"""
        _, t = _host_table(cols)
        acts = make_actions(actions)
        used = ctypes.c_uint64(0)
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(lib().st_sog_bundle_process(self.h, ctypes.byref(t), acts, ctypes.c_int32(len(actions)),
                                          ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)),
                                          ctypes.byref(used), ctypes.c_uint16(dos_time), ctypes.c_uint16(dos_date),
                                          ctypes.byref(out), ctypes.byref(size)))
        return _take(out, size), used.value

    def webp_lossless(self, rgba):
        """WebPEncodeLosslessRGBA of a host (H, W, 4) uint8 array -> .webp bytes"""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(lib().st_webp_lossless(self.h, _vp(rgba), ctypes.c_int32(w), ctypes.c_int32(h), ctypes.c_int32(w * 4),
                                     ctypes.byref(out), ctypes.byref(size)))
        return _take(out, size)

    def read_ply(self, path, resident=False):
        """readPly (read-ply.ts:111-191) -> (comments, [(element, {prop: numpy column})]); rows go through HBM.
        resident: st_ply_read_resident -- the numpy columns stay unfilled (the values live in HBM) until
        materialize(column) or a host form other than writeSog's reads them; keep them alive until then,
        or forget() them.  They belong to this context: another Context and an explicit Group refuse
        them (StError, ST_ERR_ARG) until this one has materialized them; the default group's writeSog
        copies them down first.  A form that overwrites a whole column drops its device copy; one
        that overwrites part of it (a slice) copies the column down first, so the other rows keep the
        read's values"""
        with _ply_in(path) as (fd, h):
            out = []
            read = lib().st_ply_read_resident if resident else lib().st_ply_read
            for ei, (name, count, props) in enumerate(h.layout()):
                cols = {pn: np.empty(count, dt) for pn, dt in props}
                ptrs = (ctypes.c_void_p * max(len(props), 1))(*[cols[pn].ctypes.data for pn, _ in props])
                check(read(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(ei), ptrs))
                if resident:  # st_ply_read_resident's contract: forgotten before the memory goes away
                    for a in cols.values():
                        weakref.finalize(a, _forget_column, weakref.ref(self), a.ctypes.data)
                out.append((name, cols))
            return h.comment_list(), out

    def materialize(self, col):
        """a resident read's column filled from HBM (st_ply_materialize); no-op for any other array"""
        check(lib().st_ply_materialize(self.h, ctypes.c_void_p(col.ctypes.data)))
        return col

    def forget(self, col):
        """drop a resident or mirrored column without copying it (st_ply_forget)"""
        check(lib().st_ply_forget(self.h, ctypes.c_void_p(col.ctypes.data)))

    def decompress_ply(self, chunk, vertex, sh):
        """decompressPly (decompress-ply.ts:82-232): chunk/vertex dicts of numpy columns, sh list of uint8
        columns -> dict of float32 columns in the reference's order"""
        n = len(vertex['packed_position'])
        keep = [np.ascontiguousarray(chunk[k], np.float32) for k in CHUNK_COLS]
        cp = (ctypes.c_void_p * 18)(*[a.ctypes.data for a in keep])
        vk = [np.ascontiguousarray(vertex[k], np.uint32) for k in VERTEX_COLS]
        vp = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in vk])
        sk = [np.ascontiguousarray(a, np.uint8) for a in sh]
        sp = (ctypes.c_void_p * max(len(sk), 1))(*[a.ctypes.data for a in sk])
        names = DECOMP_COLS + [f'f_rest_{i}' for i in range(len(sk))]
        out = {k: np.empty(n, np.float32) for k in names}
        op = (ctypes.c_void_p * len(names))(*[out[k].ctypes.data for k in names])
        check(lib().st_decompress_ply(self.h, ctypes.c_uint64(n), cp, vp, sp, ctypes.c_int32(len(sk)), op))
        return out

    def sog_bundle(self, cols, iters, draws, dos_time, dos_date):
        """writeSog to a .sog bundle: (archive bytes, draws used)"""
        t = make_table(cols)
        used = ctypes.c_uint64(0)
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(lib().st_sog_bundle(self.h, ctypes.byref(t), ctypes.c_int32(iters), _vp(draws),
                                  ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.c_uint16(dos_time),
                                  ctypes.c_uint16(dos_date), ctypes.byref(out), ctypes.byref(size)))
        return _take(out, size), used.value

    # ---- device-memory seams (torch tensors) --------------------------------------
    def dev_webp_lossless(self, rgba, out):
        """rgba: device uint8 (H, W, 4) tensor; out: device uint8 tensor of >= webp_max_size bytes"""
        h, w = rgba.shape[:2]
        size = ctypes.c_uint64(0)
        check(lib().st_dev_webp_lossless(self.h, _ptr(rgba), ctypes.c_int32(w), ctypes.c_int32(h),
                                         ctypes.c_int32(rgba.stride(0)), _ptr(out), ctypes.c_uint64(out.numel()),
                                         ctypes.byref(size)))
        return size.value

    def dev_crc32(self, data, n=None, crc_in=0):
        out = ctypes.c_uint32(0)
        n = data.numel() if n is None else n
        check(lib().st_dev_crc32(self.h, _ptr(data), ctypes.c_uint64(n), ctypes.c_uint32(crc_in),
                                 ctypes.byref(out)))
        return out.value

    def _dev_deflate(self, fn, data, out, n):
        n = data.numel() if n is None else n
        size = ctypes.c_uint64(0)
        check(fn(self.h, _ptr(data), ctypes.c_uint64(n), _ptr(out), ctypes.c_uint64(out.numel()), ctypes.byref(size)))
        return size.value

    def dev_deflate(self, data, out, n=None):
        """st_dev_deflate: the RFC 1951 stream (st_abi.h's rules) of the first n bytes of the device
        uint8 tensor `data` into the device uint8 tensor `out`, both of any alignment -> its bytes.
        A tensor too small raises ST_ERR_ARG and is left untouched"""
        return self._dev_deflate(lib().st_dev_deflate, data, out, n)

    def dev_gzip(self, data, out, n=None):
        """st_dev_gzip: one gzip member around that stream (spz_deflate's header, CRC-32, size)"""
        return self._dev_deflate(lib().st_dev_gzip, data, out, n)

    def _dev_inflate(self, fn, data, out, n, expect, chunk_bytes):
        n = data.numel() if n is None else n
        expect = out.numel() if expect is None else expect
        if expect > out.numel() or n > data.numel():
            raise ValueError('more bytes than the tensor holds')
        st = InflateStats()
        declined = _declined(fn(self.h, _ptr(data), ctypes.c_uint64(n), _ptr(out), ctypes.c_uint64(expect),
                                ctypes.c_uint64(chunk_bytes), ctypes.byref(st)))
        self.last_inflate_stats = st.dict()
        return None if declined else st.dict()

    def dev_inflate(self, data, out, n=None, expect=None, chunk_bytes=0):
        """st_dev_inflate: the raw deflate stream in the first n bytes of the device uint8 tensor `data`
        into the first `expect` bytes of the device uint8 tensor `out` (defaults: all of both), both of
        any alignment -> the statistics as a dict, or None when the device path DECLINES the stream
        (nothing is then promised about `out`; last_inflate_stats holds what was counted)"""
        return self._dev_inflate(lib().st_dev_inflate, data, out, n, expect, chunk_bytes)

    def dev_gunzip(self, data, out, n=None, expect=None, chunk_bytes=0):
        """st_dev_gunzip: the same for one gzip member; its CRC-32 and ISIZE are checked"""
        return self._dev_inflate(lib().st_dev_gunzip, data, out, n, expect, chunk_bytes)

    def dev_sog_bundle_view(self, meta, count, tex, dos_time, dos_date):
        """as dev_sog_bundle without the copy: (address, size) of the context's pinned archive"""
        t = SogTextures(*[(tex[k].data_ptr() if k in tex else None) for k in
                          ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(lib().st_dev_sog_bundle_view(self.h, ctypes.byref(meta), ctypes.c_uint64(count), ctypes.byref(t),
                                           ctypes.c_uint16(dos_time), ctypes.c_uint16(dos_date), ctypes.byref(out),
                                           ctypes.byref(size)))
        return out.value, size.value

    def dev_sog_bundle(self, meta, count, tex, dos_time, dos_date):
        """the .sog archive bytes of device textures (dict as for dev_sog) and their SogMeta"""
        t = SogTextures(*[(tex[k].data_ptr() if k in tex else None) for k in
                          ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        out, size = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(lib().st_dev_sog_bundle(self.h, ctypes.byref(meta), ctypes.c_uint64(count), ctypes.byref(t),
                                      ctypes.c_uint16(dos_time), ctypes.c_uint16(dos_date), ctypes.byref(out),
                                      ctypes.byref(size)))
        return _take(out, size)

    def read_ply_dev(self, path, device='cuda'):
        """readPly into device columns: (comments, [(element, {prop: torch tensor})])"""
        import torch
        tmap = {np.int8: torch.int8, np.uint8: torch.uint8, np.int16: torch.int16, np.uint16: torch.uint16,
                np.int32: torch.int32, np.uint32: torch.uint32, np.float32: torch.float32, np.float64: torch.float64}
        with _ply_in(path) as (fd, h):
            out = []
            for ei, (name, count, props) in enumerate(h.layout()):
                cols = {pn: torch.empty(count, dtype=tmap[dt], device=device) for pn, dt in props}
                ptrs = (ctypes.c_void_p * max(len(props), 1))(*[cols[pn].data_ptr() for pn, _ in props])
                check(lib().st_dev_ply_read(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(ei), ptrs))
                out.append((name, cols))
            return h.comment_list(), out

    # ---- the other input formats (index.ts:52-76) ---------------------------------------
    def _reader_out(self, n, nsh, device):
        names = reader_columns(nsh)
        if device is None:
            cols = {k: np.empty(n, np.float32) for k in names}
            ptrs = (ctypes.c_void_p * len(names))(*[cols[k].ctypes.data for k in names])
        else:
            import torch
            cols = {k: torch.empty(n, dtype=torch.float32, device=device) for k in names}
            ptrs = (ctypes.c_void_p * len(names))(*[cols[k].data_ptr() for k in names])
        return cols, ptrs

    def _read_splat(self, path, device):
        fd = os.open(path, os.O_RDONLY)
        try:
            n, nsh = splat_layout(os.fstat(fd).st_size)
            cols, ptrs = self._reader_out(n, nsh, device)
            read = lib().st_splat_read if device is None else lib().st_dev_splat_read
            check(read(self.h, ctypes.c_int32(fd), ptrs))
            return cols
        finally:
            os.close(fd)

    def _read_bytes(self, data, layout, host_fn, dev_fn, device):
        n, nsh = layout(data)
        cols, ptrs = self._reader_out(n, nsh, device)
        check((host_fn if device is None else dev_fn)(self.h, data, ctypes.c_uint64(len(data)), ptrs))
        return cols

    def read_splat(self, path):
        """readSplat (read-splat.ts:14-148) -> {name: float32 numpy column} in the reader's order; the
        rows stream through HBM in st_dev_ply_read's chunks"""
        return self._read_splat(path, None)

    def read_splat_dev(self, path, device='cuda'):
        """readSplat into device columns (torch tensors)"""
        return self._read_splat(path, device)

    def read_ksplat(self, path):
        """readKsplat (read-ksplat.ts:103-384) -> {name: float32 numpy column}"""
        with open(path, 'rb') as f:
            data = f.read()
        return self._read_bytes(data, ksplat_layout, lib().st_ksplat_read, lib().st_dev_ksplat_read, None)

    def read_ksplat_dev(self, path, device='cuda'):
        """readKsplat into device columns (torch tensors)"""
        with open(path, 'rb') as f:
            data = f.read()
        return self._read_bytes(data, ksplat_layout, lib().st_ksplat_read, lib().st_dev_ksplat_read, device)

    def _read_spz(self, path, device, inflate, chunk_bytes):
        if inflate not in ('host', 'device'):
            raise ValueError("inflate must be 'host' or 'device'")
        with open(path, 'rb') as f:
            file = f.read()
        self.last_inflate = 'host'
        if inflate == 'device':
            lay = spz_gz_layout(file)
            if lay is not None:
                cols, ptrs = self._reader_out(lay[0], lay[1], device)
                st = InflateStats()
                read = lib().st_spz_gz_read if device is None else lib().st_dev_spz_gz_read
                declined = _declined(read(self.h, file, ctypes.c_uint64(len(file)), ptrs, ctypes.c_uint64(chunk_bytes),
                                          ctypes.byref(st)))
                self.last_inflate_stats = st.dict()
                if not declined:
                    self.last_inflate = 'device'
                    return cols
        data = spz_inflate(file)
        return self._read_bytes(data, spz_layout, lib().st_spz_read, lib().st_dev_spz_read, device)

    def read_spz(self, path, inflate='host', chunk_bytes=0):
        """readSpz (read-spz.ts:49-241) -> {name: float32 numpy column}.  inflate='host': the gunzip is
        Python's.  inflate='device': the file's bytes go up as they are and the member is inflated in
        HBM (st_spz_gz_read); a file the device path declines is read the host way, so every accepted
        file and every error stays as it is.  last_inflate says which way the last read went."""
        return self._read_spz(path, None, inflate, chunk_bytes)

    def read_spz_dev(self, path, device='cuda', inflate='host', chunk_bytes=0):
        """readSpz into device columns (torch tensors); `inflate` as for read_spz"""
        return self._read_spz(path, device, inflate, chunk_bytes)

    # ---- the .sog reader (beyond the reference's CLI, which cannot read SOG) --------------------
    def dev_sog_decode(self, meta, count, tex, out):
        """SOG textures already in HBM (dict as dev_sog's: uint8 tensors of width * height * 4 bytes;
        meta's width / height / shn_width / shn_height set) -> `out`, float32 tensors under
        reader_columns(nsh).  Rows past count are not written.  StError(ST_ERR_ARG) "N shN labels
        outside the palette" when any label was (those rows are zero)."""
        t = SogTextures(*[(tex[k].data_ptr() if k in tex else None) for k in SOG_TEXTURES])
        nsh = [0, 9, 24, 45][meta.sh_bands] if 0 <= meta.sh_bands <= 3 else 0
        check(lib().st_dev_sog_decode(self.h, ctypes.byref(meta), ctypes.c_uint64(count), ctypes.byref(t),
                                      self._col_ptrs(out, nsh)))

    def _read_sog_parts(self, meta, count, images, device):
        """decoded textures (numpy (h, w, 4), SOG_TEXTURES order) -> columns through dev_sog_decode"""
        import torch
        dev = 'cuda' if device is None else device
        meta.height, meta.width = images[0].shape[:2]
        if len(images) == 7:
            meta.shn_height, meta.shn_width = images[5].shape[:2]
        wh = (ctypes.c_int32 * 2 * 7)()
        for k, im in enumerate(images):
            wh[k][0], wh[k][1] = im.shape[1], im.shape[0]
        n, nsh = _layout(lib().st_sog_read_layout, ctypes.byref(meta), ctypes.c_uint64(count), wh)
        tex = {k: torch.from_numpy(np.ascontiguousarray(im).reshape(-1)).to(dev) for k, im in zip(SOG_TEXTURES, images)}
        out = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in reader_columns(nsh)}
        self.dev_sog_decode(meta, count, tex, out)
        return out if device is not None else {k: v.cpu().numpy() for k, v in out.items()}

    def _read_sog(self, path, device):
        from concurrent.futures import ThreadPoolExecutor
        low = str(path).lower()
        if low.endswith('meta.json'):
            # the unbundled form: the textures are the sibling files meta.json names
            with open(path, 'rb') as f:
                meta, count, names = sog_read_meta(f.read())
            blobs = []
            for nm in names:
                with open(os.path.join(os.path.dirname(os.path.abspath(path)), nm), 'rb') as f:
                    blobs.append(f.read())
        else:
            with open(path, 'rb') as f:
                data = f.read()
            index = {}
            for name, off, size, _ in zip_index(data):
                index.setdefault(name, (off, size))  # the first entry of a name
            if 'meta.json' not in index:
                raise StError(ST_ERR_ARG, 'sog: the archive has no meta.json')
            off, size = index['meta.json']
            meta, count, names = sog_read_meta(data[off:off + size])
            if tuple(names) == SOG_FILES[:len(names)]:
                # the writer's names: the whole read in one native call
                nsh = [0, 9, 24, 45][meta.sh_bands]
                if names[0] in index:  # before the columns are allocated by meta.json's word alone
                    off, size = index[names[0]]
                    w, h = webp_info(data[off:off + size])
                    if count > w * h:
                        raise StError(ST_ERR_ARG, 'sog: the textures hold fewer texels than count')
                cols, ptrs = self._reader_out(count, nsh, device)
                read = lib().st_sog_read if device is None else lib().st_dev_sog_read
                check(read(self.h, data, ctypes.c_uint64(len(data)), ctypes.byref(meta), ctypes.c_uint64(count), ptrs))
                return cols
            blobs = []
            for nm in names:
                if nm not in index:
                    raise StError(ST_ERR_ARG, f'sog: the archive has no {nm}')
                off, size = index[nm]
                blobs.append(data[off:off + size])
        with ThreadPoolExecutor(max_workers=len(blobs)) as pool:  # at most seven; ctypes drops the GIL
            images = list(pool.map(webp_decode_lossless, blobs))
        return self._read_sog_parts(meta, count, images, device)

    def read_sog(self, path):
        """a SOG -> {name: float32 numpy column} under reader_columns(nsh): `*.sog` is the bundle,
        a path ending `meta.json` the unbundled form (index.ts:88 treats both as SOG).  Beyond the
        reference's CLI, which writes SOG and cannot read it: the decode rules are in st_abi.h."""
        return self._read_sog(path, None)

    def read_sog_dev(self, path, device='cuda'):
        """read_sog into device columns (torch tensors)"""
        return self._read_sog(path, device)

    def read_table(self, path):
        """the CLI's input dispatch (index.ts:52-76) on the lower-cased file name: .ksplat, .splat,
        .ply (decompressed when it is a compressed PLY, as decompress-ply.ts:35-80 tells), .spz; and,
        beyond the reference, .sog and meta.json (read_sog) -> {name: numpy column} of the splat table"""
        low = str(path).lower()
        if low.endswith('.sog') or low.endswith('meta.json'):
            return self.read_sog(path)
        if low.endswith('.ksplat'):
            return self.read_ksplat(path)
        if low.endswith('.splat'):
            return self.read_splat(path)
        if low.endswith('.ply'):
            _, els = self.read_ply(path)
            el = dict(els)
            if _is_compressed_ply(els):
                shc = [el['sh'][f'f_rest_{i}'] for i in range(len(el['sh']))] if 'sh' in el else []
                return self.decompress_ply(el['chunk'], el['vertex'], shc)
            if 'vertex' not in el:
                raise StError(ST_ERR_ARG, 'the PLY file has no vertex element')
            return el['vertex']
        if low.endswith('.spz'):
            return self.read_spz(path)
        raise StError(ST_ERR_UNSUPPORTED, f'Unsupported input file type: {path}')

    @staticmethod
    def _col_ptrs(out, nsh):
        names = reader_columns(nsh)
        return (ctypes.c_void_p * len(names))(*[out[k].data_ptr() for k in names])

    def dev_splat_decode(self, rows, out):
        """.splat rows already in HBM (uint8 tensor of n * 32 bytes, 16-byte aligned) -> `out`, a dict
        of float32 tensors (reader_columns(0))"""
        check(lib().st_dev_splat_decode(self.h, _ptr(rows), ctypes.c_uint64(rows.numel() // 32),
                                        self._col_ptrs(out, 0)))

    def dev_ksplat_decode(self, headers, file, out):
        """a .ksplat file already in HBM (uint8 tensor) with a host copy of (at least) its headers
        (bytes) -> `out` (reader_columns(nsh) of ksplat_layout)"""
        headers = bytes(headers)
        nsh = len(out) - 14
        check(lib().st_dev_ksplat_decode(self.h, headers, ctypes.c_uint64(len(headers)), _ptr(file),
                                         ctypes.c_uint64(file.numel()), self._col_ptrs(out, nsh)))

    def dev_spz_decode(self, file, out):
        """an inflated .spz stream already in HBM (uint8 tensor) -> `out` (reader_columns(nsh))"""
        check(lib().st_dev_spz_decode(self.h, _ptr(file), ctypes.c_uint64(file.numel()),
                                      self._col_ptrs(out, len(out) - 14)))

    def dev_ply_transpose(self, header, element, rows, out):
        """st_dev_ply_transpose: an element's rows already in HBM -> `out`, its property tensors in order"""
        ptrs = (ctypes.c_void_p * max(len(out), 1))(*[t.data_ptr() for t in out])
        nrows = rows.numel() // max(int(lib().st_ply_row_bytes(ctypes.byref(header), ctypes.c_int32(element))), 1)
        check(lib().st_dev_ply_transpose(self.h, ctypes.byref(header), ctypes.c_int32(element), _ptr(rows),
                                         ctypes.c_uint64(nrows), ptrs))

    def dev_decompress_ply(self, chunk, vertex, sh, out):
        """device form of decompress_ply: torch tensors in, `out` dict of float32 tensors (DECOMP_COLS + f_rest_*)"""
        n = vertex['packed_position'].numel()
        cp = (ctypes.c_void_p * 18)(*[chunk[k].data_ptr() for k in CHUNK_COLS])
        vp = (ctypes.c_void_p * 4)(*[vertex[k].data_ptr() for k in VERTEX_COLS])
        sp = (ctypes.c_void_p * max(len(sh), 1))(*[a.data_ptr() for a in sh])
        names = DECOMP_COLS + [f'f_rest_{i}' for i in range(len(sh))]
        op = (ctypes.c_void_p * len(names))(*[out[k].data_ptr() for k in names])
        check(lib().st_dev_decompress_ply(self.h, ctypes.c_uint64(n), cp, vp, sp, ctypes.c_int32(len(sh)), op))

    def dev_transform(self, cols, params):
        t = make_table(cols)
        check(lib().st_dev_transform(self.h, ctypes.byref(t), ctypes.byref(params)))

    def dev_morton_order(self, x, y, z, idx):
        check(lib().st_dev_morton_order(self.h, _ptr(x), _ptr(y), _ptr(z), _ptr(idx), ctypes.c_uint64(len(idx))))

    def dev_pack_compressed(self, cols, order, chunk, vertex, sh):
        t = make_table(cols)
        check(lib().st_dev_pack_compressed(self.h, ctypes.byref(t), _ptr(order), _ptr(chunk), _ptr(vertex),
                                           _ptr(sh)))

    def dev_filter_finite(self, cols, out_idx):
        t = make_table(cols)
        m = ctypes.c_uint64(0)
        check(lib().st_dev_filter_finite(self.h, ctypes.byref(t), _ptr(out_idx), ctypes.byref(m)))
        return m.value

    def filter_nan(self, cols):
        """filterNaN on host columns (list of (name, numpy array), any type) -> the surviving rows"""
        items, ts = _host_table(cols)
        out = [(k, np.empty_like(a)) for k, a in items]
        td = make_ttable(out)
        m = ctypes.c_uint64()
        check(lib().st_filter_nan(self.h, ctypes.byref(ts), ctypes.byref(td), ctypes.byref(m)))
        return [(k, a[:m.value].copy()) for k, a in out]

    def process(self, cols, actions):
        """processDataTable (process.ts:64-145) on host columns (list of (name, numpy array) or a
        dict) in one upload -> the processed table as a list of (name, array).  As in the
        reference, the transforms before the first filter mutate the input arrays (`result` is
        the input table until a filter copies it; filterBands renames its columns without copying
        them): that region runs first and is written back, the rest runs on the mutated columns.
        Without a filter the result's arrays ARE the input's."""
        items = list(cols.items()) if isinstance(cols, dict) else list(cols)
        first = next((i for i, a in enumerate(actions) if a['kind'] in FILTER_KINDS), len(actions))
        region = actions[:first]
        rs = process_schema(items, region, with_source=True)
        if any(a['kind'] in TRANSFORM_KINDS for a in region):
            for (_, a), (_, _, src) in zip(self._process(items, region), rs):
                np.copyto(items[src][1], a)
        if first == len(actions):
            return [(k, items[src][1]) for k, _, src in rs]
        return self._process(items, [a for i, a in enumerate(actions) if i >= first or a['kind'] not in TRANSFORM_KINDS])

    def _process(self, items, actions):
        """st_process: the action list in one upload, the input untouched"""
        n = len(items[0][1]) if items else 0
        out = [(k, np.empty(n, t)) for k, t in process_schema(items, actions)]
        ts, td = make_ttable(items), make_ttable(out, n)
        acts = make_actions(actions)
        m = ctypes.c_uint64()
        check(lib().st_process(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), ctypes.byref(td),
                               ctypes.byref(m)))
        return [(k, a[:m.value].copy()) for k, a in out]

    def compressed_ply(self, cols, actions):
        """processDataTable then writeCompressedPly's device part, one upload: (m, chunk, vertex, sh)"""
        _, ts = _host_table(cols)
        n = ts.n
        chunk = np.zeros(max(1, (n + 255) // 256 * 18), np.float32)
        vertex = np.zeros(max(1, n * 4), np.uint32)
        sh = np.zeros(max(1, n * 45), np.uint8)
        acts = make_actions(actions)
        m, C = ctypes.c_uint64(), ctypes.c_int32()
        check(lib().st_compressed_ply(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), _vp(chunk),
                                      _vp(vertex), _vp(sh), ctypes.byref(m), ctypes.byref(C)))
        m, C = m.value, C.value
        return m, chunk[:(m + 255) // 256 * 18], vertex[:m * 4], sh[:m * 3 * C]

    def dev_compressed_ply(self, cols, actions, chunk, vertex, sh):
        """the same over device columns (list of (name, tensor)) into device outputs sized for n rows"""
        ts = make_ttable(cols)
        acts = make_actions(actions)
        m, C = ctypes.c_uint64(), ctypes.c_int32()
        check(lib().st_dev_compressed_ply(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), _ptr(chunk),
                                          _ptr(vertex), _ptr(sh), ctypes.byref(m), ctypes.byref(C)))
        return m.value, C.value

    def ply_compressed_ply(self, path, actions, element=-1):
        """readPly + processDataTable + writeCompressedPly's arrays from the file, resident in HBM
        (st_ply_compressed_ply): (m, chunk, vertex, sh)"""
        with _ply_in(path) as (fd, h):
            ei = element if element >= 0 else [e[0] for e in h.layout()].index('vertex')
            n = h.layout()[ei][1]
            chunk = np.zeros(max(1, (n + 255) // 256 * 18), np.float32)
            vertex = np.zeros(max(1, n * 4), np.uint32)
            sh = np.zeros(max(1, n * 45), np.uint8)
            acts = make_actions(actions)
            m, C = ctypes.c_uint64(), ctypes.c_int32()
            check(lib().st_ply_compressed_ply(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element),
                                              acts, ctypes.c_int32(len(actions)), _vp(chunk), _vp(vertex), _vp(sh),
                                              ctypes.byref(m), ctypes.byref(C)))
        m, C = m.value, C.value
        return m, chunk[:(m + 255) // 256 * 18], vertex[:m * 4], sh[:m * 3 * C]

    def ply_compressed_ply_file(self, path, actions, out_path, version=None, element=-1):
        """readPly + processDataTable + writeCompressedPly into out_path (st_ply_compressed_ply_file:
        the arrays written at offsets as they leave HBM; the file opened without O_TRUNC, cut to
        length by the library): (m, sh_coeffs, file bytes)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            m, C, size = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
            ofd = os.open(out_path, os.O_WRONLY | os.O_CREAT, 0o644)
            try:
                check(lib().st_ply_compressed_ply_file(self.h, ctypes.c_int32(fd), ctypes.byref(h),
                                                       ctypes.c_int32(element), acts, ctypes.c_int32(len(actions)),
                                                       ctypes.c_int32(ofd), version.encode() if version else None,
                                                       ctypes.byref(m), ctypes.byref(C), ctypes.byref(size)))
            finally:
                os.close(ofd)
        return m.value, C.value, size.value

    def compressed_ply_file(self, cols, actions, out_path, version=None):
        """processDataTable + writeCompressedPly of a host table into out_path (st_compressed_ply_file):
        (m, sh_coeffs, file bytes)"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        m, C, size = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
        ofd = os.open(out_path, os.O_WRONLY | os.O_CREAT, 0o644)
        try:
            check(lib().st_compressed_ply_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)),
                                               ctypes.c_int32(ofd), version.encode() if version else None,
                                               ctypes.byref(m), ctypes.byref(C), ctypes.byref(size)))
        finally:
            os.close(ofd)
        return m.value, C.value, size.value

    # ---- writePly (write-ply.ts) ---------------------------------------------------------
    def dev_ply_rows(self, cols, out, row0=0, nrows=None):
        """st_dev_ply_rows: rows [row0, row0 + nrows) of device columns (list of (name, tensor) or a
        dict, any types) interleaved into `out`, a device uint8 tensor of >= nrows * row bytes"""
        t = make_ttable(cols)
        if nrows is None:
            nrows = t.n - row0
        check(lib().st_dev_ply_rows(self.h, ctypes.byref(t), ctypes.c_uint64(row0), ctypes.c_uint64(nrows),
                                    _ptr(out)))

    def ply_rows_file(self, cols, out):
        """the rows alone of a table (numpy columns: st_ply_rows_file, uploaded once; torch tensors:
        st_dev_ply_rows_file) written at the position of `out`, a descriptor or a path -> bytes written"""
        t = make_ttable(cols)
        dev = t.ncol and hasattr(t._keep[3][0][1], 'data_ptr')
        size = ctypes.c_uint64()
        with _OutFd(out) as fd:
            check((lib().st_dev_ply_rows_file if dev else lib().st_ply_rows_file)(self.h, ctypes.byref(t), fd,
                                                                                 ctypes.byref(size)))
        return size.value

    def dev_ply_file(self, elements, out, comments=()):
        """writePly (write-ply.ts:18-68) of tables already in HBM: elements is a list of (element name,
        columns) -- or (element name, columns, rows) for an element without columns -- or the columns
        of one 'vertex' element (list of (name, tensor) or a dict); the header is composed here and
        each element's rows stream down through st_dev_ply_rows_file.  `out`: a path or a descriptor
        (written from its position) -> bytes written"""
        if isinstance(elements, dict) or (elements and not isinstance(elements[0][1], (dict, list, tuple))):
            elements = [('vertex', elements)]
        tables = [(e[0], make_ttable(e[1], e[2] if len(e) > 2 else None)) for e in elements]
        head = b'ply\nformat binary_little_endian 1.0\n' + b''.join(b'comment %s\n' % c.encode() for c in comments)
        for e, (name, t) in zip(elements, tables):
            items = list(e[1].items()) if isinstance(e[1], dict) else list(e[1])
            head += ply_header_text(items, t.n, name, element_only=True)
        head += b'end_header\n'
        with _OutFd(out) as fd:
            total = len(head)
            pos = os.lseek(fd.value, 0, os.SEEK_CUR)
            os.pwrite(fd.value, head, pos)
            os.lseek(fd.value, pos + total, os.SEEK_SET)
            for _, t in tables:
                size = ctypes.c_uint64()
                check(lib().st_dev_ply_rows_file(self.h, ctypes.byref(t), fd, ctypes.byref(size)))
                total += size.value
        return total

    def ply_file(self, cols, actions, out, comments=()):
        """processDataTable + writePly of a host table (list of (name, numpy array) or a dict) into
        `out`, a path or a descriptor (st_ply_file): (rows written, file bytes).  The input arrays are
        not changed"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        cs, nc = _comments_arg(comments)
        m, size = ctypes.c_uint64(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_ply_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), cs, nc, fd,
                                    ctypes.byref(m), ctypes.byref(size)))
        return m.value, size.value

    def ply_ply_file(self, path, actions, out, comments=(), element=-1):
        """the CLI's `in.ply [actions] out.ply` (st_ply_ply_file): the element's rows stay in HBM from
        ingest to output: (rows written, file bytes)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            cs, nc = _comments_arg(comments)
            m, size = ctypes.c_uint64(), ctypes.c_uint64()
            with _OutFd(out) as ofd:
                check(lib().st_ply_ply_file(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                            ctypes.c_int32(len(actions)), cs, nc, ofd, ctypes.byref(m),
                                            ctypes.byref(size)))
        return m.value, size.value

    # ---- writeCsv (write-csv.ts) ---------------------------------------------------------
    def dev_csv_rows(self, cols, out, row0=0, nrows=None):
        """st_dev_csv_rows: the text of rows [row0, row0 + nrows) of device columns (list of (name,
        tensor) or a dict, any types) at `out`, a device uint8 tensor -> the bytes written.  A tensor
        too small for them raises ST_ERR_ARG and is left untouched"""
        t = make_ttable(cols)
        if nrows is None:
            nrows = t.n - row0
        size = ctypes.c_uint64()
        check(lib().st_dev_csv_rows(self.h, ctypes.byref(t), ctypes.c_uint64(row0), ctypes.c_uint64(nrows), _ptr(out),
                                    ctypes.c_uint64(out.numel()), ctypes.byref(size)))
        return size.value

    def dev_csv_file(self, cols, out):
        """writeCsv (write-csv.ts:5-23) of a table already in HBM (list of (name, tensor) or a dict)
        into `out`, a path or a descriptor (written from its position) -> bytes written"""
        t = make_ttable(cols)
        size = ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_dev_csv_file(self.h, ctypes.byref(t), fd, ctypes.byref(size)))
        return size.value

    def csv_file(self, cols, actions, out):
        """processDataTable + writeCsv of a host table (list of (name, numpy array) or a dict) into
        `out`, a path or a descriptor (st_csv_file): (rows written, file bytes).  The input arrays are
        not changed"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        m, size = ctypes.c_uint64(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_csv_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), fd,
                                    ctypes.byref(m), ctypes.byref(size)))
        return m.value, size.value

    def ply_csv_file(self, path, actions, out, element=-1):
        """the CLI's `in.ply [actions] out.csv` (st_ply_csv_file): the element's rows stay in HBM from
        ingest to output: (rows written, file bytes)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            m, size = ctypes.c_uint64(), ctypes.c_uint64()
            with _OutFd(out) as ofd:
                check(lib().st_ply_csv_file(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                            ctypes.c_int32(len(actions)), ofd, ctypes.byref(m), ctypes.byref(size)))
        return m.value, size.value

    # ---- the .splat and .spz writers (st_abi.h, "the .splat and .spz writers") ------------------
    def dev_splat_rows(self, cols, out, row0=0, nrows=None):
        """st_dev_splat_rows: rows [row0, row0 + nrows) of device columns (list of (name, tensor) or a
        dict, any types) as 32-byte .splat rows at `out`, a device uint8 tensor (4-byte aligned) of
        >= nrows * 32 bytes"""
        t = make_ttable(cols)
        if nrows is None:
            nrows = t.n - row0
        if out.numel() < 32 * nrows:
            raise StError(ST_ERR_ARG, 'splat rows: the output buffer is too small')
        check(lib().st_dev_splat_rows(self.h, ctypes.byref(t), ctypes.c_uint64(row0), ctypes.c_uint64(nrows), _ptr(out)))

    def dev_spz_planes(self, cols, planes, fractional_bits=12, row0=0, nrows=None):
        """st_dev_spz_planes: rows [row0, row0 + nrows) of device columns into the six .spz planes
        (positions, alphas, colours, scales, rotations, harmonics): `planes` is a list of six device
        uint8 tensors of any alignment -- where row0's bytes of each plane go -- or None to skip one
        -> the position values clamped"""
        t = make_ttable(cols)
        if nrows is None:
            nrows = t.n - row0
        ptrs = (ctypes.c_void_p * 6)(*[(p.data_ptr() if p is not None else None) for p in planes])
        clamped = ctypes.c_uint64()
        check(lib().st_dev_spz_planes(self.h, ctypes.byref(t), ctypes.c_int32(fractional_bits), ctypes.c_uint64(row0),
                                      ctypes.c_uint64(nrows), ptrs, ctypes.byref(clamped)))
        return clamped.value

    def dev_spz_image(self, cols, out, fractional_bits=12):
        """st_dev_spz_image: the raw .spz image (header + planes) of device columns at `out`, a device
        uint8 tensor of any alignment -> (bytes written, position values clamped).  A tensor too small
        raises ST_ERR_ARG and is left untouched"""
        t = make_ttable(cols)
        size, clamped = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().st_dev_spz_image(self.h, ctypes.byref(t), ctypes.c_int32(fractional_bits), _ptr(out),
                                     ctypes.c_uint64(out.numel()), ctypes.byref(size), ctypes.byref(clamped)))
        return size.value, clamped.value

    def dev_splat_file(self, cols, out):
        """a table already in HBM (list of (name, tensor) or a dict) as a .splat file in `out`, a path
        or a descriptor (written from its position) -> bytes written"""
        t = make_ttable(cols)
        size = ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_dev_splat_file(self.h, ctypes.byref(t), fd, ctypes.byref(size)))
        return size.value

    def splat_file(self, cols, actions, out):
        """processDataTable + the .splat writer on a host table (list of (name, numpy array) or a
        dict) into `out`, a path or a descriptor (st_splat_file): (rows written, file bytes)"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        m, size = ctypes.c_uint64(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_splat_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), fd,
                                      ctypes.byref(m), ctypes.byref(size)))
        return m.value, size.value

    def ply_splat_file(self, path, actions, out, element=-1):
        """`in.ply [actions] out.splat` (st_ply_splat_file): the element's rows stay in HBM from
        ingest to output: (rows written, file bytes)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            m, size = ctypes.c_uint64(), ctypes.c_uint64()
            with _OutFd(out) as ofd:
                check(lib().st_ply_splat_file(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                              ctypes.c_int32(len(actions)), ofd, ctypes.byref(m), ctypes.byref(size)))
        return m.value, size.value

    @staticmethod
    def _spz_out(call, out, gzip_level, deflate='host'):
        """call(fd, gz) runs a .spz file form (gz: its st_*_gz_file twin) into a descriptor and returns
        (rows, bytes, clamped).  gzip_level 0: the raw form straight into `out`.  deflate='device': the
        gz form straight into `out`, the member made on the device (any non-zero level: the stream is
        fixed by st_abi.h's rules).  Otherwise (deflate='host') the raw image goes into an anonymous memory
        file, spz_deflate makes the one gzip member and that is written at out's position, under the
        library's rules for an output descriptor: (rows, file bytes, clamped)"""
        if deflate not in ('host', 'device'):
            raise ValueError("deflate must be 'host' or 'device'")
        if gzip_level == 0 or deflate == 'device':
            with _OutFd(out) as fd:
                return call(fd, gzip_level != 0)
        import fcntl
        import mmap
        with _OutFd(out) as fd:
            try:
                flags = fcntl.fcntl(fd.value, fcntl.F_GETFL)
                pos = os.lseek(fd.value, 0, os.SEEK_CUR)
            except OSError:
                raise StError(ST_ERR_ARG, 'spz file: the output descriptor is not a seekable file') from None
            if flags & os.O_ACCMODE == os.O_RDONLY or flags & os.O_APPEND:
                raise StError(ST_ERR_ARG, 'spz file: the output descriptor must be open for writing, not O_APPEND')
            mfd = os.memfd_create('spz_raw')
            try:
                rows, size, clamped = call(ctypes.c_int32(mfd), False)
                mm = mmap.mmap(mfd, size, access=mmap.ACCESS_READ)
                try:
                    member = spz_deflate(mm, gzip_level)
                finally:
                    mm.close()
            finally:
                os.close(mfd)
            done = 0
            while done < len(member):
                done += os.pwrite(fd.value, memoryview(member)[done:done + (1 << 30)], pos + done)
            os.ftruncate(fd.value, pos + len(member))
            os.lseek(fd.value, pos + len(member), os.SEEK_SET)
            return rows, len(member), clamped

    def dev_spz_file(self, cols, out, fractional_bits=12, gzip_level=6, deflate='host'):
        """a table already in HBM (list of (name, tensor) or a dict) as a .spz file in `out`, a path or
        a descriptor (written from its position): (rows, file bytes, position values clamped).
        gzip_level 0 writes the raw image; otherwise one gzip member around it: deflate='host' makes it
        with spz_deflate at that level, deflate='device' on the device (st_dev_spz_gz_file)"""
        t = make_ttable(cols)

        def call(fd, gz):
            size, clamped = ctypes.c_uint64(), ctypes.c_uint64()
            form = lib().st_dev_spz_gz_file if gz else lib().st_dev_spz_file
            check(form(self.h, ctypes.byref(t), ctypes.c_int32(fractional_bits), fd, ctypes.byref(size),
                       ctypes.byref(clamped)))
            return t.n, size.value, clamped.value
        return self._spz_out(call, out, gzip_level, deflate)

    def spz_file(self, cols, actions, out, fractional_bits=12, gzip_level=6, deflate='host'):
        """processDataTable + the .spz writer on a host table (list of (name, numpy array) or a dict)
        into `out` (st_spz_file; deflate='device': st_spz_gz_file): (rows written, file bytes, position
        values clamped)"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)

        def call(fd, gz):
            m, size, clamped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            form = lib().st_spz_gz_file if gz else lib().st_spz_file
            check(form(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), ctypes.c_int32(fractional_bits),
                       fd, ctypes.byref(m), ctypes.byref(size), ctypes.byref(clamped)))
            return m.value, size.value, clamped.value
        return self._spz_out(call, out, gzip_level, deflate)

    def ply_spz_file(self, path, actions, out, fractional_bits=12, gzip_level=6, element=-1, deflate='host'):
        """`in.ply [actions] out.spz` (st_ply_spz_file): the element's rows stay in HBM from ingest to
        the image (deflate='device': to the gzip member, st_ply_spz_gz_file): (rows written, file bytes,
        position values clamped)"""
        acts = make_actions(actions)

        def call(ofd, gz):
            with _ply_in(path) as (fd, h):
                m, size, clamped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
                form = lib().st_ply_spz_gz_file if gz else lib().st_ply_spz_file
                check(form(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                           ctypes.c_int32(len(actions)), ctypes.c_int32(fractional_bits), ofd, ctypes.byref(m),
                           ctypes.byref(size), ctypes.byref(clamped)))
            return m.value, size.value, clamped.value
        return self._spz_out(call, out, gzip_level, deflate)

    # ---- the .ksplat writer (st_abi.h, "the .ksplat writer") -------------------------------------
    def dev_ksplat_plan(self, cols, block_size=5.0):
        """st_dev_ksplat_plan: the bucket plan of device columns (x, y, z of any types) -> a dict of
        device tensors and counts: order (source row of each record), bucket (of each record), centres
        [F + P, 3] float32, partial_sizes [P], full, partial, clamped"""
        import torch
        t = make_ttable(cols)
        items = list(cols.items()) if isinstance(cols, dict) else list(cols)
        dev = items[0][1].device
        n = max(t.n, 1)
        order = torch.empty(n, dtype=torch.int32, device=dev)
        bucket = torch.empty(n, dtype=torch.int32, device=dev)
        centres = torch.empty(3 * n, dtype=torch.float32, device=dev)
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        full, partial, clamped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().st_dev_ksplat_plan(self.h, ctypes.byref(t), ctypes.c_float(block_size), ctypes.c_uint64(n), _ptr(order),
                                       _ptr(bucket), _ptr(centres), _ptr(sizes), ctypes.byref(full), ctypes.byref(partial),
                                       ctypes.byref(clamped)))
        nb = full.value + partial.value
        return dict(order=order[:t.n], bucket=bucket[:t.n], centres=centres[:3 * nb].reshape(nb, 3),
                    partial_sizes=sizes[:partial.value], full=full.value, partial=partial.value, clamped=clamped.value)

    def dev_ksplat_records(self, cols, out, mode, order, bucket, centres, degree=-1, block_size=5.0, quant_range=32767,
                           sh_min=-1.5, sh_max=1.5, rec0=0, nrec=None):
        """st_dev_ksplat_records: records [rec0, rec0 + nrec) of device columns at `out`, a device uint8
        tensor of any alignment, through the caller's grid: order (int32 tensor or None: record r is row
        r), bucket (of each record) and centres (float32, 3 per bucket) -- None in mode 0 --, the block
        size and the quantisation range"""
        t = make_ttable(cols)
        if nrec is None:
            nrec = t.n - rec0
        nb = centres.numel() // 3 if centres is not None else 0
        check(lib().st_dev_ksplat_records(self.h, ctypes.byref(t), ctypes.c_int32(mode), ctypes.c_int32(degree),
                                          ctypes.c_float(sh_min), ctypes.c_float(sh_max), ctypes.c_float(block_size),
                                          ctypes.c_uint32(quant_range), _ptr(order), _ptr(bucket), _ptr(centres),
                                          ctypes.c_uint64(nb), ctypes.c_uint64(rec0), ctypes.c_uint64(nrec), _ptr(out)))

    def dev_ksplat_image(self, cols, out, mode=1, degree=-1, block_size=5.0, sh_min=-1.5, sh_max=1.5):
        """st_dev_ksplat_image: the whole .ksplat image of device columns at `out`, a device uint8 tensor
        of any alignment -> (bytes the image needs, position values clamped).  A tensor too small raises
        ST_ERR_ARG and is left untouched"""
        t = make_ttable(cols)
        size, clamped = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().st_dev_ksplat_image(self.h, ctypes.byref(t), ctypes.c_int32(mode), ctypes.c_int32(degree),
                                        ctypes.c_float(block_size), ctypes.c_float(sh_min), ctypes.c_float(sh_max), _ptr(out),
                                        ctypes.c_uint64(out.numel()), ctypes.byref(size), ctypes.byref(clamped)))
        return size.value, clamped.value

    def dev_ksplat_file(self, cols, out, mode=1, degree=-1, block_size=5.0, sh_min=-1.5, sh_max=1.5):
        """a table already in HBM (list of (name, tensor) or a dict) as a .ksplat file in `out`, a path or
        a descriptor (written from its position): (rows, file bytes, position values clamped)"""
        t = make_ttable(cols)
        size, clamped = ctypes.c_uint64(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_dev_ksplat_file(self.h, ctypes.byref(t), ctypes.c_int32(mode), ctypes.c_int32(degree),
                                           ctypes.c_float(block_size), ctypes.c_float(sh_min), ctypes.c_float(sh_max), fd,
                                           ctypes.byref(size), ctypes.byref(clamped)))
        return t.n, size.value, clamped.value

    def ksplat_file(self, cols, actions, out, mode=1, degree=-1, block_size=5.0, sh_min=-1.5, sh_max=1.5):
        """processDataTable + the .ksplat writer on a host table (list of (name, numpy array) or a dict)
        into `out` (st_ksplat_file): (rows written, file bytes, position values clamped)"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        m, size, clamped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_ksplat_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), ctypes.c_int32(mode),
                                       ctypes.c_int32(degree), ctypes.c_float(block_size), ctypes.c_float(sh_min),
                                       ctypes.c_float(sh_max), fd, ctypes.byref(m), ctypes.byref(size), ctypes.byref(clamped)))
        return m.value, size.value, clamped.value

    def ply_ksplat_file(self, path, actions, out, mode=1, degree=-1, block_size=5.0, sh_min=-1.5, sh_max=1.5, element=-1):
        """`in.ply [actions] out.ksplat` (st_ply_ksplat_file): the element's rows stay in HBM from ingest
        to the image: (rows written, file bytes, position values clamped)"""
        acts = make_actions(actions)
        with _ply_in(path) as (fd, h):
            m, size, clamped = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            with _OutFd(out) as ofd:
                check(lib().st_ply_ksplat_file(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                               ctypes.c_int32(len(actions)), ctypes.c_int32(mode), ctypes.c_int32(degree),
                                               ctypes.c_float(block_size), ctypes.c_float(sh_min), ctypes.c_float(sh_max), ofd,
                                               ctypes.byref(m), ctypes.byref(size), ctypes.byref(clamped)))
        return m.value, size.value, clamped.value

    # ---- writeHtml (write-html.ts) -------------------------------------------------------
    def dev_base64(self, segs, out, byte0=0, nbytes=None):
        """st_dev_base64: the base64 text of bytes [byte0, byte0 + nbytes) of the stream that `segs` (at
        most four device uint8 tensors, any alignment, possibly empty) make back to back, at `out`, a
        device uint8 tensor -> the bytes written.  A tensor too small for them, a misaligned one or a
        range the kernel does not take raises ST_ERR_ARG and `out` is left untouched"""
        arr = (BytesSeg * max(len(segs), 1))(*[BytesSeg(s.data_ptr() if s.numel() else None, s.numel()) for s in segs])
        if nbytes is None:
            nbytes = sum(s.numel() for s in segs) - byte0
        size = ctypes.c_uint64()
        check(lib().st_dev_base64(self.h, arr, ctypes.c_int32(len(segs)), ctypes.c_uint64(byte0),
                                  ctypes.c_uint64(nbytes), ctypes.c_void_p(out.data_ptr()),
                                  ctypes.c_uint64(out.numel()), ctypes.byref(size)))
        return size.value

    def html_file(self, cols, actions, template, out, camera=(2, 2, -2), target=(0, 0, 0), version=None):
        """processDataTable + writeHtml of a host table (list of (name, numpy array) or a dict) into
        `out`, a path or a descriptor (st_html_file).  template: the viewer's (html, css, js), str or
        UTF-8 bytes -> (rows embedded, sh_coeffs, file bytes).  The input arrays are not changed"""
        _, ts = _host_table(cols)
        acts = make_actions(actions)
        enc = [t.encode('utf-8') if isinstance(t, str) else bytes(t) for t in template]
        m, C, size = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
        with _OutFd(out) as fd:
            check(lib().st_html_file(self.h, ctypes.byref(ts), acts, ctypes.c_int32(len(actions)), enc[0], enc[1],
                                     enc[2], _vec3(camera), _vec3(target), fd, version.encode() if version else None,
                                     ctypes.byref(m), ctypes.byref(C), ctypes.byref(size)))
        return m.value, C.value, size.value

    def ply_html_file(self, path, actions, template, out, camera=(2, 2, -2), target=(0, 0, 0), version=None,
                      element=-1):
        """the CLI's `in.ply [actions] out.html` (st_ply_html_file): the element's rows stay in HBM from
        ingest to the text: (rows embedded, sh_coeffs, file bytes)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            enc = [t.encode('utf-8') if isinstance(t, str) else bytes(t) for t in template]
            m, C, size = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
            with _OutFd(out) as ofd:
                check(lib().st_ply_html_file(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                             ctypes.c_int32(len(actions)), enc[0], enc[1], enc[2], _vec3(camera),
                                             _vec3(target), ofd, version.encode() if version else None,
                                             ctypes.byref(m), ctypes.byref(C), ctypes.byref(size)))
        return m.value, C.value, size.value

    def ply_sog_bundle(self, path, actions, iters, draws, dos_time, dos_date, element=-1):
        """readPly + processDataTable + writeSog to .sog bytes from the file (st_ply_sog_bundle):
        (archive bytes, draws used)"""
        with _ply_in(path) as (fd, h):
            acts = make_actions(actions)
            draws = np.ascontiguousarray(draws, np.float64)
            used, size = ctypes.c_uint64(), ctypes.c_uint64()
            out = ctypes.c_void_p()
            check(lib().st_ply_sog_bundle(self.h, ctypes.c_int32(fd), ctypes.byref(h), ctypes.c_int32(element), acts,
                                          ctypes.c_int32(len(actions)), ctypes.c_int32(iters), _vp(draws),
                                          ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.c_uint16(dos_time),
                                          ctypes.c_uint16(dos_date), ctypes.byref(out), ctypes.byref(size)))
        return _take(out, size), used.value

    def dev_filter_finite_t(self, cols, out_idx):
        t = make_ttable(cols)
        m = ctypes.c_uint64()
        check(lib().st_dev_filter_finite_t(self.h, ctypes.byref(t), _ptr(out_idx), ctypes.byref(m)))
        return m.value

    def dev_permute_rows_t(self, src, idx, m, dst):
        ts, td = make_ttable(src), make_ttable(dst, m)
        check(lib().st_dev_permute_rows_t(self.h, ctypes.byref(ts), _ptr(idx), ctypes.c_uint64(m), ctypes.byref(td)))

    def dev_combine(self, tables, dst):
        """tables: lists of (name, device tensor); dst: list of (name, tensor) in combine_layout order"""
        tts = [make_ttable(t) for t in tables]
        arr = (ctypes.POINTER(TTable) * len(tts))(*[ctypes.pointer(t) for t in tts])
        td = make_ttable(dst)
        check(lib().st_dev_combine(self.h, arr, ctypes.c_int32(len(tts)), ctypes.byref(td)))

    def dev_permute_rows(self, src, idx, m, dst):
        ts, td = make_table(src), make_table(dst)
        check(lib().st_dev_permute_rows(self.h, ctypes.byref(ts), _ptr(idx), ctypes.c_uint64(m), ctypes.byref(td)))

    def dev_kmeans(self, col_list, k, iters, draws, centroids, labels):
        d, n = len(col_list), len(col_list[0])
        used = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_kmeans(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(n), ctypes.c_int32(k),
                                  ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used),
                                  _ptr(centroids), _ptr(labels)))
        return used.value

    def dev_cluster1d(self, col_list, iters, draws, centroids, labels):
        n = len(col_list[0])
        used = ctypes.c_uint64(0)
        ptrs = (ctypes.c_void_p * len(col_list))(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_cluster1d(self.h, ptrs, ctypes.c_int32(len(col_list)), ctypes.c_uint64(n),
                                     ctypes.c_int32(iters), _vp(draws), ctypes.c_uint64(len(draws)),
                                     ctypes.byref(used), _ptr(centroids), _ptr(labels)))
        return used.value

    def dev_sog_sharded(self, comm, locals_, iters, draws, tex=None):
        """this rank's part of a sharded writeSog; locals_: list of dicts name -> device column (this
        rank's tables in global order); tex (rank 0): dict of device outputs as dev_sog's"""
        ts, arr = _tables_arg(locals_)
        meta = SogMeta()
        used = ctypes.c_uint64()
        out = None
        if tex is not None:
            out = SogTextures(*[(_ptr(tex[k]).value if k in tex else None) for k in
                                ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        check(lib().st_dev_sog_sharded(self.h, comm.h, arr, ctypes.c_int32(len(ts)), ctypes.c_int32(iters),
                                       _vp(draws), ctypes.c_uint64(len(draws)), ctypes.byref(used),
                                       ctypes.byref(meta) if tex is not None else None,
                                       ctypes.byref(out) if out is not None else None))
        return meta, used.value

    def dev_sog(self, cols, iters, draws, tex):
        """tex: dict of device uint8 tensors (see sog_geometry for sizes)"""
        t = make_table(cols)
        out = SogTextures(*[(tex[k].data_ptr() if k in tex else None) for k in
                            ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        meta = SogMeta()
        used = ctypes.c_uint64(0)
        check(lib().st_dev_sog(self.h, ctypes.byref(t), ctypes.c_int32(iters), _vp(draws),
                               ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.byref(meta),
                               ctypes.byref(out)))
        return meta, used.value

    def dev_sog_file(self, cols, iters, draws, tex, path, dos_time=0, dos_date=0):
        """writeSog into the file at `path` (st_dev_sog_file: the step, the archive streamed to the
        file while the SH k-means runs): (meta, draws used, file bytes)"""
        t = make_table(cols)
        out = SogTextures(*[(tex[k].data_ptr() if k in tex else None) for k in
                            ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        meta = SogMeta()
        used, size = ctypes.c_uint64(0), ctypes.c_uint64(0)
        import time
        t0 = time.perf_counter()
        # no O_TRUNC: st_dev_sog_file cuts the file to the archive's length itself, and a file
        # truncated to zero and rewritten is flushed at close on ext4 (replace-via-truncate), and
        # frees its old pages first -- 10-14 ms each for a 157 MB archive
        fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)
        t1 = time.perf_counter()
        try:
            check(lib().st_dev_sog_file(self.h, ctypes.byref(t), ctypes.c_int32(iters), _vp(draws),
                                        ctypes.c_uint64(len(draws)), ctypes.byref(used), ctypes.byref(meta),
                                        ctypes.byref(out), ctypes.c_int32(fd), ctypes.c_uint16(dos_time),
                                        ctypes.c_uint16(dos_date), ctypes.byref(size)))
        finally:
            t2 = time.perf_counter()
            os.close(fd)
            if os.environ.get('ST_DEBUG'):
                print(f'[splat_hip] dev_sog_file: open {1e3 * (t1 - t0):.1f} ms, call {1e3 * (t2 - t1):.1f} ms, '
                      f'close {1e3 * (time.perf_counter() - t2):.1f} ms', file=sys.stderr)
        return meta, used.value, size.value

    # ---- multi-GPU building blocks (device tensors; see splat_dist.py) ----------------
    def dev_minmax(self, cols):
        m = len(cols)
        lo, hi = (ctypes.c_double * m)(), (ctypes.c_double * m)()
        ptrs = (ctypes.c_void_p * m)(*[c.data_ptr() for c in cols])
        check(lib().st_dev_minmax(self.h, ptrs, ctypes.c_int32(m), ctypes.c_uint64(len(cols[0])), lo, hi))
        return list(lo), list(hi)

    def dev_kmeans_prepare(self, col_list):
        d, n = len(col_list), len(col_list[0])
        ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_kmeans_prepare(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(n)))

    def dev_kmeans_assign(self, col_list, k, centroids, labels):
        d, n = len(col_list), len(col_list[0])
        ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_kmeans_assign(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(n), ctypes.c_int32(k),
                                         _ptr(centroids), _ptr(labels)))

    def dev_kmeans_partials(self, col_list, nseg, k, labels, sums, sabs, emin, counts):
        d, n = len(col_list), len(col_list[0])
        ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_kmeans_partials(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(n), ctypes.c_int32(nseg),
                                           ctypes.c_int32(k), _ptr(labels), _ptr(sums), _ptr(sabs), _ptr(emin),
                                           _ptr(counts)))

    def dev_kmeans_seqsum(self, d, k, seg, pairs, running, emin, sabs):
        check(lib().st_dev_kmeans_seqsum(self.h, ctypes.c_int32(d), ctypes.c_int32(k), ctypes.c_int32(seg),
                                         _ptr(pairs), ctypes.c_uint32(len(pairs)), _ptr(running), _ptr(emin),
                                         _ptr(sabs)))

    def dev_kmeans_init_rows(self, draws, n, k, rows):
        """initializeCentroids over n global rows: rows (device uint32/int32, k) filled; returns draws used"""
        used = ctypes.c_uint64(0)
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        check(lib().st_dev_kmeans_init_rows(self.h, _vp(draws), ctypes.c_uint64(len(draws)), ctypes.c_uint64(n),
                                            ctypes.c_int32(k), _ptr(rows), ctypes.byref(used)))
        return used.value

    def dev_gather_rows(self, col_list, offset, rows, out):
        """out (device f32, d*k) = the rows this rank holds, bit pattern 0 elsewhere"""
        d, k = len(col_list), len(rows)
        ptrs = (ctypes.c_void_p * d)(*[c.data_ptr() for c in col_list])
        check(lib().st_dev_gather_rows(self.h, ptrs, ctypes.c_int32(d), ctypes.c_uint64(len(col_list[0])),
                                       ctypes.c_uint64(offset), _ptr(rows), ctypes.c_int32(k), _ptr(out)))

    def dev_kmeans_finish(self, d, k, sums, sabs, emin, counts, centroids, pending):
        np_ = ctypes.c_uint32(0)
        check(lib().st_dev_kmeans_finish(self.h, ctypes.c_int32(d), ctypes.c_int32(k), _ptr(sums), _ptr(sabs),
                                         _ptr(emin), _ptr(counts), _ptr(centroids), _ptr(pending), ctypes.byref(np_)))
        return np_.value

    def dev_kmeans_average(self, d, k, pairs, running, counts, centroids):
        check(lib().st_dev_kmeans_average(self.h, ctypes.c_int32(d), ctypes.c_int32(k), _ptr(pairs),
                                          ctypes.c_uint32(len(pairs)), _ptr(running), _ptr(counts), _ptr(centroids)))

    def dev_cluster1d_codebook(self, centroids, labels, codebook, labels8):
        check(lib().st_dev_cluster1d_codebook(self.h, _ptr(centroids), _ptr(labels), ctypes.c_uint64(len(labels)),
                                              _ptr(codebook), _ptr(labels8)))

    def dev_sog_scatter(self, cols, pos, lo, hi, scale_labels, color_labels, shn_labels, tex):
        t = make_table(cols)
        out = SogTextures(*[(tex[k].data_ptr() if tex.get(k) is not None else None) for k in
                            ('means_l', 'means_u', 'quats', 'scales', 'sh0', 'shN_centroids', 'shN_labels')])
        meta = SogMeta()
        check(lib().st_dev_sog_scatter(self.h, ctypes.byref(t), _ptr(pos), (ctypes.c_double * 3)(*lo),
                                       (ctypes.c_double * 3)(*hi), _ptr(scale_labels), _ptr(color_labels),
                                       _ptr(shn_labels), ctypes.byref(meta), ctypes.byref(out)))
        return meta

    def dev_sog_shn_centroids(self, codebook_labels, sh_coeffs, palette, out):
        check(lib().st_dev_sog_shn_centroids(self.h, _ptr(codebook_labels), ctypes.c_int32(sh_coeffs),
                                             ctypes.c_int32(palette), _ptr(out)))
