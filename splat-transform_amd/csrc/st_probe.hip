// st_probe.hip -- st_dev_probe, a test hook (include/st_abi.h): st_jsmath.h's scalar rules in the
// library's normal device compile, and thin calls of st_prims.hip's primitives.  Nothing in the
// library calls it.
#include "st_internal.h"
#include "st_probe_ops.h"

namespace st {

namespace {

__global__ __launch_bounds__(256) void k_probe_scalar(int op, const double *__restrict__ a, const double *__restrict__ b,
                                                      double s, uint64_t n, void *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = probe::scalar(op, a[i], b ? b[i] : 0.0, s);
    switch (probe::out_size(op)) {
        case 1: static_cast<uint8_t *>(out)[i] = (uint8_t)r; break;
        case 4: static_cast<uint32_t *>(out)[i] = (uint32_t)r; break;
        default: static_cast<uint64_t *>(out)[i] = r; break;
    }
}

bool aligned(const void *p, size_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

// a pointer the op reads or writes n elements through
void need(const void *p, uint64_t n, size_t elem, const char *what) {
    ST_REQUIRE(p || n == 0, ST_ERR_ARG, std::string("probe: NULL ") + what);
    ST_REQUIRE(aligned(p, elem), ST_ERR_ARG, std::string("probe: ") + what + " is not aligned to its element type");
}

void probe_dev(st_ctx *c, int op, st_probe_args *a) {
    const uint64_t n = a->n;
    ST_REQUIRE(n < (1ull << 32), ST_ERR_ARG, "probe: n must be < 2^32");
    uint32_t *in0 = static_cast<uint32_t *>(a->in0), *in1 = static_cast<uint32_t *>(a->in1);
    uint32_t *out0 = static_cast<uint32_t *>(a->out0), *out1 = static_cast<uint32_t *>(a->out1);
    const int b0 = a->begin_bit, b1 = a->end_bit;
    const bool sort = op >= ST_PROBE_SORT_U32 && op <= ST_PROBE_SORT_U64;
    if (sort) {
        const int width = op == ST_PROBE_SORT_U64 ? 64 : 32;
        ST_REQUIRE(0 <= b0 && b0 <= b1 && b1 <= width, ST_ERR_ARG, "probe: bit range outside the key");
    }
    if (probe::is_scalar(op)) {
        need(a->in0, n, 8, "in0");
        if (probe::two_inputs(op)) need(a->in1, n, 8, "in1");
        need(a->out0, n, probe::out_size(op), "out0");
        if (n) {
            hipLaunchKernelGGL(k_probe_scalar, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, op,
                               static_cast<const double *>(a->in0),
                               probe::two_inputs(op) ? static_cast<const double *>(a->in1) : nullptr, a->s, n, a->out0);
            ST_LAUNCH_CHECK();
        }
    } else if (op == ST_PROBE_SCAN) {
        need(in0, n, 4, "in0");
        need(out0, n, 4, "out0");
        ST_REQUIRE(aligned(a->aux, 4), ST_ERR_ARG, "probe: aux is not aligned to its element type");
        scan_u32(c, in0, out0, n, static_cast<uint32_t *>(a->aux));
    } else if (op == ST_PROBE_SORT_U32) {
        need(out0, n, 4, "out0");
        need(out1, n, 4, "out1");
        radix_sort_u32(c, out0, out1, n, b0, b1, "probe.sort");
    } else if (op == ST_PROBE_SORT_FROM || op == ST_PROBE_SORT_IOTA) {
        need(in0, n, 4, "in0");
        if (op == ST_PROBE_SORT_FROM) ST_REQUIRE(aligned(in1, 4), ST_ERR_ARG, "probe: in1 is not aligned to its element type");
        need(out0, n, 4, "out0");
        need(out1, n, 4, "out1");
        if (op == ST_PROBE_SORT_FROM) radix_sort_u32_from(c, in0, in1, n, b0, b1, out0, out1, nullptr, "probe.sort");
        else radix_sort_u32_iota(c, in0, n, b0, b1, out0, out1, "probe.sort");
    } else if (op == ST_PROBE_SORT_SWAP) {
        need(in0, n, 4, "in0");
        need(in1, n, 4, "in1");
        need(out0, n, 4, "out0");
        need(out1, n, 4, "out1");
        uint32_t *rk = nullptr, *rv = nullptr;
        radix_sort_u32_inplace_or_swap(c, in0, in1, n, b0, b1, "probe.sort", &rk, &rv);
        a->result = rk == in0 && rv == in1;
        if (n && rk != out0) ST_HIP(hipMemcpyAsync(out0, rk, n * 4, hipMemcpyDeviceToDevice, c->stream));
        if (n && rv != out1) ST_HIP(hipMemcpyAsync(out1, rv, n * 4, hipMemcpyDeviceToDevice, c->stream));
    } else if (op == ST_PROBE_SORT_U64) {
        need(out0, n, 8, "out0");
        need(out1, n, 4, "out1");
        radix_sort_u64(c, static_cast<uint64_t *>(a->out0), out1, n, b0, b1, "probe.sort");
    } else if (op == ST_PROBE_MINMAX) {
        ST_REQUIRE(a->ncols >= 1 && a->ncols <= 64, ST_ERR_ARG, "probe: 1..64 columns");
        ST_REQUIRE(a->cols && out0 && aligned(out0, 4), ST_ERR_ARG, "probe: bad cols or out0");
        for (int i = 0; i < a->ncols; ++i) need(a->cols[i], n, 4, "column");
        minmax_keys_dev(c, a->cols, a->ncols, n, out0);
    } else if (op == ST_PROBE_IOTA) {
        need(out0, n, 4, "out0");
        iota_u32(c, out0, n);
    } else {
        ST_REQUIRE(false, ST_ERR_ARG, "probe: unknown op");
    }
    ST_HIP(hipStreamSynchronize(c->stream));
}

}  // namespace

}  // namespace st

using namespace st;

extern "C" int st_dev_probe(st_ctx *c, int32_t op, st_probe_args *args) {
    return guard([&] {
        ST_REQUIRE(c && args, ST_ERR_ARG, "NULL argument");
        use_device(c);
        probe_dev(c, op, args);
    });
}
