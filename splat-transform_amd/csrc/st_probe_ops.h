// st_probe_ops.h -- the scalar ops of st_dev_probe (include/st_abi.h, "st_dev_probe: a test hook"):
// one expression per op over st_jsmath.h's functions and the bare f64 operations the kernels use
// beside them.  st_probe.hip evaluates it on the device, tests/native/jsmath_cpu_check.cpp on the
// host; both are built with -ffp-contract=off.
#pragma once

#include "../../include/st_abi.h"
#include "st_jsmath.h"

namespace st {
namespace probe {

// bytes of one output element
__host__ __device__ inline int out_size(int op) {
    if (op == ST_PROBE_TO_UINT8) return 1;
    if (op == ST_PROBE_TO_INT32 || op == ST_PROBE_F32_STORE || op == ST_PROBE_F32_CAST) return 4;
    return 8;
}
__host__ __device__ inline bool two_inputs(int op) { return op >= ST_PROBE_DIV && op <= ST_PROBE_MAX; }
__host__ __device__ inline bool is_scalar(int op) { return op >= ST_PROBE_EXP && op <= ST_PROBE_MAX; }

// the result's bits, in the low out_size(op) bytes
__host__ __device__ inline uint64_t scalar(int op, double a, double b, double s) {
    double r = 0;
    switch (op) {
        case ST_PROBE_EXP: r = js::exp(a); break;
        case ST_PROBE_LOG: r = js::log(a); break;
        case ST_PROBE_SIGMOID: r = js::sigmoid(a); break;
        case ST_PROBE_LOG_TRANSFORM: r = js::log_transform(a); break;
        case ST_PROBE_LOG1ABS: r = js::log(__builtin_fabs(a) + 1); break;
        case ST_PROBE_LOGEXP: r = js::log(js::x86_nan(js::exp(a) * s, a != a || s != s)); break;
        case ST_PROBE_SQRT: r = __builtin_sqrt(a); break;
        case ST_PROBE_ROUND: r = __builtin_floor(a + 0.5); break;
        case ST_PROBE_TO_INT32: return (uint32_t)js::to_int32(a);
        case ST_PROBE_TO_UINT8: return js::to_uint8(a);
        case ST_PROBE_F32_STORE: return __builtin_bit_cast(uint32_t, js::f32_store(a));
        case ST_PROBE_F32_CAST: return __builtin_bit_cast(uint32_t, (float)a);
        case ST_PROBE_SIGN: r = js::sign_(a); break;
        case ST_PROBE_DIV: r = a / b; break;
        case ST_PROBE_MIN: r = js::min_(a, b); break;
        case ST_PROBE_MAX: r = js::max_(a, b); break;
        default: break;
    }
    return __builtin_bit_cast(uint64_t, r);
}

}  // namespace probe
}  // namespace st
