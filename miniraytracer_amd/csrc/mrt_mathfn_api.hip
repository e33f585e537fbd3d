// mrt_mathfn_api.hip -- the numerics contract's transcendentals (include/mrt_mathfn.h) as array calls
// behind the C-ABI (include/mrt.h "the contract's transcendentals"): mrt_mathfn / mrt_mathfn_d on the
// host, mrt_mathfn_device / mrt_mathfn_d_device on the GPU.  Both sides call the header's functions
// exactly as it defines them, under the exact contract's flags (no contraction, IEEE division and
// square root), in a translation unit of its own so no other object changes with it.  What callers of
// the pano and surface-probe formulas get is those formulas' functions; what the tests get is the
// device build of the header beside its host build, function by function and core by core.
//
// One thread per element, no LDS, no atomics; `which` is uniform, so the switch is a scalar branch.
#include <hip/hip_runtime.h>

#include <math.h>  // (not <cmath>: the header's host side names ::signbit)
#include <cstdint>
#include <cstring>
#include <string>

#include "mrt_internal.h"
#include "../../include/mrt_mathfn.h"

static __host__ __device__ inline float mathfn_f(uint32_t which, float a, float b) {
    switch (which) {
    case MRT_FN_SIN: return mrt_sinf(a);
    case MRT_FN_COS: return mrt_cosf(a);
    case MRT_FN_TAN: return mrt_tanf(a);
    case MRT_FN_LOG: return mrt_logf(a);
    case MRT_FN_LOG10: return mrt_log10f(a);
    case MRT_FN_ASIN: return mrt_asinf(a);
    case MRT_FN_EXP: return mrt_expf(a);
    case MRT_FN_POW5: return mrt_pow5f(a);
    case MRT_FN_ATAN2: return mrt_atan2f(a, b);
    default: return mrt_powf(a, b);
    }
}

// the double cores: out2 is written by MRT_FND_SINCOS only
static __host__ __device__ inline void mathfn_d(uint32_t which, double a, double b, double* out, double* out2) {
    switch (which) {
    case MRT_FND_SINCOS: mrt_sincos_d(a, out, out2); break;
    case MRT_FND_LOG: *out = mrt_log_d(a); break;
    case MRT_FND_EXP: *out = mrt_exp_d(a); break;
    default: *out = mrt_atan2_d(a, b); break;
    }
}

__global__ void __launch_bounds__(256) mrt_mathfn_kernel(uint32_t which, uint32_t n, const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = mathfn_f(which, a[i], which >= MRT_FN_ATAN2 ? b[i] : 0.0f);
}

__global__ void __launch_bounds__(256) mrt_mathfn_d_kernel(uint32_t which, uint32_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                          double* __restrict__ out, double* __restrict__ out2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r, r2 = 0.0;
    mathfn_d(which, a[i], which == MRT_FND_ATAN2 ? b[i] : 0.0, &r, &r2);
    out[i] = r;
    if (which == MRT_FND_SINCOS) out2[i] = r2;
}

static mrt_status check_f(const char* who, uint32_t which, const void* a, const void* b, const void* out) {
    if (which > MRT_FN_POW) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": unknown function").c_str());
    if (!a || !out || (which >= MRT_FN_ATAN2 && !b)) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    return MRT_OK;
}

static mrt_status check_d(const char* who, uint32_t which, const void* a, const void* b, const void* out, const void* out2) {
    if (which > MRT_FND_ATAN2) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": unknown function").c_str());
    if (!a || !out || (which == MRT_FND_ATAN2 && !b) || (which == MRT_FND_SINCOS && !out2))
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    return MRT_OK;
}

extern "C" mrt_status mrt_mathfn(uint32_t which, uint32_t n, const float* a, const float* b, float* out) {
    if (mrt_status st = check_f("mrt_mathfn", which, a, b, out)) return st;
    for (uint32_t i = 0; i < n; i++) out[i] = mathfn_f(which, a[i], which >= MRT_FN_ATAN2 ? b[i] : 0.0f);
    return MRT_OK;
}

extern "C" mrt_status mrt_mathfn_d(uint32_t which, uint32_t n, const double* a, const double* b, double* out, double* out2) {
    if (mrt_status st = check_d("mrt_mathfn_d", which, a, b, out, out2)) return st;
    for (uint32_t i = 0; i < n; i++) {
        double r, r2 = 0.0;
        mathfn_d(which, a[i], which == MRT_FND_ATAN2 ? b[i] : 0.0, &r, &r2);
        out[i] = r;
        if (which == MRT_FND_SINCOS) out2[i] = r2;
    }
    return MRT_OK;
}

static mrt_status launched(void) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
}

extern "C" mrt_status mrt_mathfn_device(uint32_t which, uint32_t n, const float* d_a, const float* d_b, float* d_out, void* stream) {
    if (mrt_status st = check_f("mrt_mathfn_device", which, d_a, d_b, d_out)) return st;
    if (n == 0) return MRT_OK;
    hipLaunchKernelGGL(mrt_mathfn_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, which, n, d_a, d_b, d_out);
    return launched();
}

extern "C" mrt_status mrt_mathfn_d_device(uint32_t which, uint32_t n, const double* d_a, const double* d_b, double* d_out, double* d_out2,
                                          void* stream) {
    if (mrt_status st = check_d("mrt_mathfn_d_device", which, d_a, d_b, d_out, d_out2)) return st;
    if (n == 0) return MRT_OK;
    hipLaunchKernelGGL(mrt_mathfn_d_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, which, n, d_a, d_b, d_out, d_out2);
    return launched();
}
