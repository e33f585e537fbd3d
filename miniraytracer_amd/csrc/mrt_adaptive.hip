// mrt_adaptive.hip -- per-pixel sample moments behind the C-ABI (include/mrt.h "sample moments and
// the adaptive render"): mrt_moments on the host, mrt_moments_device on the GPU, both running the
// functions of include/mrt_adaptive.h (float32, no contraction): the same bits.  Also what the
// adaptive render's drivers share: the argument check, the refinement decision (compiled here, once,
// for both backends) and the merge kernel.
//
// mrt_moments_kernel: one lane per local pixel of a radiance chunk in the render's workspace layout
// ([s][local pixel] float3, so a wave's 12-byte loads of one sample are 768 contiguous bytes),
// MRT_MOMENTS_DEPTH samples in flight before the dependent adds (as mrt_fold_kernel's FOLD_DEPTH: the
// sums are sequential per pixel, so the kernel is bound by load latency).  One lane owns one slot of
// `moments` -- loaded and stored as one 16-byte access -- so there are no atomics and no LDS.
// mrt_merge_kernel: one lane per pixel of a refinement pass, C[slot] = merge(C[slot], c[lane]).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "mrt_moments.h"
#include "../../include/mrt_adaptive.h"

#ifndef MRT_MOMENTS_DEPTH
#define MRT_MOMENTS_DEPTH 16
#endif
__global__ void __launch_bounds__(256) mrt_moments_kernel(const float* __restrict__ rad, uint32_t npix, uint32_t ns,
                                                         const uint32_t* __restrict__ slots, mrt_m4* __restrict__ moments) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    const uint32_t slot = slots ? slots[lp] : lp;
    mrt_m4 m = moments[slot];
    const float* q = rad + (size_t)lp * 3;
    const size_t stride = (size_t)npix * 3;
    uint32_t s = 0;
    for (; s + MRT_MOMENTS_DEPTH <= ns; s += MRT_MOMENTS_DEPTH) {
        float v[MRT_MOMENTS_DEPTH][3];
#pragma unroll
        for (int k = 0; k < MRT_MOMENTS_DEPTH; k++) {
            const float* e = q + (size_t)(s + k) * stride;
            v[k][0] = __builtin_nontemporal_load(e);
            v[k][1] = __builtin_nontemporal_load(e + 1);
            v[k][2] = __builtin_nontemporal_load(e + 2);
        }
#pragma unroll
        for (int k = 0; k < MRT_MOMENTS_DEPTH; k++) m = mrt_moments_add(m, v[k][0], v[k][1], v[k][2]);
    }
    for (; s < ns; s++) {
        const float* e = q + (size_t)s * stride;
        m = mrt_moments_add(m, e[0], e[1], e[2]);
    }
    moments[slot] = m;
}

__global__ void __launch_bounds__(256) mrt_merge_kernel(const mrt_m4* __restrict__ c, uint32_t n, const uint32_t* __restrict__ slots,
                                                       mrt_m4* __restrict__ C, float N, float nsf) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t slot = slots[j];
    const mrt_m4 a = c[j];
    mrt_m4 r = C[slot];
    r.x = mrt_adaptive_merge(r.x, a.x, N, nsf);
    r.y = mrt_adaptive_merge(r.y, a.y, N, nsf);
    r.z = mrt_adaptive_merge(r.z, a.z, N, nsf);
    C[slot] = r;
}

static mrt_status hip_fail(hipError_t e) { return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e)); }

mrt_status mrt_internal_moments_enqueue(const float* d_rad, uint32_t n_pixels, uint32_t n_samples, const uint32_t* d_slots, float* d_moments,
                                        void* stream) {
    if ((uint64_t)n_pixels * n_samples == 0) return MRT_OK;
    hipLaunchKernelGGL(mrt_moments_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d_rad, n_pixels, n_samples, d_slots,
                       (mrt_m4*)d_moments);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : hip_fail(e);
}

mrt_status mrt_internal_merge_enqueue(const float* d_c, uint32_t n, const uint32_t* d_slots, float* d_C, float N, float nsf, void* stream) {
    if (n == 0) return MRT_OK;
    hipLaunchKernelGGL(mrt_merge_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, (const mrt_m4*)d_c, n, d_slots, (mrt_m4*)d_C, N,
                       nsf);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : hip_fail(e);
}

static mrt_status check_moments(const char* who, const void* rgb, uint32_t n_pixels, uint32_t n_samples, const void* moments) {
    if (!rgb || !moments) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    if ((uint64_t)n_pixels * n_samples == 0) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": no samples").c_str());
    return MRT_OK;
}

extern "C" mrt_status mrt_moments(const float* path_rgb, uint32_t n_pixels, uint32_t n_samples, const uint32_t* slots, float* moments) {
    if (mrt_status st = check_moments("mrt_moments", path_rgb, n_pixels, n_samples, moments)) return st;
    mrt_m4* const M = (mrt_m4*)moments;
    const size_t stride = (size_t)n_pixels * 3;
    for (uint32_t lp = 0; lp < n_pixels; lp++) {
        const uint32_t slot = slots ? slots[lp] : lp;
        mrt_m4 m = M[slot];
        const float* q = path_rgb + (size_t)lp * 3;
        for (uint32_t s = 0; s < n_samples; s++) {
            const float* e = q + (size_t)s * stride;
            m = mrt_moments_add(m, e[0], e[1], e[2]);
        }
        M[slot] = m;
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_moments_device(const float* d_path_rgb, uint32_t n_pixels, uint32_t n_samples, const uint32_t* d_slots,
                                         float* d_moments, void* stream) {
    if (mrt_status st = check_moments("mrt_moments_device", d_path_rgb, n_pixels, n_samples, d_moments)) return st;
    if ((uintptr_t)d_moments & 15u) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_moments_device: d_moments must be 16-byte aligned");
    return mrt_internal_moments_enqueue(d_path_rgb, n_pixels, n_samples, d_slots, d_moments, stream);
}

extern "C" mrt_status mrt_moments_decide(const float* moments, uint32_t n, float atol, float rtol, uint8_t* refine_out, float* se_out) {
    if (!moments || (!refine_out && !se_out)) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_moments_decide: null");
    const mrt_m4* const M = (const mrt_m4*)moments;
    for (uint32_t i = 0; i < n; i++) {
        if (refine_out) refine_out[i] = mrt_moments_refine(M[i], atol, rtol) ? 1u : 0u;
        if (se_out) se_out[i] = mrt_moments_se(M[i]);
    }
    return MRT_OK;
}

extern "C" void mrt_default_adaptive_params(mrt_adaptive_params* p) {
    if (!p) return;
    // chosen on the Cornell box at a 16-spp base, 128 x 128, against the reference at 1024 spp
    p->max_passes = 2;
    p->atol = 0.03f;
    p->rtol = 0.0f;
}

mrt_status mrt_internal_adaptive_check(const void* scene, const mrt_render_desc* d, const mrt_adaptive_params* p, const void* rgb_out) {
    if (!scene || !d || !p || !rgb_out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: null");
    if (p->max_passes > 4u || !(p->atol >= 0.0f) || !(p->rtol >= 0.0f) || !std::isfinite(p->atol) || !std::isfinite(p->rtol))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: max_passes <= 4, atol and rtol >= 0 and finite");
    if (d->width == 0 || d->height == 0 || d->sqrt_samples == 0 || (d->world && d->rank >= d->world))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: bad desc");
    if (d->mode != 0) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: mode 0 only");
    if (d->flags & ~MRT_RF_FAST) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: flags other than MRT_RF_FAST");
    // the finest pass's grid: (sqrt_samples * 2^max_passes)^2 samples in 32 bits
    if (((uint64_t)d->sqrt_samples << p->max_passes) > 0xFFFFull)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_adaptive: sqrt_samples * 2^max_passes above 65535");
    return mrt_internal_check_pixels(d);
}

std::vector<uint32_t> mrt_internal_refine_slots(const float* moments, uint32_t n, float atol, float rtol) {
    std::vector<uint32_t> out;
    const mrt_m4* const M = (const mrt_m4*)moments;
    for (uint32_t i = 0; i < n; i++)
        if (mrt_moments_refine(M[i], atol, rtol)) out.push_back(i);
    return out;
}
