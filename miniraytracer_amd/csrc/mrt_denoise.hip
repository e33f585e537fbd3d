// mrt_denoise.hip -- the edge-avoiding a-trous filter behind the C-ABI (include/mrt.h "feature
// buffers and denoise"): mrt_denoise on the host, mrt_denoise_device on the GPU, both running the
// per-pixel function of include/mrt_denoise.h (no contraction, the numerics contract's exp / pow):
// the same bits.
//
// mrt_atrous_kernel: one thread per pixel on 64 x 4 workgroups -- a wave is 64 pixels of one row,
// so each tap of a pass is one contiguous 1 KiB float4 load per wave -- and one launch per pass.
// No atomics, no LDS: the three frames of a 500 x 500 image are 12 MB and stay in cache between the
// taps.  Passes alternate between d_tmp and d_out so that the last one lands in d_out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <thread>
#include <vector>
#include <cstring>

#include "mrt_internal.h"
#include "../../include/mrt_denoise.h"

static constexpr uint32_t kAtrousWgX = 64, kAtrousWgY = 4;
__global__ void __launch_bounds__(kAtrousWgX * kAtrousWgY) mrt_atrous_kernel(mrt_atrous_pass ps, const mrt_f4* __restrict__ rgb,
                                                                           const mrt_f4* __restrict__ normal, const mrt_f4* __restrict__ albedo,
                                                                           mrt_f4* __restrict__ out) {
    const uint32_t x = blockIdx.x * kAtrousWgX + threadIdx.x, y = blockIdx.y * kAtrousWgY + threadIdx.y;
    if (x >= ps.width || y >= ps.height) return;
    out[(size_t)y * ps.width + x] = mrt_atrous_pixel(&ps, rgb, normal, albedo, x, y);
}

extern "C" void mrt_default_denoise_params(mrt_denoise_params* p) {
    if (!p) return;
    // chosen on the Cornell box at 16 spp, 128 x 128, against the reference at 1024 spp
    p->iterations = 3;
    p->sigma_color = 8.0f;
    p->sigma_normal = 32.0f;
    p->sigma_albedo = 0.3f;
    p->sigma_depth = 0.02f;
}

static mrt_status check_denoise(const char* who, const void* a, const void* b, const void* c, const void* o, uint32_t w, uint32_t h,
                                const mrt_denoise_params* p) {
    if (!a || !b || !c || !o || !p) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    if ((uint64_t)w * h == 0) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": empty image").c_str());
    if (w > (1u << 16) || h > (1u << 16)) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": width / height above 65536 pixels").c_str());
    if (p->iterations > 16u || !(p->sigma_color > 0.0f) || !(p->sigma_albedo > 0.0f) || !(p->sigma_depth > 0.0f) || !(p->sigma_normal >= 0.0f))
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": iterations <= 16, sigmas > 0 (sigma_normal >= 0)").c_str());
    return MRT_OK;
}

extern "C" mrt_status mrt_denoise(const float* rgb, const float* normal, const float* albedo, uint32_t width, uint32_t height,
                                  const mrt_denoise_params* p, float* rgb_out) {
    if (mrt_status st = check_denoise("mrt_denoise", rgb, normal, albedo, rgb_out, width, height, p)) return st;
    const size_t n = (size_t)width * height;
    if (p->iterations == 0) {
        if (rgb_out != rgb) memmove(rgb_out, rgb, n * 16);
        return MRT_OK;
    }
    // the passes alternate between two scratch frames (rgb_out may be the input itself)
    std::vector<float> buf[2];
    try {
        buf[0].resize(n * 4);
        if (p->iterations > 1) buf[1].resize(n * 4);
    } catch (const std::bad_alloc&) {
        return mrt_internal_fail(MRT_ERR_OOM, "mrt_denoise: out of memory");
    }
    const uint32_t workers = (uint32_t)std::min<size_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), (n + 4095) / 4096);
    const float* src = rgb;
    for (uint32_t i = 0; i < p->iterations; i++) {
        mrt_atrous_pass ps;
        mrt_atrous_pass_setup(width, height, i, p->sigma_color, p->sigma_normal, p->sigma_albedo, p->sigma_depth, &ps);
        float* dst = buf[i & 1u].data();
        auto rows = [&](uint32_t k) {  // worker k of `workers`: every workers-th row
            for (uint32_t y = k; y < height; y += workers)
                for (uint32_t x = 0; x < width; x++) ((mrt_f4*)dst)[(size_t)y * width + x] = mrt_atrous_pixel(&ps, (const mrt_f4*)src, (const mrt_f4*)normal, (const mrt_f4*)albedo, x, y);
        };
        std::vector<std::thread> pool;
        for (uint32_t k = 1; k < workers; k++) pool.emplace_back(rows, k);
        rows(0u);
        for (std::thread& t : pool) t.join();
        src = dst;
    }
    memcpy(rgb_out, src, n * 16);
    return MRT_OK;
}

extern "C" mrt_status mrt_denoise_device(const float* d_rgb, const float* d_normal, const float* d_albedo, uint32_t width, uint32_t height,
                                         const mrt_denoise_params* p, float* d_out, float* d_tmp, void* stream) {
    if (mrt_status st = check_denoise("mrt_denoise_device", d_rgb, d_normal, d_albedo, d_out, width, height, p)) return st;
    if (!d_tmp) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_denoise_device: null");
    if (d_out == d_rgb || d_tmp == d_rgb || d_out == d_tmp)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_denoise_device: d_rgb, d_out and d_tmp must be three frames");
    hipStream_t q = (hipStream_t)stream;
    const size_t n = (size_t)width * height;
    auto hip_fail = [](hipError_t e) { return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e)); };
    if (p->iterations == 0) {
        const hipError_t e = hipMemcpyAsync(d_out, d_rgb, n * 16, hipMemcpyDeviceToDevice, q);
        return e == hipSuccess ? MRT_OK : hip_fail(e);
    }
    const dim3 grid((width + kAtrousWgX - 1u) / kAtrousWgX, (height + kAtrousWgY - 1u) / kAtrousWgY);
    const float* src = d_rgb;
    for (uint32_t i = 0; i < p->iterations; i++) {
        mrt_atrous_pass ps;
        mrt_atrous_pass_setup(width, height, i, p->sigma_color, p->sigma_normal, p->sigma_albedo, p->sigma_depth, &ps);
        // the last pass writes d_out, the one before it d_tmp, and so on back
        float* dst = ((p->iterations - 1u - i) & 1u) ? d_tmp : d_out;
        hipLaunchKernelGGL(mrt_atrous_kernel, grid, dim3(kAtrousWgX, kAtrousWgY), 0, q, ps, (const mrt_f4*)src, (const mrt_f4*)d_normal,
                           (const mrt_f4*)d_albedo, (mrt_f4*)dst);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e);
        src = dst;
    }
    return MRT_OK;
}
