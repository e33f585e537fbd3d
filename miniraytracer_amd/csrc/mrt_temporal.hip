// mrt_temporal.hip -- temporal reprojection behind the C-ABI (include/mrt.h "camera and temporal
// accumulation"): mrt_reproject on the host, mrt_reproject_device on the GPU, both running the
// per-pixel function of include/mrt_temporal.h (no contraction): the same bits.  Also the one-wave
// kernel behind mrt_scene_set_camera_device (mrt_render.hip reaches the scene struct and calls
// mrt_internal_camera_store).
//
// mrt_reproject_kernel: one thread per pixel on 64 x 4 workgroups, as mrt_atrous_kernel -- a wave is
// 64 pixels of one row, so the current frame's loads are contiguous 1 KiB float4 loads per wave and,
// under small camera motion, neighbouring lanes' taps are neighbouring pixels of the previous frame.
// Every access is a whole 16-byte pixel.  No LDS, no atomics; both cameras and the setup struct are
// kernel arguments (scalar registers).  A lane without history stores its colour and leaves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mrt_internal.h"
#include "../../include/mrt_temporal.h"

// MRT_TEMPORAL_HOST_ONLY (`make temporal-check`: the host forms under sanitizers, no code object to
// link): the kernels and the entry points that launch them are left out
#ifndef MRT_TEMPORAL_HOST_ONLY
static constexpr uint32_t kReprojWgX = 64, kReprojWgY = 4;
__global__ void __launch_bounds__(kReprojWgX * kReprojWgY)
    mrt_reproject_kernel(mrt_reproject_setup rs, mrt_camera cam, mrt_camera pcam, const mrt_f4* __restrict__ rgb, const mrt_f4* __restrict__ normal,
                         const mrt_f4* __restrict__ albedo, const mrt_f4* __restrict__ hist, const mrt_f4* __restrict__ pnormal,
                         const mrt_f4* __restrict__ palbedo, mrt_f4* __restrict__ out) {
    const uint32_t x = blockIdx.x * kReprojWgX + threadIdx.x, y = blockIdx.y * kReprojWgY + threadIdx.y;
    if (x >= rs.width || y >= rs.height) return;
    out[(size_t)y * rs.width + x] = mrt_reproject_pixel(&rs, &cam, &pcam, rgb, normal, albedo, hist, pnormal, palbedo, x, y);
}

// the camera record of an uploaded scene, replaced in stream order: the new camera arrives as the
// kernel argument and lane 0 of the one wave stores its 128 bytes with ordinary vector stores: to
// the record the path kernels read at each path start (16-byte aligned: eight float4 stores) and,
// word by word, to the camera inside the uploaded DScene (4-byte aligned there).  A kernel boundary
// orders the later kernels' loads after these stores.
struct __attribute__((aligned(16))) CamRecord {
    float4 v[sizeof(mrt_camera) / 16];
};
static_assert(sizeof(mrt_camera) == 128 && sizeof(CamRecord) == sizeof(mrt_camera), "mrt_camera is eight float4");
__global__ void __launch_bounds__(64) mrt_camera_store_kernel(CamRecord cam, CamRecord* __restrict__ rec, float* __restrict__ words) {
    if (threadIdx.x != 0) return;
    *rec = cam;
    if (words)
        for (uint32_t i = 0; i < sizeof(mrt_camera) / 16; i++) {
            words[4 * i + 0] = cam.v[i].x;
            words[4 * i + 1] = cam.v[i].y;
            words[4 * i + 2] = cam.v[i].z;
            words[4 * i + 3] = cam.v[i].w;
        }
}

mrt_status mrt_internal_camera_store(const mrt_camera* cam, void* d_record, void* d_words, void* stream) {
    if (!cam || !d_record || ((uintptr_t)d_record & 15u) || ((uintptr_t)d_words & 3u))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_internal_camera_store: null or misaligned");
    CamRecord rec;
    memcpy(&rec, cam, sizeof rec);
    hipLaunchKernelGGL(mrt_camera_store_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rec, (CamRecord*)d_record, (float*)d_words);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
}
#endif

extern "C" void mrt_default_temporal_params(mrt_temporal_params* p) {
    if (!p) return;
    // the CPU prototype's values; measured again on the Cornell orbit of tests/test_temporal_host.py
    p->max_history = 32.0f;
    p->normal_min = 0.9f;
    p->depth_tol = 0.02f;
    p->albedo_tol = 0.1f;
    p->min_weight = 0.25f;
}

static bool camera_finite(const mrt_camera* c) {
    const float* f = (const float*)c;
    for (size_t i = 0; i < sizeof(mrt_camera) / 4; i++)
        if (!std::isfinite(f[i])) return false;
    return true;
}

static mrt_status check_reproject(const char* who, const void* rgb, const void* normal, const void* albedo, const mrt_camera* cam, const void* hist,
                                  const void* pnormal, const void* palbedo, const mrt_camera* pcam, uint32_t w, uint32_t h,
                                  const mrt_temporal_params* p, const void* out) {
    const std::string W(who);
    if (!rgb || !normal || !albedo || !cam || !p || !out) return mrt_internal_fail(MRT_ERR_INVALID, (W + ": null").c_str());
    if (hist && (!pnormal || !palbedo || !pcam)) return mrt_internal_fail(MRT_ERR_INVALID, (W + ": a history frame needs its feature buffers and camera").c_str());
    if ((uint64_t)w * h == 0) return mrt_internal_fail(MRT_ERR_INVALID, (W + ": empty image").c_str());
    if (w > (1u << 16) || h > (1u << 16)) return mrt_internal_fail(MRT_ERR_INVALID, (W + ": width / height above 65536 pixels").c_str());
    if (!(p->max_history >= 1.0f) || !std::isfinite(p->max_history) || !(p->normal_min >= -1.0f && p->normal_min <= 1.0f) ||
        !(p->depth_tol > 0.0f) || !std::isfinite(p->depth_tol) || !(p->albedo_tol > 0.0f) || !std::isfinite(p->albedo_tol) ||
        !(p->min_weight > 0.0f && p->min_weight <= 1.0f))
        return mrt_internal_fail(MRT_ERR_INVALID,
                                 (W + ": max_history >= 1, normal_min in [-1, 1], depth_tol and albedo_tol > 0, min_weight in (0, 1]").c_str());
    if (!camera_finite(cam) || (hist && !camera_finite(pcam))) return mrt_internal_fail(MRT_ERR_INVALID, (W + ": a camera with a non-finite field").c_str());
    // the new history frame is a frame of its own: taps read neighbours of the old one
    if (out == rgb || out == normal || out == albedo || (hist && (out == hist || out == pnormal || out == palbedo)))
        return mrt_internal_fail(MRT_ERR_INVALID, (W + ": the output frame must not be one of the inputs").c_str());
    return MRT_OK;
}

static mrt_reproject_setup make_setup(uint32_t w, uint32_t h, const mrt_camera* pcam, const mrt_temporal_params* p) {
    mrt_reproject_setup rs;
    mrt_reproject_setup_make(w, h, pcam, p->max_history, p->normal_min, p->depth_tol, p->albedo_tol, p->min_weight, &rs);
    return rs;
}

extern "C" mrt_status mrt_reproject(const float* rgb, const float* normal, const float* albedo, const mrt_camera* cam, const float* hist,
                                    const float* prev_normal, const float* prev_albedo, const mrt_camera* prev_cam, uint32_t width, uint32_t height,
                                    const mrt_temporal_params* p, float* hist_out) {
    if (mrt_status st = check_reproject("mrt_reproject", rgb, normal, albedo, cam, hist, prev_normal, prev_albedo, prev_cam, width, height, p, hist_out))
        return st;
    const size_t n = (size_t)width * height;
    const mrt_reproject_setup rs = make_setup(width, height, hist ? prev_cam : nullptr, p);
    const mrt_camera pc = hist ? *prev_cam : *cam;
    const uint32_t workers = (uint32_t)std::min<size_t>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), (n + 4095) / 4096);
    auto rows = [&](uint32_t k) {  // worker k of `workers`: every workers-th row
        for (uint32_t y = k; y < height; y += workers)
            for (uint32_t x = 0; x < width; x++)
                ((mrt_f4*)hist_out)[(size_t)y * width + x] = mrt_reproject_pixel(&rs, cam, &pc, (const mrt_f4*)rgb, (const mrt_f4*)normal, (const mrt_f4*)albedo,
                                                                                 (const mrt_f4*)hist, (const mrt_f4*)prev_normal, (const mrt_f4*)prev_albedo, x, y);
    };
    std::vector<std::thread> pool;
    for (uint32_t k = 1; k < workers; k++) pool.emplace_back(rows, k);
    rows(0u);
    for (std::thread& t : pool) t.join();
    return MRT_OK;
}

#ifndef MRT_TEMPORAL_HOST_ONLY
extern "C" mrt_status mrt_reproject_device(const float* d_rgb, const float* d_normal, const float* d_albedo, const mrt_camera* cam, const float* d_hist,
                                           const float* d_prev_normal, const float* d_prev_albedo, const mrt_camera* prev_cam, uint32_t width,
                                           uint32_t height, const mrt_temporal_params* p, float* d_hist_out, void* stream) {
    if (mrt_status st = check_reproject("mrt_reproject_device", d_rgb, d_normal, d_albedo, cam, d_hist, d_prev_normal, d_prev_albedo, prev_cam, width,
                                        height, p, d_hist_out))
        return st;
    const mrt_reproject_setup rs = make_setup(width, height, d_hist ? prev_cam : nullptr, p);
    const dim3 grid((width + kReprojWgX - 1u) / kReprojWgX, (height + kReprojWgY - 1u) / kReprojWgY);
    hipLaunchKernelGGL(mrt_reproject_kernel, grid, dim3(kReprojWgX, kReprojWgY), 0, (hipStream_t)stream, rs, *cam, d_hist ? *prev_cam : *cam,
                       (const mrt_f4*)d_rgb, (const mrt_f4*)d_normal, (const mrt_f4*)d_albedo, (const mrt_f4*)d_hist, (const mrt_f4*)d_prev_normal,
                       (const mrt_f4*)d_prev_albedo, (mrt_f4*)d_hist_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
}
#endif
