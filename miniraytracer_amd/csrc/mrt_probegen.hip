// mrt_probegen.hip -- the probe generators behind the C-ABI (include/mrt.h: mrt_camera_path_probes,
// mrt_pano_probes, mrt_camera_pixel_rays, mrt_surface_probes and their _device forms), host and device
// from the one definition of each record in mrt_probegen.h, built once under the exact numerics
// contract (MRT_FAST=0, no contraction on either side): the same bits, and the bits of the per-record
// functions.  A translation unit of its own: no other object changes with it.
//
// The four generator kernels share one design: one lane per record, 256-thread groups, no LDS, no atomics, no
// barrier; a lane past n touches no memory; a record is built in registers and stored as three
// 16-byte words (the ProbeRec / CastRay layout).  Lane l of a wave stores at a 48-byte stride, as
// mrt_cast_kernel loads its rays: each of the three store instructions of a wave covers the wave's
// 3 KiB once, so every 128-byte line is written whole within the three back-to-back stores.
// The host structs (camera, grid) travel in the kernel arguments.  The range kernels come in two
// widths: where the host has shown that every path index of the call fits 32 bits, the pixel / sample
// split is a 32-bit division.
#define MRT_HOST_BACKEND 1  // mrt_probegen.h's functions for the host forms as well
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "mrt_internal.h"
#include "mrt_probegen.h"

using namespace mrtd;

// the range kernels' only argument
struct GenRangeParams {
    mrt_camera cam;  // first: camera_ray_args reads it through a pointer into the argument segment
    GenGrid g;
    uint64_t first;
    uint4* __restrict__ out;
    uint32_t n;
};
static_assert(offsetof(GenRangeParams, cam) == 0, "the camera opens the argument segment");

namespace {

[[maybe_unused]] constexpr uint32_t kGenWg = 256u;

// the host's split of path q of a render: pixel = q / ns, sample = q % ns
inline void split_path(uint64_t q, uint64_t ns, uint32_t* pixel, uint32_t* sample) {
    *pixel = (uint32_t)(q / ns);
    *sample = (uint32_t)(q % ns);
}

#ifndef MRT_PROBEGEN_HOST_ONLY
__device__ __forceinline__ void gen_store(uint4* __restrict__ out, uint32_t j, const mrt_gen_rec& r) {
    uint4* dst = out + (size_t)j * 3u;
    dst[0] = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    dst[1] = make_uint4(r.w[4], r.w[5], r.w[6], r.w[7]);
    dst[2] = make_uint4(r.w[8], r.w[9], r.w[10], r.w[11]);
}

// path first + j of the grid -> (pixel, sample); k32: first + n <= 2^32 and ns < 2^32
template <bool k32>
__device__ __forceinline__ void gen_split(uint64_t first, uint32_t j, uint64_t ns, uint32_t* pixel, uint32_t* sample) {
    if constexpr (k32) {
        const uint32_t q = (uint32_t)first + j, n32 = (uint32_t)ns;
        *pixel = q / n32;
        *sample = q - *pixel * n32;
    } else {
        const uint64_t q = first + j;
        const uint64_t p = q / ns;
        *pixel = (uint32_t)p;
        *sample = (uint32_t)(q - p * ns);
    }
}
#endif

}  // namespace

#ifndef MRT_PROBEGEN_HOST_ONLY
template <bool k32>
__global__ void __launch_bounds__(kGenWg) mrt_gen_camera_kernel(GenRangeParams P) {
    const uint32_t j = blockIdx.x * kGenWg + threadIdx.x;
    if (j >= P.n) return;
    uint32_t pixel, sample;
    gen_split<k32>(P.first, j, P.g.ns, &pixel, &sample);
    // the camera where it lies in the argument segment: scalar loads, as the path kernels read theirs
    const MRT_CONST_AS mrt_camera* cp = (const MRT_CONST_AS mrt_camera*)__builtin_amdgcn_kernarg_segment_ptr();
    gen_store(P.out, j, gen_camera_probe((const mrt_camera*)cp, P.g, pixel, sample));
}

template <bool k32>
__global__ void __launch_bounds__(kGenWg) mrt_gen_pano_kernel(GenRangeParams P) {
    const uint32_t j = blockIdx.x * kGenWg + threadIdx.x;
    if (j >= P.n) return;
    uint32_t pixel, sample;
    gen_split<k32>(P.first, j, P.g.ns, &pixel, &sample);
    gen_store(P.out, j, gen_pano_probe(P.cam, P.g, pixel, sample));
}

template <bool k32>
__global__ void __launch_bounds__(kGenWg) mrt_gen_pixel_rays_kernel(mrt_camera cam, uint32_t width, uint32_t height, uint64_t first, uint32_t n,
                                                                    uint4* __restrict__ out) {
    const uint32_t j = blockIdx.x * kGenWg + threadIdx.x;
    if (j >= n) return;
    uint32_t x, y;
    if constexpr (k32) {
        const uint32_t q = (uint32_t)first + j;
        y = q / width;
        x = q - y * width;
    } else {
        const uint64_t q = first + j;
        const uint64_t yy = q / width;
        y = (uint32_t)yy;
        x = (uint32_t)(q - yy * width);
    }
    gen_store(out, j, mrt_gen_pixel_ray(cam, width, height, x, y));
}

// n = n_hits * P records; the P lanes of one hit read the same two (four) 16-byte words
__global__ void __launch_bounds__(kGenWg) mrt_gen_surface_kernel(const uint4* __restrict__ hits, const float4* __restrict__ rays, uint32_t n,
                                                                 uint32_t sq, uint32_t P, uint64_t seed, uint64_t first_id,
                                                                 uint4* __restrict__ out) {
    const uint32_t j = blockIdx.x * kGenWg + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = j / P, k = j - i * P;
    const uint4 tp = hits[(size_t)i * 2u], nm = hits[(size_t)i * 2u + 1u];
    f3 rd{0.0f, 0.0f, 0.0f};
    float rtime = 0.0f;
    if (rays) {
        const float4 ot = rays[(size_t)i * 3u], dm = rays[(size_t)i * 3u + 1u];
        rd = f3{dm.x, dm.y, dm.z};
        rtime = ot.w;
    }
    gen_store(out, j, gen_surface_probe(tp, nm, rays != nullptr, rd, rtime, sq, seed, first_id + j, k));
}

// mrt_radiance_rays_device: *total += the rays words of n radiance records.  A grid-stride sum per lane
// (the host caps the grid), a wave sum by shuffles, one 64-bit atomic per wave; every lane of a launched
// wave reaches the shuffles.
constexpr uint32_t kRaysMaxBlocks = 1024u;
__global__ void __launch_bounds__(kGenWg) mrt_radiance_rays_kernel(const uint4* __restrict__ rad, uint32_t n, unsigned long long* __restrict__ total) {
    const uint32_t T = gridDim.x * kGenWg;
    unsigned long long sum = 0;
    for (uint64_t i = blockIdx.x * kGenWg + threadIdx.x; i < n; i += T) sum += rad[i].w;
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63u) == 0u && sum != 0) atomicAdd(total, sum);
}
#endif  // MRT_PROBEGEN_HOST_ONLY

// ---- argument rules shared by the host and device forms -----------------------------------------
namespace {

mrt_status gen_fail(const char* who, const char* what) { return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": " + what).c_str()); }

// the range [first, first + n) of a width x height x sq^2 render; n > 0
mrt_status check_range(const char* who, uint32_t width, uint32_t height, uint32_t sq, uint64_t first, uint32_t n) {
    if (width == 0 || height == 0 || sq == 0) return gen_fail(who, "a zero size");
    const uint64_t wh = (uint64_t)width * height;
    // pixel indices are 32-bit, as in the per-record forms
    if (wh > (1ull << 32)) return gen_fail(who, "an image above 2^32 pixels");
    const unsigned __int128 total = (unsigned __int128)wh * ((uint64_t)sq * sq);
    if ((unsigned __int128)first + n > total) return gen_fail(who, "the range ends past the render");
    return MRT_OK;
}

// the panorama's frame (u, v, w) as the camera's constructor makes it; the lens parameters are not read
mrt_status pano_frame(const mrt_camera_params* p, mrt_camera* frame) {
    mrt_camera_params q = *p;
    q.vfov_deg = 90.0f;
    q.aspect = 1.0f;
    q.aperture = 0.0f;
    q.focus_dist = 1.0f;
    return mrt_make_camera(&q, frame);
}

mrt_status check_surface(const char* who, uint32_t n_hits, uint32_t sq, uint32_t* n_out) {
    if (sq == 0) return gen_fail(who, "sqrt_per_hit == 0");
    const uint64_t P = (uint64_t)sq * sq;
    if (sq >= (1u << 16) || P * n_hits >= (1ull << 32)) return gen_fail(who, "n_hits * sqrt_per_hit^2 must stay below 2^32");
    *n_out = (uint32_t)(P * n_hits);
    return MRT_OK;
}

bool misaligned(const void* a, const void* b = nullptr, const void* c = nullptr) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) != 0; }

#ifndef MRT_PROBEGEN_HOST_ONLY
mrt_status launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
}
dim3 gen_blocks(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + kGenWg - 1u) / kGenWg)); }
#endif

}  // namespace

// ---- host forms ------------------------------------------------------------------------------------
extern "C" mrt_status mrt_camera_path_probes(const mrt_camera* cam, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* out) {
    if (n == 0) return MRT_OK;
    if (!cam || !d || !out) return gen_fail("mrt_camera_path_probes", "null");
    if (mrt_status st = check_range("mrt_camera_path_probes", d->width, d->height, d->sqrt_samples, first, n)) return st;
    const GenGrid g = gen_grid(d->width, d->height, d->sqrt_samples, d->seed);
    for (uint32_t j = 0; j < n; j++) {
        uint32_t pixel, sample;
        split_path(first + j, g.ns, &pixel, &sample);
        const mrt_gen_rec r = gen_camera_probe(cam, g, pixel, sample);
        memcpy(out + j, &r, sizeof r);
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_pano_probes(const mrt_camera_params* p, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* out) {
    if (n == 0) return MRT_OK;
    if (!p || !d || !out) return gen_fail("mrt_pano_probes", "null");
    mrt_camera frame;
    if (mrt_status st = pano_frame(p, &frame)) return st;
    if (mrt_status st = check_range("mrt_pano_probes", d->width, d->height, d->sqrt_samples, first, n)) return st;
    const GenGrid g = gen_grid(d->width, d->height, d->sqrt_samples, d->seed);
    for (uint32_t j = 0; j < n; j++) {
        uint32_t pixel, sample;
        split_path(first + j, g.ns, &pixel, &sample);
        const mrt_gen_rec r = gen_pano_probe(frame, g, pixel, sample);
        memcpy(out + j, &r, sizeof r);
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_camera_pixel_rays(const mrt_camera* cam, uint32_t width, uint32_t height, uint64_t first, uint32_t n, mrt_ray* out) {
    if (n == 0) return MRT_OK;
    if (!cam || !out) return gen_fail("mrt_camera_pixel_rays", "null");
    if (width == 0 || height == 0) return gen_fail("mrt_camera_pixel_rays", "a zero size");
    const uint64_t wh = (uint64_t)width * height;
    if (first > wh || n > wh - first) return gen_fail("mrt_camera_pixel_rays", "the range ends past the image");
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t q = first + j;
        const mrt_gen_rec r = mrt_gen_pixel_ray(*cam, width, height, (uint32_t)(q % width), (uint32_t)(q / width));
        memcpy(out + j, &r, sizeof r);
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_surface_probes(const mrt_hit* hits, const mrt_ray* rays, uint32_t n_hits, uint32_t sqrt_per_hit, uint64_t seed,
                                         uint64_t first_id, mrt_probe* out) {
    if (n_hits == 0) return MRT_OK;
    if (!hits || !out) return gen_fail("mrt_surface_probes", "null");
    uint32_t n;
    if (mrt_status st = check_surface("mrt_surface_probes", n_hits, sqrt_per_hit, &n)) return st;
    const uint32_t P = sqrt_per_hit * sqrt_per_hit;
    for (uint32_t i = 0; i < n_hits; i++) {
        uint4 hw[2];
        memcpy(hw, hits + i, sizeof hw);
        f3 rd{0.0f, 0.0f, 0.0f};
        float rtime = 0.0f;
        if (rays) {
            rd = f3{rays[i].d[0], rays[i].d[1], rays[i].d[2]};
            rtime = rays[i].time;
        }
        for (uint32_t k = 0; k < P; k++) {
            const uint32_t j = i * P + k;
            const mrt_gen_rec r = gen_surface_probe(hw[0], hw[1], rays != nullptr, rd, rtime, sqrt_per_hit, seed, first_id + j, k);
            memcpy(out + j, &r, sizeof r);
        }
    }
    return MRT_OK;
}

// ---- device forms ----------------------------------------------------------------------------------
#ifndef MRT_PROBEGEN_HOST_ONLY
// every path index of [first, first + n) and ns itself fit 32 bits: the kernels' 32-bit split
static bool range32(uint64_t first, uint32_t n, uint64_t ns) { return first + n <= (1ull << 32) && ns < (1ull << 32); }

extern "C" mrt_status mrt_camera_path_probes_device(const mrt_camera* cam, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* d_out,
                                                    void* stream) {
    if (n == 0) return MRT_OK;
    if (!cam || !d || !d_out) return gen_fail("mrt_camera_path_probes_device", "null");
    if (misaligned(d_out)) return gen_fail("mrt_camera_path_probes_device", "records not 16-byte aligned");
    if (mrt_status st = check_range("mrt_camera_path_probes_device", d->width, d->height, d->sqrt_samples, first, n)) return st;
    GenRangeParams P{*cam, gen_grid(d->width, d->height, d->sqrt_samples, d->seed), first, (uint4*)d_out, n};
    if (range32(first, n, P.g.ns)) hipLaunchKernelGGL(mrt_gen_camera_kernel<true>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(mrt_gen_camera_kernel<false>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, P);
    return launched();
}

extern "C" mrt_status mrt_pano_probes_device(const mrt_camera_params* p, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* d_out,
                                             void* stream) {
    if (n == 0) return MRT_OK;
    if (!p || !d || !d_out) return gen_fail("mrt_pano_probes_device", "null");
    if (misaligned(d_out)) return gen_fail("mrt_pano_probes_device", "records not 16-byte aligned");
    GenRangeParams P{};
    if (mrt_status st = pano_frame(p, &P.cam)) return st;
    if (mrt_status st = check_range("mrt_pano_probes_device", d->width, d->height, d->sqrt_samples, first, n)) return st;
    P.g = gen_grid(d->width, d->height, d->sqrt_samples, d->seed);
    P.first = first;
    P.out = (uint4*)d_out;
    P.n = n;
    if (range32(first, n, P.g.ns)) hipLaunchKernelGGL(mrt_gen_pano_kernel<true>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(mrt_gen_pano_kernel<false>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, P);
    return launched();
}

extern "C" mrt_status mrt_camera_pixel_rays_device(const mrt_camera* cam, uint32_t width, uint32_t height, uint64_t first, uint32_t n,
                                                   mrt_ray* d_out, void* stream) {
    if (n == 0) return MRT_OK;
    if (!cam || !d_out) return gen_fail("mrt_camera_pixel_rays_device", "null");
    if (misaligned(d_out)) return gen_fail("mrt_camera_pixel_rays_device", "records not 16-byte aligned");
    if (width == 0 || height == 0) return gen_fail("mrt_camera_pixel_rays_device", "a zero size");
    const uint64_t wh = (uint64_t)width * height;
    if (first > wh || n > wh - first) return gen_fail("mrt_camera_pixel_rays_device", "the range ends past the image");
    if (first + n <= (1ull << 32))
        hipLaunchKernelGGL(mrt_gen_pixel_rays_kernel<true>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, *cam, width, height, first, n,
                           (uint4*)d_out);
    else
        hipLaunchKernelGGL(mrt_gen_pixel_rays_kernel<false>, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, *cam, width, height, first, n,
                           (uint4*)d_out);
    return launched();
}

extern "C" mrt_status mrt_surface_probes_device(const mrt_hit* d_hits, const mrt_ray* d_rays, uint32_t n_hits, uint32_t sqrt_per_hit,
                                                uint64_t seed, uint64_t first_id, mrt_probe* d_out, void* stream) {
    if (n_hits == 0) return MRT_OK;
    if (!d_hits || !d_out) return gen_fail("mrt_surface_probes_device", "null");
    if (misaligned(d_hits, d_rays, d_out)) return gen_fail("mrt_surface_probes_device", "records not 16-byte aligned");
    uint32_t n;
    if (mrt_status st = check_surface("mrt_surface_probes_device", n_hits, sqrt_per_hit, &n)) return st;
    hipLaunchKernelGGL(mrt_gen_surface_kernel, gen_blocks(n), dim3(kGenWg), 0, (hipStream_t)stream, (const uint4*)d_hits, (const float4*)d_rays, n,
                       sqrt_per_hit, sqrt_per_hit * sqrt_per_hit, seed, first_id, (uint4*)d_out);
    return launched();
}

extern "C" mrt_status mrt_radiance_rays_device(const mrt_radiance* d_rad, uint32_t n, uint64_t* d_rays, void* stream) {
    if (n == 0) return MRT_OK;
    if (!d_rad || !d_rays) return gen_fail("mrt_radiance_rays_device", "null");
    if (misaligned(d_rad) || ((uintptr_t)d_rays & 7u)) return gen_fail("mrt_radiance_rays_device", "records not 16-byte aligned, or the total not 8-byte aligned");
    const uint32_t blocks = std::min(gen_blocks(n).x, kRaysMaxBlocks);
    hipLaunchKernelGGL(mrt_radiance_rays_kernel, dim3(blocks), dim3(kGenWg), 0, (hipStream_t)stream, (const uint4*)d_rad, n, (unsigned long long*)d_rays);
    return launched();
}
#endif  // MRT_PROBEGEN_HOST_ONLY
