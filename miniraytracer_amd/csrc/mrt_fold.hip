// mrt_fold.hip -- the render's own device code and the host functions that enqueue it (mrt_fold.h):
//   mrt_fold_kernel   per pixel, folds the chunk's samples in sample order into the running
//                     accumulator with draw() (mode 0, main.cpp:161-167) or draw2() (mode 1,
//                     main.cpp:212-229) semantics -- bit-for-bit the reference's sequential sum;
//                     mrt_fold_async_kernel and mrt_fold_lean_kernel are the same fold in other shapes.
//   mrt_final_kernel  mode 0: color /= ns, luminance clamp (main.cpp:168-173); writes the float4
//                     output in local-pixel order.
//   mrt_lum_max_kernel, mrt_tonemap_kernel   the image output (main.cpp:416-444).
// Nothing here knows the scene context.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mrt_internal.h"
#include "mrt_launch.h"
#include "mrt_fold.h"
#include "../../include/mrt_tonemap.h"

using namespace mrtd;

// The sum is sequential per pixel (bit-exact order), so the kernel is load-latency bound when
// few pixels are local (multi-GPU shards): samples are fetched FOLD_DEPTH at a time (coalesced
// across the wave's pixels) before the dependent adds.
#ifndef FOLD_DEPTH
#define FOLD_DEPTH 16
#endif
// (FoldEnd: mrt_fold.h)
// what the render's path kernels consumed, reset for the context's next render in stream order
// after them: the counter slots (word (k * MRT_CNT_SLOTS + slot) * MRT_COUNTER_STRIDE) and the
// progress snapshots -- instead of clearing fills enqueued before each render (a blit kernel
// needs a free wave slot, which the other pipelined contexts' persistent path kernels hold)
MRT_DFN void reset_counters(const FoldEnd& e, uint32_t i) {
    if (i < e.nreset) e.counters[(size_t)i * MRT_COUNTER_STRIDE] = 0ull;
    if (i < e.nprog && e.hprog) __hip_atomic_store(e.hprog + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void __launch_bounds__(256) mrt_fold_kernel(const float* __restrict__ rad, float4* __restrict__ acc, uint32_t npix, uint32_t s0,
                                                      uint32_t s1, uint32_t mode, float max_lum, FoldEnd fe) {
    uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    reset_counters(fe, lp);
    if (lp >= npix) return;
    // a render's first chunk starts from +0 without reading acc (no per-render clearing fill:
    // folding +0 first gives the same bits as starting from a zeroed accumulator)
    f3 c{0.0f, 0.0f, 0.0f};
    if (s0 != 0) {
        const float4 a = acc[lp];
        c = f3{a.x, a.y, a.z};
    }
    const float* q = rad + (size_t)lp * 3;
    const size_t stride = (size_t)npix * 3;
    uint32_t s = s0;
    for (; s + FOLD_DEPTH <= s1; s += FOLD_DEPTH) {
        f3 v[FOLD_DEPTH];
#pragma unroll
        for (int k = 0; k < FOLD_DEPTH; k++) {
            const float* e = q + (size_t)(s - s0 + k) * stride;
            v[k] = f3{__builtin_nontemporal_load(e), __builtin_nontemporal_load(e + 1), __builtin_nontemporal_load(e + 2)};
        }
#pragma unroll
        for (int k = 0; k < FOLD_DEPTH; k++) c = fold_sample(c, v[k], s + k, mode, max_lum);
    }
    for (; s < s1; s++) {
        const float* e = q + (size_t)(s - s0) * stride;
        c = fold_sample(c, f3{e[0], e[1], e[2]}, s, mode, max_lum);
    }
    if (fe.out) {
        c = final_pixel(c, fe.ns, mode, max_lum);
        fe.out[lp] = make_float4(c.x, c.y, c.z, 0.0f);
    } else {
        acc[lp] = make_float4(c.x, c.y, c.z, 0.0f);
    }
}

// The fold of an MRT_RF_FOLD_ASYNC launch, on the context's own stream beside the next launch's
// path kernel: one 256-thread group per CU (one wave slot per SIMD while it runs), each lane folding
// pixels grid-strided with FOLD_ASYNC_DEPTH samples in flight -- the same operations in the same
// order as mrt_fold_kernel (bit-identical): from +0 or the accumulator, into the accumulator or,
// for the render's last launch, finished into the output with the counters reset.
// kSide: the launch left side slots free (kSideSlots) and the fold is that many one-wave groups, each
// with two batches of FOLD_SIDE_DEPTH samples in flight.
#ifndef MRT_FOLD_ASYNC_GROUPS
#define MRT_FOLD_ASYNC_GROUPS 1  // 256-thread groups per CU: one wave per SIMD
#endif
#ifndef FOLD_ASYNC_DEPTH
#define FOLD_ASYNC_DEPTH 8
#endif
#ifndef FOLD_SIDE_DEPTH
#define FOLD_SIDE_DEPTH 6  // (two batches of 6 take 60 VGPRs; of 8 spill 19)
#endif
#ifndef MRT_FOLD_ASYNC_WG
#define MRT_FOLD_ASYNC_WG 256  // threads per group
#endif
#ifndef MRT_FOLD_ASYNC_WPE
#define MRT_FOLD_ASYNC_WPE 8  // (register cap 64, a side slot's: FOLD_ASYNC_DEPTH 8 takes 46)
#endif
template <bool kSide>
__global__ void __launch_bounds__(MRT_FOLD_ASYNC_WG) __attribute__((amdgpu_waves_per_eu(MRT_FOLD_ASYNC_WPE)))
mrt_fold_async_kernel(const float* __restrict__ rad, float4* __restrict__ acc, uint32_t npix, uint32_t s0, uint32_t s1, uint32_t mode,
                      float max_lum, FoldEnd fe) {
    const uint32_t step = gridDim.x * blockDim.x;
    const uint32_t nthr = max(npix, fe.nreset);
    for (uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x; lp < nthr; lp += step) {
        reset_counters(fe, lp);
        if (lp >= npix) continue;
        f3 c{0.0f, 0.0f, 0.0f};
        if (s0 != 0) {
            const float4 a = acc[lp];
            c = f3{a.x, a.y, a.z};
        }
        const float* q = rad + (size_t)lp * 3;
        const size_t stride = (size_t)npix * 3;
        uint32_t s = s0;
        if constexpr (kSide) {
            // the loads of one batch are in flight while the other is folded: beside a path kernel the
            // wave waits its turn for every instruction, so the adds take as long as the loads
            auto load = [&](f3(&v)[FOLD_SIDE_DEPTH], uint32_t at) {
#pragma unroll
                for (int k = 0; k < FOLD_SIDE_DEPTH; k++) {
                    const float* e = q + (size_t)(at - s0 + k) * stride;
                    v[k] = f3{__builtin_nontemporal_load(e), __builtin_nontemporal_load(e + 1), __builtin_nontemporal_load(e + 2)};
                }
            };
            auto fold = [&](const f3(&v)[FOLD_SIDE_DEPTH]) {
#pragma unroll
                for (int k = 0; k < FOLD_SIDE_DEPTH; k++) c = fold_sample(c, v[k], s + k, mode, max_lum);
                s += FOLD_SIDE_DEPTH;
            };
            if (s + FOLD_SIDE_DEPTH <= s1) {
                f3 a[FOLD_SIDE_DEPTH], b[FOLD_SIDE_DEPTH];
                load(a, s);
                for (;;) {
                    bool more = s + 2 * FOLD_SIDE_DEPTH <= s1;
                    if (more) load(b, s + FOLD_SIDE_DEPTH);
                    fold(a);
                    if (!more) break;
                    more = s + 2 * FOLD_SIDE_DEPTH <= s1;
                    if (more) load(a, s + FOLD_SIDE_DEPTH);
                    fold(b);
                    if (!more) break;
                }
            }
        } else {
            for (; s + FOLD_ASYNC_DEPTH <= s1; s += FOLD_ASYNC_DEPTH) {
                f3 v[FOLD_ASYNC_DEPTH];
#pragma unroll
                for (int k = 0; k < FOLD_ASYNC_DEPTH; k++) {
                    const float* e = q + (size_t)(s - s0 + k) * stride;
                    v[k] = f3{__builtin_nontemporal_load(e), __builtin_nontemporal_load(e + 1), __builtin_nontemporal_load(e + 2)};
                }
#pragma unroll
                for (int k = 0; k < FOLD_ASYNC_DEPTH; k++) c = fold_sample(c, v[k], s + k, mode, max_lum);
            }
        }
        for (; s < s1; s++) {
            const float* e = q + (size_t)(s - s0) * stride;
            c = fold_sample(c, f3{e[0], e[1], e[2]}, s, mode, max_lum);
        }
        if (fe.out) {
            c = final_pixel(c, fe.ns, mode, max_lum);
            fe.out[lp] = make_float4(c.x, c.y, c.z, 0.0f);
        } else {
            acc[lp] = make_float4(c.x, c.y, c.z, 0.0f);
        }
    }
}

// draw()'s fold (mode 0) in 8 VGPRs: the persistent path kernel fills 7 waves per SIMD with 72
// VGPRs each (504 of 512), so only a kernel this lean fits the 8th wave slot beside it -- the fold
// of one render then runs under the next render's path kernel (bench.py --pipeline, two contexts
// on two streams) instead of after it.  Buffer loads (a scalar resource + one 32-bit VGPR offset;
// a launch chunk's radiance is < 4 GiB, mrt_prepare) keep it at 8 VGPRs: the offset, the acc
// offset, c and one sample, so one 12-B load is in flight per lane.  (Staging rows in LDS with
// buffer loads to LDS was tried: the compiler then reserves 97 VGPRs for the kernel.)  The same
// operations in the same order as mrt_fold_kernel (bit-identical).
#ifndef MRT_FOLD_LEAN_WG
#define MRT_FOLD_LEAN_WG 64  // one-wave groups take any single free wave slot (C2 step 8.44 -> 8.38 ms vs 256)
#endif
__global__ void __launch_bounds__(MRT_FOLD_LEAN_WG) __attribute__((amdgpu_num_vgpr(8)))
mrt_fold_lean_kernel(const float* __restrict__ rad, float4* __restrict__ acc, uint32_t npix, uint32_t n, uint32_t first) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npix) return;
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rad), 0, 0xFFFFFFFFu, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(acc, 0, 0xFFFFFFFFu, 0x00020000);
    f3 c{0.0f, 0.0f, 0.0f};  // the render's first chunk: from +0 (as mrt_fold_kernel)
    if (!first) {
        const auto a = __builtin_amdgcn_raw_buffer_load_b96(ra, lp * 16u, 0, 0);
        c = f3{__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2])};
    }
    const uint32_t stride = npix * 12u;
    uint32_t off = lp * 12u;
    for (uint32_t s = 0; s < n; s++, off += stride) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rr, off, 0, 2 /* nt */);
        c = fold_sample(c, f3{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2])}, s, 0u, 0.0f);
    }
    using u3 = decltype(__builtin_amdgcn_raw_buffer_load_b96(ra, 0u, 0, 0));
    const u3 o = {__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z)};
    __builtin_amdgcn_raw_buffer_store_b96(o, ra, lp * 16u, 0, 0);
}

// Also resets what the render's path kernels consumed, for the context's next render, in stream
// order after them: the counter slots of its launches (word (k * MRT_CNT_SLOTS + slot) *
// MRT_COUNTER_STRIDE) and their progress snapshots in host memory -- instead of clearing fills
// enqueued before each render (a blit kernel needs a free wave slot, which the persistent path
// kernels of the other pipelined contexts hold: up to 49 ms waits in the bench trace).
// Lean like mrt_fold_lean_kernel (one-wave groups, 8 VGPRs): a 256-thread group of a 13-VGPR
// kernel needs a wave slot on every SIMD, which the other pipelined contexts' persistent path
// kernels (7 waves x 72 VGPRs per SIMD) do not leave free -- the final of one render then waited
// for another render's path kernel to end, and the next render on its stream with it (the
// bench's 3-context timeline, DESIGN.md "Pipelined renders").  Same operations, same bits.
#ifndef MRT_FINAL_WG
#define MRT_FINAL_WG 64
#endif
__global__ void __launch_bounds__(MRT_FINAL_WG) __attribute__((amdgpu_num_vgpr(8)))
mrt_final_kernel(const float4* __restrict__ acc, float4* __restrict__ out, uint32_t npix, uint32_t ns, uint32_t mode, float max_lum,
                 unsigned long long* __restrict__ counters, unsigned long long* hprog, uint32_t nreset, uint32_t nprog) {
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp < nreset) counters[(size_t)lp * MRT_COUNTER_STRIDE] = 0ull;
    if (lp < nprog && hprog) __hip_atomic_store(hprog + lp, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (lp >= npix) return;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(acc), 0, 0xFFFFFFFFu, 0x00020000);
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, 0xFFFFFFFFu, 0x00020000);
    const auto a = __builtin_amdgcn_raw_buffer_load_b96(ra, lp * 16u, 0, 0);
    const f3 c = final_pixel(f3{__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2])}, ns, mode, max_lum);
    using u4 = decltype(__builtin_amdgcn_raw_buffer_load_b128(ra, 0u, 0, 0));
    const u4 o = {__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), 0u};
    __builtin_amdgcn_raw_buffer_store_b128(o, ro, lp * 16u, 0, 0);
}

// Image output on the device (main.cpp:416-444): global max luminance, then per-pixel Drago +
// ARGB32 -- the functions of include/mrt_tonemap.h, the same bits as the host mrt_tonemap_argb.
__global__ void __launch_bounds__(256) mrt_lum_max_kernel(const float4* __restrict__ rgb, uint32_t n, unsigned int* __restrict__ lwmax_bits) {
    float m = 0.0f;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 c = rgb[i];
        const float cc[3] = {c.x, c.y, c.z};
        const float l = mrt_luminance(cc);
        m = (m < l) ? l : m;  // std::max(L_wmax, lum): NaN and negative luminance never win
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off);
        m = (m < o) ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(lwmax_bits, __float_as_uint(m));  // m >= +0: bit order == value order
}
__global__ void __launch_bounds__(256) mrt_tonemap_kernel(const float4* __restrict__ rgb, uint32_t n, const float* __restrict__ lwmax,
                                                         uint32_t* __restrict__ argb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mrt_tonemap_params tp;
    mrt_tonemap_setup(*lwmax, &tp);
    const float4 c = rgb[i];
    const float cc[3] = {c.x, c.y, c.z};
    argb[i] = mrt_tonemap_pixel(&tp, cc);
}

mrt_status mrt_fold_enqueue(FoldShape shape, uint32_t groups, const float* rad, float4* acc, uint32_t npix, uint32_t s0, uint32_t s1,
                            uint32_t mode, float max_lum, const FoldEnd& fe, hipStream_t q) {
    switch (shape) {
    case FoldShape::AsyncSide:
        hipLaunchKernelGGL(mrt_fold_async_kernel<true>, dim3(groups), dim3(64), 0, q, rad, acc, npix, s0, s1, mode, max_lum, fe);
        break;
    case FoldShape::Async:
        hipLaunchKernelGGL(mrt_fold_async_kernel<false>, dim3(groups * MRT_FOLD_ASYNC_GROUPS), dim3(MRT_FOLD_ASYNC_WG), 0, q, rad, acc, npix, s0, s1,
                           mode, max_lum, fe);
        break;
    case FoldShape::Lean:
        hipLaunchKernelGGL(mrt_fold_lean_kernel, dim3((npix + MRT_FOLD_LEAN_WG - 1) / MRT_FOLD_LEAN_WG), dim3(MRT_FOLD_LEAN_WG), 0, q, rad, acc, npix,
                           s1 - s0, (uint32_t)(s0 == 0));
        break;
    case FoldShape::Full:
        hipLaunchKernelGGL(mrt_fold_kernel, dim3((std::max(npix, fe.nreset) + 255) / 256), dim3(256), 0, q, rad, acc, npix, s0, s1, mode, max_lum, fe);
        break;
    }
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

mrt_status mrt_final_enqueue(const float4* acc, float4* out, uint32_t npix, uint32_t ns, uint32_t mode, float max_lum,
                             unsigned long long* counters, unsigned long long* hprog, uint32_t nreset, uint32_t nprog, hipStream_t q) {
    const uint32_t blocks = (std::max(npix, nreset) + MRT_FINAL_WG - 1) / MRT_FINAL_WG;
    hipLaunchKernelGGL(mrt_final_kernel, dim3(blocks), dim3(MRT_FINAL_WG), 0, q, acc, out, npix, ns, mode, max_lum, counters, hprog, nreset, nprog);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

extern "C" mrt_status mrt_lum_max_device(const float* d_rgb, uint32_t n, float* d_lwmax, void* stream) {
    if (!d_rgb || !d_lwmax) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_lum_max_device: null");
    if (n == 0) return MRT_OK;
    const uint32_t blocks = std::min<uint32_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(mrt_lum_max_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)d_rgb, n, (unsigned int*)d_lwmax);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}
extern "C" mrt_status mrt_tonemap_device(const float* d_rgb, uint32_t n, const float* d_lwmax, uint32_t* d_argb, void* stream) {
    if (!d_rgb || !d_lwmax || !d_argb) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_tonemap_device: null");
    if (n == 0) return MRT_OK;
    hipLaunchKernelGGL(mrt_tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)d_rgb, n, d_lwmax, d_argb);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}
