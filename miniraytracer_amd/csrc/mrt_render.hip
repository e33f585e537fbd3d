// mrt_render.hip -- the MI355X render path behind the C-ABI (include/mrt.h).
//
// Kernels (DESIGN.md "Kernels"):
//   mrt_path_kernel   persistent waves pull 256-path batches (64 near the end of a launch) from per-XCD partition counters (one atomic
//                     per wave per batch, like work_queue::getWork pulls a tile,
//                     work_queue.cpp:158-166) and run trace() for each lane's path to completion;
//                     per-path radiance is written sample-major [s][local pixel] (coalesced).
//   mrt_fold_kernel   per pixel, folds the chunk's samples in sample order into the running
//                     accumulator with draw() (mode 0, main.cpp:161-167) or draw2() (mode 1,
//                     main.cpp:212-229) semantics -- bit-for-bit the reference's sequential sum.
//   mrt_final_kernel  mode 0: color /= ns, luminance clamp (main.cpp:168-173); writes the float4
//                     output in local-pixel order.
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <memory>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#include "mrt_internal.h"
#include "mrt_launch.h"
#include "mrt_aux.h"
#include "mrt_cast.h"
#include "mrt_probe.h"
#include "mrt_tables.h"
#include "mrt_cpu.h"
#include "mrt_moments.h"
#include "../../include/mrt_tonemap.h"

using namespace mrtd;

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return mrt_internal_fail(MRT_ERR_HIP, (std::string(#x) + ": " + hipGetErrorString(e_)).c_str()); \
    } while (0)

// The tolerance contract's kernels: per variant the path-exact build (kPathExact), else the
// denormal-flushing build (kFtzVariant), else the plain fast build -- the variant's whole column
// (a build's workgroup shape, LDS fold levels and walk flags follow its own switches).
// MRT_PATH_EXACT=0 / MRT_FTZ=0 in the environment skip a build for every variant (A/B).
static void take_variant(KernelTable& m, const KernelTable& s, uint32_t i) {
    m.kernel[i] = s.kernel[i];
    m.lev_k[i] = s.lev_k[i];
    m.wg[i] = s.wg[i];
    m.tree[i] = s.tree[i];
    m.pq[i] = s.pq[i];
    m.box6_walk[i] = s.box6_walk[i];
    m.rewrite[i] = s.rewrite[i];
}
static const KernelTable& fast_table() {
    static const KernelTable t = [] {
        KernelTable m = kernel_table_fast();
        auto off = [](const char* name) {  // A/B hooks: MRT_FTZ=0, MRT_PATH_EXACT=0
            const char* e = getenv(name);
            return e && *e && atoi(e) == 0;
        };
        const KernelTable& z = kernel_table_fast_ftz();
        const KernelTable& x = kernel_table_fast_pex();
        for (uint32_t i = 0; i < kNumVariants; i++) {
            if (x.kernel[i] && !off("MRT_PATH_EXACT")) take_variant(m, x, i);
            else if (z.kernel[i] && !off("MRT_FTZ")) take_variant(m, z, i);
            // the exact arithmetic for the rounding-critical paths of the fast variants (mrt_retrace_kernel)
            m.retrace[i] = x.retrace[i];
        }
        return m;
    }();
    return t;
}

// first variant covering the scene's features: its own program shape first, then the interpreter
static uint32_t pick_variant(uint32_t features) {
    const uint32_t feat = features & 0xFFFFu, sig = MRT_SIG_OF(features);
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t i = 0; i < kNumVariants; i++) {
            const uint32_t vf = kVariants[i] & 0xFFFFu, vs = MRT_SIG_OF(kVariants[i]);
            if ((feat & ~vf) != 0 || (vf & FT_LIN) != (feat & FT_LIN)) continue;
            if (pass == 0 ? (vs == sig && sig != SIG_NONE) : vs == SIG_NONE) return i;
        }
    return kNumVariants - 1;
}

// The sum is sequential per pixel (bit-exact order), so the kernel is load-latency bound when
// few pixels are local (multi-GPU shards): samples are fetched FOLD_DEPTH at a time (coalesced
// across the wave's pixels) before the dependent adds.
#ifndef FOLD_DEPTH
#define FOLD_DEPTH 16
#endif
// The render's last chunk (out != null) also finishes the pixels -- final_pixel into the caller's
// output -- and resets the counters (FoldEnd), so no separate final kernel follows it.
struct FoldEnd {
    float4* out;                     // the render's output (last chunk), or null: keep folding into acc
    uint32_t ns;                     // samples per pixel (mode 0 divides by it)
    unsigned long long* counters;    // work counters of the render's launches (MRT_COUNTER_STRIDE apart)
    unsigned long long* hprog;       // their progress snapshots in host memory (or null)
    uint32_t nreset;                 // counter slots to reset (MRT_CNT_SLOTS per launch)
    uint32_t nprog;                  // progress snapshots to reset (MRT_NPART per launch)
};
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

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
// Wave slots an MRT_RF_FOLD_ASYNC launch leaves free for its own retrace and fold (DESIGN.md, round
// 14): the Cornell walk kernel (box6_walk), whose one-wave groups take all eight wave slots of every
// SIMD and which is bound by VALU issue, not by its wave count, is launched with kSideSlots fewer
// groups (a multiple of MRT_NPART: every work partition gives up as many waves), and the retrace
// and the fold, both one-wave groups of at most kSideVgprs registers, run in those slots on the
// context's own stream while the next launch's path kernel already runs on the caller's.  Every
// other kernel keeps its grid: the exact contract's Cornell kernel (seven waves per SIMD) lost 5 %
// and the room + mesh kernel 1.5 % with the same slots gone (profiles/r14_ab.txt section 5).
// 768 of the MI355X's 8192: the Cornell kernel is VALU-issue bound and runs no slower without them,
// while the fold of a 3 GB launch in 512 slots outlasted the kernel beside it (profiles/r14_ab.txt).
static constexpr int kSideSlots = 768;
static constexpr int kSideVgprs = 64;
// Beside the path kernel the fold lasts about as long as that kernel does (6.2 of 6.35 ms at depth 32),
// and the launch after next waits for it: with a depth limit of 1 / 2 / 3 the kernel is short enough
// for the step to become the fold's (+3.8 % / +1.0 % / -0.2 % against the full grid, -1.0 % from 4 on),
// so launches of fewer than 4 bounces keep the full grid and the retrace on the render's stream.
static constexpr uint32_t kSideMinBounces = 4;
// one numerics build of the scene's path kernel (exact / fast): kernel, grid, registers
struct PathLaunch {
    path_kernel_t fn = nullptr;
    int grid = 0;
    int side = 0;  // one-wave groups an MRT_RF_FOLD_ASYNC launch leaves out of the grid: wave slots for its retrace and fold (kSideSlots)
    size_t lds_bytes = 0;
    uint32_t vgprs = 0;
    uint32_t wg = 64;     // threads per workgroup
    uint32_t tree_n = 0;  // BvhWide nodes kept in each workgroup's LDS (treelet kernels)
    uint32_t lds_save = 0;  // LDS words per lane slot for the query ray parked during instances
    bool rewrite = false;   // the kernel runs the tolerance-contract program rewrite (s->prog_fast)
    path_kernel_t retrace = nullptr;  // the exact arithmetic for its rounding-critical paths (mrt_retrace_kernel)
    bool handover = false;  // the kernel hands its rounding-critical paths to it (fast arithmetic)
    bool retrace_side = false;  // the retrace kernel fits a side slot (at most kSideVgprs registers)
    uint32_t walk_min = 32;  // resumable mesh walk threshold of this build (PathParams::walk_min)
};

// A workspace buffer on the device, grown on demand (mrt_prepare) and freed with its scene.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // the bytes asked for
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // at least `bytes` (a zero-byte request gets 16); before it reallocates, waits for the scene's
    // last enqueued render (quiesce)
    mrt_status grow(mrt_scene* s, size_t bytes);
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct mrt_scene {
    int device = 0;
    mrt_cpu_scene* cpu = nullptr;  // MRT_DEVICE_CPU: the CPU backend's scene (mrt_cpu.hip); nothing below is used
    DScene S{};
    DScene* d_S = nullptr;
    std::vector<void*> allocs;
    uint32_t n_nodes = 0;
    // workspace
    mrt_render_desc wdesc{};
    std::vector<uint32_t> wpixels;   // the pixel list of wdesc (mrt_render_desc.pixels), copied
    const LinOp* prog_fast = nullptr;  // the tolerance contract's program for the interpreter (lin_rewrite_fast)
    bool have_ws = false;
    uint32_t npix = 0, chunk = 0;
    DevBuf<uint2> d_pixels;
    DevBuf<float2> d_sdist;
    uint32_t sdist_sq = 0;
    DevBuf<float> d_rad;
    DevBuf<uint32_t> d_path_rays;
    DevBuf<float4> d_acc;
    DevBuf<float4> d_lev;
    DevBuf<float4> d_out;            // mrt_render's device framebuffer (local-pixel order)
    // progressive preview (MRT_RF_PREVIEW): device staging image, pinned host copy guarded by a
    // sequence word the render's stream writes around each copy (odd = copy in flight) and the
    // sample count the copy holds
    DevBuf<float4> d_prev;
    float4* h_prev = nullptr;
    size_t h_prev_cap = 0;
    uint32_t* h_seq = nullptr;       // [0] sequence, [1] samples folded into h_prev
    uint32_t prev_epoch = 0;
    std::vector<uint32_t> prev_px;   // local pixel -> row-major pixel of the previewed render
    uint32_t prev_w = 0, prev_h = 0;
    uint32_t lev_rows = 0;
    uint64_t* d_counter = nullptr;   // 64 B scratch: [0] paths handed to the exact arithmetic since upload, [2] ray total of mrt_render, [4] cancel flag,
                                     // [1] rounding-critical paths listed (u32), [3] retrace groups done (u32), [5] listed beyond the cap since upload,
                                     // [6] the parity-1 list's count (u32) and retrace groups done (u32)
    DevBuf<uint32_t> d_rt;           // rounding-critical paths listed for the retrace kernel (path indices)
    DevBuf<uint64_t> d_counters;     // one work counter per chunk launch (progress reads them)
    std::vector<uint64_t> chunk_paths;
    hipStream_t pstream = nullptr;   // non-blocking stream for the cancel-flag copy
    // host-coherent pinned memory: per-launch snapshots of the work counters, stored by the path
    // kernel itself (mrt_progress reads them with no GPU work), and the cancel flag's source
    uint64_t* h_prog = nullptr;
    size_t h_prog_cap = 0;
    std::vector<uint64_t> h_seen;  // largest snapshot read per launch (waves store out of order)
    int* h_one = nullptr;
    std::atomic<uint32_t> n_chunks{0};  // launches of the current render (0 until all are enqueued)
    // mrt_progress may run on another host thread: it and every change to the launch bookkeeping
    // above (h_prog, h_seen, ev, chunk_paths) hold this lock
    std::mutex prog_mu;
    // recorded at the end of every mrt_render_device on the caller's stream: workspace changes
    // (relayout uploads, reallocation) wait for it, so a render still running on another stream
    // never sees its buffers rewritten or freed
    hipEvent_t ev_done = nullptr;
    bool ev_done_pending = false;
    // the same for the last mrt_render_aux_device (it reads the pixel table and the sample grid)
    hipEvent_t ev_aux = nullptr;
    bool ev_aux_pending = false;
    // MRT_RF_FOLD_ASYNC: launches alternate between two radiance buffers (parity lpar), renders
    // between two sets of counter slots (rpar); the fold of parity p runs on fstream and ev_fold[p]
    // marks its end, which the next path kernel writing parity p's radiance buffer waits for (folds
    // run in order on fstream, so it also orders every earlier fold)
    hipStream_t fstream = nullptr;
    hipEvent_t ev_kern = nullptr;
    hipEvent_t ev_fold[2] = {nullptr, nullptr};
    bool fold_pending[2] = {false, false};
    uint32_t lpar = 0, rpar = 0;
    DevBuf<float> d_rad2;
    uint32_t n_cu = 0;
    uint32_t prog_base = 0;  // launch slot of the current render's counters and progress snapshots
    uint32_t slot_half = 0;  // launch slots per set (renders use set rpar at rpar * slot_half; mrt_prepare)
    unsigned long long* d_rays = nullptr;
    uint32_t features = 0, variant = 0;
    uint32_t lds_frames = 0, lds_rays = 0, lds_mesh = 0, lds_save = 0;
    uint32_t walk_min = 32;  // resumable mesh walk threshold (PathParams::walk_min)
    PathLaunch pl[2];            // [0] exact contract, [1] tolerance contract (MRT_RF_FAST)
    size_t max_threads = 0;  // largest path-kernel grid in threads (per-lane level rows)
    std::vector<hipEvent_t> ev;  // [2*k]: start/stop of path-kernel launch k of the last render
    uint32_t n_launch = 0;
    uint64_t last_paths = 0;
    uint32_t last_numerics = 0;
    uint32_t last_grid = 0;  // path-kernel groups of the last render's launches (0: none yet)
    uint32_t prog_ops = 0;  // linear hit program length (0: generic machine)
    // the adaptive render's moments sink (internal, mrt_render_adaptive): while mom is set, every
    // launch chunk's radiance is also added to mom[mom_slots ? mom_slots[lp] : lp] (mrt_moments_kernel)
    // on the render's stream, after the chunk's fold and before the next launch reuses the buffer
    float* mom = nullptr;
    const uint32_t* mom_slots = nullptr;
    // its refinement passes' pixel lists come from mrt_internal_refine_slots over checked pixels (in
    // range, no repeats): mrt_prepare skips the list check (a sort) for them
    bool trust_pixels = false;
    // the blocking mrt_cast_rays on a GPU scene: a stream and staging records of its own (rays, then
    // hits), so the call waits for its own work only; kept until the scene is freed
    hipStream_t cast_stream = nullptr;
    void* d_cast = nullptr;
    size_t d_cast_cap = 0;
    // the same for the blocking mrt_trace_rays: staging records (probes, then radiance) and the
    // fold-level workspace of its launches
    hipStream_t trace_stream = nullptr;
    void* d_trace = nullptr;
    size_t d_trace_cap = 0;
    void* d_trace_work = nullptr;
    size_t d_trace_work_cap = 0;
};

// The LDS of a one-wave launch that only walks (the retrace and aux kernels): the generic machine's
// frames and transformed rays, the mesh / bvh_node walk's stack, `lds_save` words for the query ray
// parked during instances (mrt_launch.h WaveLds, which the kernels index it by).
static WaveLds walk_lds(const mrt_scene* s, uint32_t lds_save) {
    return WaveLds{s->lds_frames, s->lds_rays, s->lds_mesh, lds_save};
}

static mrt_status dev_alloc(mrt_scene* s, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return mrt_internal_fail(e == hipErrorOutOfMemory ? MRT_ERR_OOM : MRT_ERR_HIP, "hipMalloc failed");
    s->allocs.push_back(*p);
    return MRT_OK;
}
static mrt_status upload(mrt_scene* s, const void* src, size_t bytes, void** dst) {
    void* p = nullptr;
    mrt_status st = dev_alloc(s, &p, bytes);
    if (st) return st;
    if (bytes) {
        hipError_t e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_HIP, "hipMemcpy upload failed");
    }
    *dst = p;
    return MRT_OK;
}

extern "C" mrt_status mrt_init(int* device_count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        if (device_count) *device_count = 0;
        return mrt_internal_fail(MRT_ERR_NO_DEVICE, "no HIP device visible");
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, 0));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return mrt_internal_fail(MRT_ERR_NO_DEVICE, (std::string("device is ") + prop.gcnArchName + ", libmrt is built for gfx950").c_str());
    if (device_count) *device_count = n;
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_upload(int device, const mrt_scene_view* v, mrt_scene** out) {
    if (!out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_upload: null");
    if (device == MRT_DEVICE_CPU) {  // the CPU backend (explicit choice only)
        mrt_cpu_scene* c = nullptr;
        mrt_status st = mrt_cpu_scene_create(v, &c);
        if (st) return st;
        mrt_scene* s = new mrt_scene();
        s->device = MRT_DEVICE_CPU;
        s->cpu = c;
        s->n_nodes = v->n_nodes;
        s->features = mrt_cpu_scene_features(c);
        *out = s;
        return MRT_OK;
    }
    if (device < 0) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_upload: bad device");
    SceneTables T;
    mrt_status st = mrt_internal_scene_tables(v, &T);
    if (st) return st;
    HIPCHK(hipSetDevice(device));
    // owned until *out takes it: every early return below frees the scene and what it has uploaded
    std::unique_ptr<mrt_scene, decltype(&mrt_scene_free)> owner(new mrt_scene(), mrt_scene_free);
    mrt_scene* const s = owner.get();
    s->device = device;
    DScene& S = s->S;
#define UP(src, n, dst) { void* t_ = nullptr; if ((st = upload(s, src, (size_t)(n) * sizeof(*(src)), &t_))) return st; *(dst) = (decltype(+*(dst)))t_; }
    UP(T.nodes.data(), T.nodes.size(), &S.nodes);
    UP(v->children, v->n_children, &S.children);
    UP(v->mesh_nodes, v->n_mesh_nodes, &S.mnodes);
    UP(T.wide.data(), T.wide.size(), &S.mwide);
    S.mwide_n = (uint32_t)T.wide.size();
    UP(T.bwide.data(), T.bwide.size(), &S.bwide);
    UP(T.bprims.data(), T.bprims.size(), &S.bprims);
    UP((const float4*)v->tri_geo, (size_t)v->n_tris * 3, &S.tri_geo);
    UP((const float4*)v->tri_nrm, (size_t)v->n_tris * 3, &S.tri_nrm);
    UP(T.dmats.data(), T.dmats.size(), &S.mats);
    UP(T.bleaf.data(), T.bleaf.size(), &S.bleaf);
    S.nbleaf = T.nbleaf;
    S.nbleaf_f = (float)T.nbleaf;
    S.inv_nbleaf = 1.0f / S.nbleaf_f;
    S.blist = T.blist;
    S.blazy = T.blazy;
    S.light_once = T.light_once;
    UP(v->textures, v->n_textures, &S.texs);
    UP((const float4*)v->perlin_ranvec, 256, &S.ranvec);
    UP(v->perlin_perm, 768, &S.perm);
    UP(v->texels, (size_t)v->n_texels, &S.texels);
    if (T.cornell_hits.empty()) {
        UP(T.prog.data(), T.prog.size(), &S.prog);
    } else {  // Cornell shape: the hit table behind the END op, one op's size per entry (mrt_sig.h)
        std::vector<LinOp> pw(T.prog);
        pw.resize(T.prog.size() + kHitCount);
        memcpy(pw.data() + T.prog.size(), T.cornell_hits.data(), (size_t)kHitCount * kHitWords * 4);
        UP(pw.data(), pw.size(), &S.prog);
    }
    {
        const char* e = getenv("MRT_NO_REWRITE");  // A/B hook: the interpreter on the program as compiled
        if (!T.prog_fast.empty() && !(e && *e && *e != '0')) UP(T.prog_fast.data(), T.prog_fast.size(), &s->prog_fast);
    }
    UP(&v->camera, 1, &S.camp);
#undef UP
    S.root = v->root;
    S.biased = v->biased;
    S.sky = v->sky;
    S.cam = v->camera;
    s->n_nodes = v->n_nodes;
    s->prog_ops = T.prog_ops;
    void* p;
    if ((st = upload(s, &s->S, sizeof(DScene), &p))) return st;
    s->d_S = (DScene*)p;
    if ((st = dev_alloc(s, &p, 64))) return st;
    s->d_counter = (uint64_t*)p;
    s->d_rays = (unsigned long long*)((char*)p + 16);
    HIPCHK(hipMemset(p, 0, 64));  // the cancel flag (d_counter + 4) starts clear
    // kernel variant + LDS stacks sized from the scene graph (top frame lives in registers)
    s->features = T.features;
    s->variant = pick_variant(s->features);
    const bool lin_kernel = (kVariants[s->variant] & FT_LIN) != 0;
    s->lds_frames = lin_kernel ? 0 : (uint32_t)std::max(T.max_frames - 1, 0);
    s->lds_rays = lin_kernel ? 0 : (uint32_t)T.max_rays;
    s->lds_mesh = (uint32_t)T.max_mesh;
    // the query ray parked in LDS: instances (scene_hit_lin)
    s->lds_save = (lin_kernel && (kVariants[s->variant] & FT_INST)) ? 9u : 0u;  // (round 6: 15 -> 9, mrt_lin.h inst_ray)
    // resumable mesh walk: deeper pod_bvh trees keep the wave walking longer
    s->walk_min = T.wide.size() >= 2048 ? 40u : 32u;  // inner nodes: bunny 2937, teapot ~1045
    bool walk_min_env = false;
    if (const char* e = getenv("MRT_WALK_MIN"))  // sweep hook (tools/ab_walk.sh)
        if (*e) {
            s->walk_min = (uint32_t)atoi(e);
            walk_min_env = true;
        }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    s->n_cu = (uint32_t)prop.multiProcessorCount;
    // resident workgroups per CU: one 256-thread group = one wave per SIMD (a 64-thread group =
    // a quarter of that); VGPRs (512 per SIMD lane, granule 8) and LDS (160 KiB per CU) bound it.
    // (The runtime occupancy query under-counts gfx950 register budgets, so it is computed from
    // the kernel's attributes.)  Per numerics build: their register counts differ.
    const KernelTable* tabs[2] = {&kernel_table_exact(), &fast_table()};
    for (int k = 0; k < 2; k++) {
        PathLaunch& L = s->pl[k];
        L.fn = tabs[k]->kernel[s->variant];
        L.wg = tabs[k]->wg[s->variant];
        const uint32_t waves_per_wg = L.wg / 64u;
        // the Cornell walk of the tolerance contract (mrt_sig.h cornell_fast_hit) parks no ray
        L.lds_save = tabs[k]->box6_walk[s->variant] ? 0u : s->lds_save;
        L.rewrite = tabs[k]->rewrite[s->variant] != 0;
        L.retrace = tabs[k]->retrace[s->variant];
        // a fast-arithmetic kernel hands its rounding-critical paths to the exact arithmetic
        // (mrt_shade.h light_critical); MRT_RETRACE=0 at upload keeps them (A/B)
        {
            const char* e = getenv("MRT_RETRACE");
            L.handover = k == 1 && L.retrace && L.fn != kernel_table_fast_pex().kernel[s->variant] && !(e && *e && atoi(e) == 0);
        }
        // the path-exact build (the metal bunny under the tolerance contract) yields at 32 walking
        // lanes: 40 -1.2%, 28 -1.7%, 48 -10% (bunny 1024x1024x64, profiles/r04_ab.txt section 13)
        L.walk_min = (!walk_min_env && L.fn == kernel_table_fast_pex().kernel[s->variant]) ? 32u : s->walk_min;
        hipFuncAttributes fa{};
        HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(L.fn)));
        const int vg = std::max(8, (fa.numRegs + 7) & ~7);
        const int nb_vgpr = std::max(1, std::min(8, 512 / vg) * 4 / (int)waves_per_wg);  // waves per CU / waves per group
        auto groups = [&](size_t lds) { return std::max(1, lds ? std::min<int>(nb_vgpr, (int)((160u * 1024u) / lds)) : nb_vgpr); };
        // the group's LDS as the kernel indexes it (mrt_launch.h WaveLds): the stacks, the variant's fold
        // levels and queue of path starts, each wave's copy of the Cornell hit table (mrt_sig.h;
        // T.cornell_hits, uploaded behind the program)
        WaveLds lds = walk_lds(s, L.lds_save);
        lds.lev_k = tabs[k]->lev_k[s->variant];
        lds.pq = tabs[k]->pq[s->variant];
        lds.box6 = tabs[k]->box6_walk[s->variant] != 0;
        lds.waves = waves_per_wg;
        if (lds.box6 && T.cornell_hits.empty()) return mrt_internal_fail(MRT_ERR_INVALID, "Cornell walk without a hit table");
        if (lds.bytes() > (size_t)prop.sharedMemPerBlock) return mrt_internal_fail(MRT_ERR_INVALID, "scene graph too deep for the LDS stacks");
        int nb = groups(lds.bytes());
        if (tabs[k]->tree[s->variant]) {
            // the LDS the resident groups leave free, split among them: the treelet of each group
            const size_t per = std::min<size_t>((160u * 1024u) / nb, (size_t)prop.sharedMemPerBlock);
            const uint32_t node_bytes = WaveLds::kNodeWords * 4u;  // BvhWide
            const uint32_t n_nodes = (uint32_t)T.bwide.size();
            uint32_t cap = per > lds.bytes() ? (uint32_t)((per - lds.bytes()) / node_bytes) : 0u;
#ifdef MRT_EXPERIMENTS
            if (const char* e = getenv("MRT_TREELET_NODES"))  // sweep hook
                if (*e) cap = std::min<uint32_t>(cap, (uint32_t)atoi(e));
#endif
            lds.tree_n = L.tree_n = std::min(cap, n_nodes);
        }
        L.lds_bytes = lds.bytes();
        L.vgprs = (uint32_t)fa.numRegs;
#ifdef MRT_EXPERIMENTS
        if (const char* e = getenv("MRT_BLOCKS_PER_CU"))  // experiment hook
            if (*e) nb = std::max(1, atoi(e));
#endif
        L.grid = prop.multiProcessorCount * nb;
        // every work partition needs waves of its own: a wave leaves its partition only once it is
        // handed out, and visits at most MRT_STEAL_TRIES partitions (mrt_kernels.hip)
        if (L.grid < (int)MRT_NPART) return mrt_internal_fail(MRT_ERR_HIP, "path kernel grid smaller than the work partitions");
        s->max_threads = std::max(s->max_threads, (size_t)L.grid * L.wg);
        // the slots of an async launch's side kernels (kSideSlots): the Cornell walk kernel at eight
        // one-wave groups per SIMD, the register-bound grid
        const int wps = std::min(8, 512 / vg);
        if (tabs[k]->box6_walk[s->variant] && L.wg == 64u && nb == wps * 4 && wps == 8)
            L.side = std::min(kSideSlots, L.grid / 2) / (int)MRT_NPART * (int)MRT_NPART;
        if (L.side && L.retrace) {  // a retrace that does not fit a freed slot stays on the render's stream
            hipFuncAttributes ra{};
            HIPCHK(hipFuncGetAttributes(&ra, reinterpret_cast<const void*>(L.retrace)));
            L.retrace_side = ra.numRegs <= kSideVgprs;
        }
    }
    *out = owner.release();
    return MRT_OK;
}

extern "C" void mrt_scene_free(mrt_scene* s) {
    if (!s) return;
    if (s->cpu) {
        mrt_cpu_scene_free(s->cpu);
        delete s;
        return;
    }
    (void)hipSetDevice(s->device);
    if (s->ev_done_pending) (void)hipEventSynchronize(s->ev_done);
    for (void* p : s->allocs) (void)hipFree(p);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    if (s->pstream) (void)hipStreamDestroy(s->pstream);
    if (s->h_prog) (void)hipHostFree(s->h_prog);
    if (s->h_one) (void)hipHostFree(s->h_one);
    if (s->h_prev) (void)hipHostFree(s->h_prev);
    if (s->h_seq) (void)hipHostFree(s->h_seq);
    if (s->ev_done) (void)hipEventDestroy(s->ev_done);
    if (s->ev_aux_pending) (void)hipEventSynchronize(s->ev_aux);
    if (s->ev_aux) (void)hipEventDestroy(s->ev_aux);
    if (s->fstream) (void)hipStreamDestroy(s->fstream);
    if (s->cast_stream) (void)hipStreamDestroy(s->cast_stream);
    if (s->d_cast) (void)hipFree(s->d_cast);
    if (s->trace_stream) (void)hipStreamDestroy(s->trace_stream);
    if (s->d_trace) (void)hipFree(s->d_trace);
    if (s->d_trace_work) (void)hipFree(s->d_trace_work);
    for (hipEvent_t e : {s->ev_kern, s->ev_fold[0], s->ev_fold[1]})
        if (e) (void)hipEventDestroy(e);
    delete s;  // (the workspace buffers release themselves: DevBuf)
}

static uint32_t auto_chunk(uint32_t npix, uint32_t ns) {
    // keep the per-chunk radiance buffer within ~4 GiB of HBM (288 GB per MI355X)
    const size_t budget = (size_t)4 << 30;
    size_t per_sample = (size_t)npix * 12;
    size_t c = per_sample ? budget / per_sample : ns;
    if (c < 1) c = 1;
    return (uint32_t)std::min<size_t>(c, ns);
}

static bool same_layout(const mrt_render_desc& a, const std::vector<uint32_t>& a_px, const mrt_render_desc& b) {
    if (a.width != b.width || a.height != b.height || (a.pixels != nullptr) != (b.pixels != nullptr)) return false;
    if (b.pixels) return a_px.size() == b.n_pixels && std::equal(a_px.begin(), a_px.end(), b.pixels);
    return a.tile_size == b.tile_size && a.rank == b.rank && a.world == b.world;
}

// Before the workspace is rewritten or reallocated: wait for the last enqueued render of this
// context (it may still run on a caller stream that the synchronous uploads do not order against).
static mrt_status quiesce(mrt_scene* s) {
    if (s->ev_done_pending) {
        HIPCHK(hipEventSynchronize(s->ev_done));
        s->ev_done_pending = false;
    }
    if (s->ev_aux_pending) {
        HIPCHK(hipEventSynchronize(s->ev_aux));
        s->ev_aux_pending = false;
    }
    return MRT_OK;
}
template <typename T>
mrt_status DevBuf<T>::grow(mrt_scene* s, size_t bytes) {
    if (cap >= bytes && p) return MRT_OK;
    mrt_status st = quiesce(s);
    if (st) return st;
    release();
    hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 16);
    if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "workspace allocation failed");
    cap = bytes;
    return MRT_OK;
}

// rounding-critical paths listed per launch (mrt_shade.h light_critical; a full list loses the rest,
// which keep their fast radiance): measured ~1e-5 per path in the Cornell scenes
static constexpr uint32_t kRtCap = 1u << 20;
// one-wave groups of the retrace kernel: 16384 lanes, a path each (more loop); its time is the longest
// listed path's, plus the launch
static constexpr uint32_t kRetraceGroups = 256;
// (Round 6: the retrace of an MRT_RF_FOLD_ASYNC launch beside the next launch's path kernel -- on the
// context's fold stream, and there in one-wave slots the next kernel left free -- measured slower:
// the previous launch's fold uses the GPU during the retrace's gap on the render's stream, and behind
// the retrace on the fold stream it got only the free slots, profiles/r06_ab.txt sections 2 and 7.
// Round 14 does it with slots for both, a fold of one-wave groups and a retrace of at most 64
// registers: kSideSlots.)

#define MRT_GPU_ONLY(s, what) \
    if ((s) && (s)->cpu) return mrt_internal_fail(MRT_ERR_INVALID, what " is a GPU-backend entry point (scene on MRT_DEVICE_CPU)")

extern "C" mrt_status mrt_prepare(mrt_scene* s, const mrt_render_desc* d) {
    MRT_GPU_ONLY(s, "mrt_prepare");
    if (!s || !d || d->width == 0 || d->height == 0 || d->sqrt_samples == 0 || (d->world && d->rank >= d->world))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_prepare: bad desc");
    // the path kernel's u = (x + dx) / W by one reciprocal is exact up to 2^24 (mrt_kernels.hip)
    if (d->width > (1u << 24) || d->height > (1u << 24))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_prepare: width / height above 2^24 pixels");
    // every GPU entry point renders in per-path stream order (mrt_render_device and mrt_render come here)
    if (d->flags & MRT_RF_REF_ORDER)
        return mrt_internal_fail(MRT_ERR_INVALID, "MRT_RF_REF_ORDER is a CPU-backend mode (the GPU keys its PCG streams per path)");
    mrt_status st;
    if (!s->trust_pixels && (st = mrt_internal_check_pixels(d))) return st;
    HIPCHK(hipSetDevice(s->device));
    bool relayout = !s->have_ws || !same_layout(s->wdesc, s->wpixels, *d);
    uint32_t ns = d->sqrt_samples * d->sqrt_samples;
    if (relayout) {
        std::vector<uint32_t> px = mrt_internal_local_pixels(d);
        std::vector<uint2> xy(px.size());
        for (size_t i = 0; i < px.size(); i++) xy[i] = make_uint2(px[i] % d->width, px[i] / d->width);
        if ((st = quiesce(s))) return st;
        if ((st = s->d_pixels.grow(s, xy.size() * 8))) return st;
        HIPCHK(hipMemcpy(s->d_pixels.p, xy.data(), xy.size() * 8, hipMemcpyHostToDevice));
        s->npix = (uint32_t)px.size();
    }
    if (s->sdist_sq != d->sqrt_samples) {  // sample grid of main.cpp:319-332, in float like the reference
        const uint32_t sq = d->sqrt_samples;
        std::vector<float2> sd((size_t)sq * sq);
        for (uint32_t i = 0; i < sq; i++)
            for (uint32_t j = 0; j < sq; j++)
                sd[(size_t)i * sq + j] = make_float2(((float)i + 0.5f) / (float)sq, ((float)j + 0.5f) / (float)sq);
        if ((st = quiesce(s))) return st;
        if ((st = s->d_sdist.grow(s, sd.size() * 8))) return st;
        HIPCHK(hipMemcpy(s->d_sdist.p, sd.data(), sd.size() * 8, hipMemcpyHostToDevice));
        s->sdist_sq = sq;
    }
    uint32_t chunk = d->chunk_samples ? std::min(d->chunk_samples, ns) : auto_chunk(s->npix, ns);
    chunk = (uint32_t)std::min<uint64_t>(chunk, 0xFFFFFFFFull / std::max<uint32_t>(s->npix, 1));  // 32-bit path index
    // 32-bit byte offsets of the chunk's radiance (the path kernel's held store, mrt_kernels.hip)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, 0xFFFFFFFFull / (12ull * std::max<uint32_t>(s->npix, 1))));
    if (chunk == 0) return mrt_internal_fail(MRT_ERR_INVALID, "image too large for one launch");
    if (d->flags & MRT_RF_PATH_DEBUG) chunk = ns;  // debug keeps every path
    if (chunk != s->chunk && (st = quiesce(s))) return st;  // the fold of a running render reads `chunk` rows
    s->chunk = chunk;
    size_t paths = (size_t)s->npix * s->chunk;
    if ((st = s->d_rad.grow(s, paths * 12))) return st;
    if (d->flags & MRT_RF_FOLD_ASYNC) {
        if (d->flags & (MRT_RF_PREVIEW | MRT_RF_PATH_DEBUG | MRT_RF_FOLD_BEHIND))
            return mrt_internal_fail(MRT_ERR_INVALID, "MRT_RF_FOLD_ASYNC: no preview, debug or lean fold");
        if ((st = s->d_rad2.grow(s, paths * 12))) return st;
        if (!s->fstream) HIPCHK(hipStreamCreateWithFlags(&s->fstream, hipStreamNonBlocking));
        if (!s->ev_kern) HIPCHK(hipEventCreateWithFlags(&s->ev_kern, hipEventDisableTiming));
        for (hipEvent_t& e : s->ev_fold)
            if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // (two lists: one per radiance parity of the async fold)
    if ((d->flags & MRT_RF_FAST) && !(d->flags & MRT_RF_PATH_DEBUG) && s->pl[1].handover &&
        (st = s->d_rt.grow(s, (size_t)2 * kRtCap * sizeof(uint32_t))))
        return st;
    if ((st = s->d_acc.grow(s, (size_t)s->npix * 16))) return st;
    if ((st = s->d_out.grow(s, (size_t)s->npix * 16 + 16))) return st;
    if (d->flags & MRT_RF_PREVIEW) {
        if ((st = s->d_prev.grow(s, (size_t)s->npix * 16 + 16))) return st;
        std::lock_guard<std::mutex> lk(s->prog_mu);
        if (s->h_prev_cap < s->npix) {
            if ((st = quiesce(s))) return st;
            if (s->h_prev) (void)hipHostFree(s->h_prev);
            s->h_prev = nullptr;
            s->h_prev_cap = 0;
            HIPCHK(hipHostMalloc((void**)&s->h_prev, (size_t)s->npix * 16 + 16, hipHostMallocPortable));
            s->h_prev_cap = s->npix;
        }
        if (!s->h_seq) {
            HIPCHK(hipHostMalloc((void**)&s->h_seq, 64, hipHostMallocPortable | hipHostMallocCoherent));
            memset(s->h_seq, 0, 64);
        }
        if (relayout || s->prev_px.size() != s->npix) {
            s->prev_px = mrt_internal_local_pixels(d);
        }
        s->prev_w = d->width;
        s->prev_h = d->height;
    }
    if (d->flags & MRT_RF_PATH_DEBUG)
        if ((st = s->d_path_rays.grow(s, paths * 4))) return st;
    s->lev_rows = std::max<uint32_t>(d->max_bounces, 1);
    if ((st = s->d_lev.grow(s, (size_t)s->lev_rows * s->max_threads * 16))) return st;
    // Two sets of counter slots / progress snapshots, `slot_half` launches each, at FIXED offsets 0
    // and slot_half: consecutive MRT_RF_FOLD_ASYNC renders alternate between them, because a render's
    // last fold still resets its set while the next render's kernels count in the other.  The stride
    // must not follow each render's own launch count: a render of 1 launch after one of 4 would
    // otherwise start its set inside the previous render's (whose reset then lands mid-claim).  The
    // set is grown only after quiesce() (no render pending), and render R+2 -- the next user of R's
    // set -- waits for R's last fold (its first launch waits for the fold of the same radiance
    // parity, and folds run in order on the context's stream).
    const uint32_t need = (ns + s->chunk - 1) / s->chunk;
    const uint32_t half = std::max(s->slot_half, need);
    const uint32_t launches = 2 * half;
    const size_t cnt_words = (size_t)MRT_CNT_SLOTS * MRT_COUNTER_STRIDE;  // per launch
    {
        const size_t bytes = (size_t)launches * cnt_words * 8;
        const bool kept = s->d_counters.p && s->d_counters.cap >= bytes;
        if ((st = s->d_counters.grow(s, bytes))) return st;
        // zeroed once at allocation; afterwards every render's final kernel leaves them zero
        if (!kept) HIPCHK(hipMemset(s->d_counters.p, 0, s->d_counters.cap));
    }
    if (!s->pstream) HIPCHK(hipStreamCreateWithFlags(&s->pstream, hipStreamNonBlocking));
    if (!s->ev_done) HIPCHK(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    if (!s->ev_aux) HIPCHK(hipEventCreateWithFlags(&s->ev_aux, hipEventDisableTiming));
    {
        std::lock_guard<std::mutex> lk(s->prog_mu);
        if (s->h_prog_cap < (size_t)launches) {
            if ((st = quiesce(s))) return st;
            if (s->h_prog) (void)hipHostFree(s->h_prog);
            s->h_prog = nullptr;
            s->h_prog_cap = 0;
            HIPCHK(hipHostMalloc((void**)&s->h_prog, (size_t)launches * MRT_NPART * 8, hipHostMallocPortable | hipHostMallocCoherent));
            memset(s->h_prog, 0, (size_t)launches * MRT_NPART * 8);  // later: reset by each render's final kernel
            s->h_prog_cap = launches;
        }
        s->slot_half = half;  // (both buffers now hold 2 * half launches)
        if (s->h_seen.size() < (size_t)launches * MRT_NPART) s->h_seen.resize((size_t)launches * MRT_NPART, 0);
        if (s->chunk_paths.size() < launches) s->chunk_paths.resize(launches, 0);
        while (s->ev.size() < 2 * (size_t)launches) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            s->ev.push_back(e);
        }
    }
    if (!s->h_one) {
        HIPCHK(hipHostMalloc((void**)&s->h_one, sizeof(int), hipHostMallocPortable));
        *s->h_one = 1;
    }
    if (relayout) s->wpixels = d->pixels ? std::vector<uint32_t>(d->pixels, d->pixels + d->n_pixels) : std::vector<uint32_t>();
    s->wdesc = *d;
    s->wdesc.pixels = nullptr;  // (the caller's list is not kept; wpixels holds a copy)
    if (d->pixels) s->wdesc.pixels = s->wpixels.data();
    s->have_ws = true;
    return MRT_OK;
}

// What a render launch and the aux launch share of PathParams (after mrt_prepare): the scene, the
// build's LDS stack words, the pixel table and the sample grid, the image and the path streams.
static PathParams launch_params(const mrt_scene* s, const PathLaunch& PL, const mrt_render_desc* d) {
    PathParams P{};
    P.sc = s->S;
    P.lds_frames = s->lds_frames;
    P.lds_rays = s->lds_rays;
    P.lds_mesh = s->lds_mesh;
    P.lds_save = PL.lds_save;
    P.pixels = s->d_pixels.p;
    P.sdist = s->d_sdist.p;
    P.npix = s->npix;
    P.inv_npix = 1.0 / (double)std::max<uint32_t>(s->npix, 1);
    P.width = d->width;
    P.height = d->height;
    P.inv_w = 1.0f / (float)d->width;
    P.inv_h = 1.0f / (float)d->height;
    P.fast_uv = 1;  // checked by mrt_prepare (and sq < 2^16 since sq^2 fits in 32 bits)
    P.sq = d->sqrt_samples;
    P.ns = d->sqrt_samples * d->sqrt_samples;
    P.seed = d->seed;
    return P;
}

extern "C" mrt_status mrt_render_device(mrt_scene* s, const mrt_render_desc* d, float* d_local, uint64_t* d_rays, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_device");
    if (!s || !d || !d_local) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_device: null");
    s->n_chunks.store(0, std::memory_order_release);  // progress: a new render, not started
    mrt_status st = mrt_prepare(s, d);
    if (st) return st;
    const PathLaunch& PL = s->pl[(d->flags & MRT_RF_FAST) ? 1 : 0];
    hipStream_t q = (hipStream_t)stream;
    uint32_t ns = d->sqrt_samples * d->sqrt_samples;
    // No clearing fills enqueued here: the first fold chunk starts from +0 instead of reading the
    // accumulator, and the work counters and progress snapshots were left zero by the previous
    // render's final kernel (stream order; zeroed at allocation before the first).  The cancel flag
    // is clear unless a cancelled mrt_render set it, and that clears it again before returning.
    const uint32_t launches = (ns + s->chunk - 1) / s->chunk;
    {
        std::lock_guard<std::mutex> lk(s->prog_mu);
        for (uint32_t k = 0; k < launches; k++) {
            s->chunk_paths[k] = (uint64_t)s->npix * (std::min(ns, (k + 1) * s->chunk) - k * s->chunk);
            // the host's running maxima only: a snapshot is read only once this render's launch k
            // has started (its start event), i.e. after the previous render's final kernel reset it
            for (uint32_t j = 0; j < MRT_NPART; j++) s->h_seen[(size_t)k * MRT_NPART + j] = 0;
        }
    }
    s->n_launch = 0;
    s->last_numerics = (d->flags & MRT_RF_FAST) ? 1u : 0u;
    const bool preview = (d->flags & MRT_RF_PREVIEW) != 0;
    // MRT_RF_FOLD_ASYNC: each launch writes the radiance buffer of its parity, whose last fold (on
    // fstream) must have ended first; the render uses the counter slots of its parity (the previous
    // render's folds may still reset theirs).  Any other render waits for every pending fold.
    const bool async = (d->flags & MRT_RF_FOLD_ASYNC) != 0;
    const uint32_t rpar = async ? s->rpar : 0u;
    if (async) s->rpar ^= 1u;
    if (!async)
        for (uint32_t p = 0; p < 2; p++)
            if (s->fold_pending[p]) HIPCHK(hipStreamWaitEvent(q, s->ev_fold[p], 0));
    {
        std::lock_guard<std::mutex> lk(s->prog_mu);
        s->prog_base = rpar * s->slot_half;
    }
    unsigned long long* const d_cnt = (unsigned long long*)(s->d_counters.p + (size_t)rpar * s->slot_half * MRT_CNT_SLOTS * MRT_COUNTER_STRIDE);
    unsigned long long* const h_prog = (unsigned long long*)(s->h_prog + (size_t)rpar * s->slot_half * MRT_NPART);
    uint32_t seq = 0;
    if (preview) {  // a new render: no snapshot yet (sequence 0), in stream order
        std::lock_guard<std::mutex> lk(s->prog_mu);
        HIPCHK(hipStreamWriteValue32(q, s->h_seq + 1, 0u, 0));
        HIPCHK(hipStreamWriteValue32(q, s->h_seq, 0u, 0));
        s->prev_epoch++;
    }
    // the rounding-critical paths' hand-over: tolerance contract, not the per-path debug output
    // (whose radiance is the fast kernel's own)
    const bool handover = PL.handover && !(d->flags & MRT_RF_PATH_DEBUG);
    // MRT_RF_FOLD_ASYNC on a kernel that fills every SIMD: PL.side groups fewer, whose wave slots the
    // launch's retrace and fold take on fstream (kSideSlots).  Per-path streams: which wave runs a
    // path changes neither the image nor the ray total.
    // (not below kSideMinBounces: a shallow launch's kernel is shorter than its fold runs beside it)
    const int side = async && d->max_bounces >= kSideMinBounces ? PL.side : 0;
    const int grid = PL.grid - side;
    s->last_grid = (uint32_t)grid;
    for (uint32_t s0 = 0; s0 < ns; s0 += s->chunk) {
        uint32_t s1 = std::min(ns, s0 + s->chunk);
        const uint32_t par = async ? s->lpar : 0u;
        if (async) {
            s->lpar ^= 1u;
            if (s->fold_pending[par]) HIPCHK(hipStreamWaitEvent(q, s->ev_fold[par], 0));
        }
        float* const d_rad = par ? s->d_rad2.p : s->d_rad.p;
        PathParams P = launch_params(s, PL, d);
        // the interpreter's tolerance-contract program (rooms and box.h lists as slab tests); the
        // shape-specialised walks read the program as compiled
        if ((d->flags & MRT_RF_FAST) && s->prog_fast && PL.rewrite) P.sc.prog = s->prog_fast;
        P.walk_min = PL.walk_min;
        P.tree_src = reinterpret_cast<const float4*>(s->S.bwide);
        P.tree_n = PL.tree_n;
        P.s0 = s0;
        P.n_paths = s->npix * (s1 - s0);
        P.tail_zone = (uint32_t)std::min<uint64_t>((uint64_t)grid * (PL.wg / 64u) * 2 * MRT_BATCH, P.n_paths);  // ~2 big claims per wave
        P.static_first = (uint64_t)P.n_paths < (uint64_t)grid * (PL.wg / 64u) * MRT_BATCH * 64u;
        // MRT_NPART contiguous work partitions, one counter each; the waves of partition k (workgroups
        // b with b % MRT_NPART == k) take its first batches statically when P.static_first
        for (uint32_t k = 0; k <= MRT_NPART; k++) P.part_base[k] = (uint64_t)P.n_paths * k / MRT_NPART;
        for (uint32_t k = 0; k < MRT_NPART; k++) {
            const uint64_t waves_k = (uint64_t)((grid - k + MRT_NPART - 1) / MRT_NPART) * (PL.wg / 64u);
            P.part_dyn[k] = P.part_base[k] + (P.static_first ? waves_k * MRT_BATCH : 0);
        }
        P.max_bounces = d->max_bounces;
        P.rad = d_rad;
        P.path_rays = (d->flags & MRT_RF_PATH_DEBUG) ? s->d_path_rays.p : nullptr;
        P.counter = d_cnt + (size_t)s->n_launch * MRT_CNT_SLOTS * MRT_COUNTER_STRIDE;
        P.hprog = h_prog + (size_t)s->n_launch * MRT_NPART;
        P.cancel = (const int*)(s->d_counter + 4);
        P.rays = d_rays ? (unsigned long long*)d_rays : s->d_rays;
        P.lev = s->d_lev.p;
        P.lev_rows = s->lev_rows;
        // the list of the launch's radiance parity: entries at par * kRtCap, its count and its groups-done
        // word at d_counter[1] / [3] (parity 0) or the two halves of d_counter[6] (parity 1)
        if (handover)
            P.rt = RetraceList{s->d_rt.p + (size_t)par * kRtCap, par ? (uint32_t*)(s->d_counter + 6) : (uint32_t*)(s->d_counter + 1), kRtCap,
                               par ? (uint32_t*)(s->d_counter + 6) + 1 : (uint32_t*)(s->d_counter + 3), (unsigned long long*)s->d_counter,
                               (unsigned long long*)(s->d_counter + 5)};
        HIPCHK(hipEventRecord(s->ev[2 * s->n_launch], q));
        hipLaunchKernelGGL(PL.fn, dim3(grid), dim3(PL.wg), PL.lds_bytes, q, P);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s->ev[2 * s->n_launch + 1], q));
        s->n_launch++;
        // this launch's rounding-critical paths, exact, into the radiance buffer before its fold (the
        // exact arithmetic walks the program as compiled: the tolerance contract's rewrite has ops -- a
        // room's slab test, one-step box instances -- only the fast builds compile)
        // (with side slots: on fstream in front of the fold, so the caller's stream goes straight on to
        // the next launch; the list it empties is its parity's, which the launch after next fills only
        // after ev_fold[par])
        const bool rside = side && PL.retrace_side;
        if (rside) {
            HIPCHK(hipEventRecord(s->ev_kern, q));
            HIPCHK(hipStreamWaitEvent(s->fstream, s->ev_kern, 0));
        }
        if (handover) {
            PathParams PR = P;
            PR.sc.prog = s->S.prog;
            PR.lds_save = s->lds_save;  // (the exact arithmetic parks a ray where the Cornell walk does not)
            hipLaunchKernelGGL(PL.retrace, dim3(kRetraceGroups), dim3(64), walk_lds(s, PR.lds_save).bytes(), rside ? s->fstream : q, PR);
            HIPCHK(hipGetLastError());
        }
        // the last chunk's full fold finishes the render (no preview: no snapshot of acc needed;
        // the 8-VGPR lean fold cannot take the division as well: a final kernel follows it); an
        // MRT_RF_FOLD_ASYNC render has neither preview nor lean fold (mrt_prepare)
        const bool lean = (d->flags & MRT_RF_FOLD_BEHIND) && d->mode == 0;
        const bool last = s1 == ns && !preview && !lean;
        const FoldEnd fe{last ? (float4*)d_local : nullptr, ns, last ? d_cnt : nullptr, last ? h_prog : nullptr,
                         last ? launches * MRT_CNT_SLOTS : 0u, last ? launches * MRT_NPART : 0u};
        if (async) {  // the fold on the fold stream, beside the next launch's path kernel
            // (with side slots: one-wave groups, as many as the launch left free -- a 256-thread group
            // needs a free slot on all four SIMDs of a CU at once)
            if (!rside) {
                HIPCHK(hipEventRecord(s->ev_kern, q));
                HIPCHK(hipStreamWaitEvent(s->fstream, s->ev_kern, 0));
            }
            if (side)
                hipLaunchKernelGGL(mrt_fold_async_kernel<true>, dim3(side), dim3(64), 0, s->fstream, d_rad, s->d_acc.p, s->npix, s0, s1, d->mode,
                                   d->max_luminance, fe);
            else
                hipLaunchKernelGGL(mrt_fold_async_kernel<false>, dim3(s->n_cu * MRT_FOLD_ASYNC_GROUPS), dim3(MRT_FOLD_ASYNC_WG), 0, s->fstream, d_rad,
                                   s->d_acc.p, s->npix, s0, s1, d->mode, d->max_luminance, fe);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(s->ev_fold[par], s->fstream));
            s->fold_pending[par] = true;
            s->last_paths = P.n_paths;
            continue;
        }
        const uint32_t nthr = std::max(s->npix, fe.nreset);
        if (lean)
            hipLaunchKernelGGL(mrt_fold_lean_kernel, dim3((s->npix + MRT_FOLD_LEAN_WG - 1) / MRT_FOLD_LEAN_WG), dim3(MRT_FOLD_LEAN_WG), 0, q,
                               d_rad, s->d_acc.p, s->npix, s1 - s0, (uint32_t)(s0 == 0));
        else
            hipLaunchKernelGGL(mrt_fold_kernel, dim3((nthr + 255) / 256), dim3(256), 0, q, d_rad, s->d_acc.p, s->npix, s0, s1, d->mode,
                               d->max_luminance, fe);
        HIPCHK(hipGetLastError());
        if (s->mom && (st = mrt_internal_moments_enqueue(d_rad, s->npix, s1 - s0, s->mom_slots, s->mom, q))) return st;
        if (preview) {  // the image after s1 samples, copied under the sequence lock
            hipLaunchKernelGGL(mrt_final_kernel, dim3((s->npix + MRT_FINAL_WG - 1) / MRT_FINAL_WG), dim3(MRT_FINAL_WG), 0, q, s->d_acc.p, s->d_prev.p,
                               s->npix, s1, d->mode, d->max_luminance,
                               (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0u, 0u);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamWriteValue32(q, s->h_seq, 2 * seq + 1, 0));
            HIPCHK(hipMemcpyAsync(s->h_prev, s->d_prev.p, (size_t)s->npix * 16, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamWriteValue32(q, s->h_seq + 1, s1, 0));
            HIPCHK(hipStreamWriteValue32(q, s->h_seq, 2 * seq + 2, 0));
            seq++;
        }
        s->last_paths = P.n_paths;
    }
    if (preview || ((d->flags & MRT_RF_FOLD_BEHIND) && d->mode == 0)) {  // (otherwise the last fold wrote the output and reset the counters)
        const uint32_t nreset = launches * MRT_CNT_SLOTS;
        const uint32_t blocks = (std::max(s->npix, nreset) + MRT_FINAL_WG - 1) / MRT_FINAL_WG;
        hipLaunchKernelGGL(mrt_final_kernel, dim3(blocks), dim3(MRT_FINAL_WG), 0, q, s->d_acc.p, (float4*)d_local, s->npix, ns, d->mode,
                           d->max_luminance, d_cnt, h_prog, nreset, launches * MRT_NPART);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(s->ev_done, async ? s->fstream : q));
    s->ev_done_pending = true;
    s->n_chunks.store(launches, std::memory_order_release);  // progress reads start once every launch and its events are enqueued
    return MRT_OK;
}

// mrt_render on the GPU up to the end of the wait: the render of d into the scene's device
// framebuffer (d_out, local-pixel order; s->npix pixels) and its ray total (d_rays), both complete
// when it returns.  *cancelled: the caller's flag stopped it (a partial image).
static mrt_status render_wait(mrt_scene* s, const mrt_render_desc* d, const volatile int* cancel, bool* was_cancelled) {
    *was_cancelled = false;
    s->n_chunks.store(0, std::memory_order_release);
    if (cancel && *cancel) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled");
    mrt_render_desc dc = *d;  // a cancellable render runs as >= 16 launches; cancel lands between them
    const uint32_t ns = d->sqrt_samples * d->sqrt_samples;
    // (so does a previewed one: each launch adds a snapshot)
    if ((cancel || (dc.flags & MRT_RF_PREVIEW)) && dc.chunk_samples == 0 && !(dc.flags & MRT_RF_PATH_DEBUG))
        dc.chunk_samples = std::max(1u, ns / 16);
    d = &dc;
    mrt_status st = mrt_prepare(s, d);
    if (st) return st;
    HIPCHK(hipMemset(s->d_rays, 0, 8));
    st = mrt_render_device(s, d, (float*)s->d_out.p, (uint64_t*)s->d_rays, nullptr);
    if (st) return st;
    // wait, forwarding the caller's cancel flag to the device flag the path kernel polls
    bool cancelled = false;
    if (!cancel) {
        HIPCHK(hipEventSynchronize(s->ev_done));
    } else {
        for (;;) {
            const hipError_t q = hipEventQuery(s->ev_done);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(q));
            if (*cancel && !cancelled) {
                HIPCHK(hipMemcpyAsync(s->d_counter + 4, s->h_one, sizeof(int), hipMemcpyHostToDevice, s->pstream));
                HIPCHK(hipStreamSynchronize(s->pstream));
                cancelled = true;
            }
            usleep(200);
        }
    }
    s->ev_done_pending = false;
    if (cancelled) HIPCHK(hipMemset(s->d_counter + 4, 0, 8));  // the render is over: clear the flag for the next one
    *was_cancelled = cancelled;
    return MRT_OK;
}

extern "C" mrt_status mrt_render(mrt_scene* s, const mrt_render_desc* d, float* rgb_out, uint64_t* rays_out, const volatile int* cancel) {
    if (!s || !d || !rgb_out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render: null");
    if (s->cpu) return mrt_cpu_render(s->cpu, d, rgb_out, rays_out, cancel);
    bool cancelled = false;
    if (mrt_status st = render_wait(s, d, cancel, &cancelled)) return st;
    std::vector<float> local((size_t)s->npix * 4);
    std::vector<uint32_t> px = mrt_internal_local_pixels(d);
    HIPCHK(hipMemcpy(local.data(), s->d_out.p, local.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < px.size(); i++) memcpy(rgb_out + (size_t)px[i] * 4, &local[i * 4], 16);
    uint64_t rays = 0;
    HIPCHK(hipMemcpy(&rays, s->d_rays, 8, hipMemcpyDeviceToHost));
    if (rays_out) *rays_out = rays;
    if (cancelled) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (partial image)");
    return MRT_OK;
}

// ---- the adaptive render (include/mrt.h "sample moments and the adaptive render") ----
// The call's own device buffers: the running colour C and the moments m of the pass-0 local pixels
// (one slot each) and the slot map of the current refinement pass.  Every pass is a render_wait --
// mrt_render's own path, stream-ordered fold included -- with the moments sink set; a refinement
// pass lands in the scene's d_out in list order and mrt_merge_kernel folds it into C through the
// slot map.  The decision runs on the host from a copy of the moments.
namespace {
struct AdaptiveBufs {  // one allocation: C, then m (n float4 each), then the slot map
    float *C = nullptr, *m = nullptr;
    uint32_t* slots = nullptr;
    mrt_scene* s = nullptr;
    ~AdaptiveBufs() {
        if (s) s->mom = nullptr, s->mom_slots = nullptr, s->trust_pixels = false;
        if (C) (void)hipFree(C);
    }
};
}  // namespace

static mrt_status render_adaptive_gpu(mrt_scene* s, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out, float* moments_out,
                                      uint64_t* rays_out, const volatile int* cancel) {
    HIPCHK(hipSetDevice(s->device));
    const std::vector<uint32_t> px0 = mrt_internal_local_pixels(d);
    const uint32_t n0 = (uint32_t)px0.size();
    AdaptiveBufs B;
    if (hipMalloc((void**)&B.C, (size_t)n0 * 36 + 16) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "mrt_render_adaptive: device buffers");
    B.m = B.C + (size_t)n0 * 4;
    B.slots = (uint32_t*)(B.m + (size_t)n0 * 4);
    HIPCHK(hipMemset(B.m, 0, (size_t)n0 * 16));
    B.s = s;  // (from here on the sink is unset on every way out)
    uint64_t total = 0;
    if (rays_out) *rays_out = 0;
    // one pass: the render with the sink set; its pixels are then in d_out, its rays added to the total
    auto pass = [&](const mrt_render_desc* dk, const uint32_t* d_slots) -> mrt_status {
        s->mom = B.m;
        s->mom_slots = d_slots;
        s->trust_pixels = d_slots != nullptr;  // a refinement pass: the list is this call's own
        bool cancelled = false;
        const mrt_status st = render_wait(s, dk, cancel, &cancelled);
        s->mom = nullptr;
        s->mom_slots = nullptr;
        s->trust_pixels = false;
        if (st) return st;
        uint64_t rays = 0;
        HIPCHK(hipMemcpy(&rays, s->d_rays, 8, hipMemcpyDeviceToHost));
        total += rays;
        if (rays_out) *rays_out = total;
        if (cancelled) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (partial image)");
        return MRT_OK;
    };
    mrt_status st = pass(d, nullptr);
    if (st) return st;
    HIPCHK(hipMemcpy(B.C, s->d_out.p, (size_t)n0 * 16, hipMemcpyDeviceToDevice));
    float N = (float)(d->sqrt_samples * d->sqrt_samples);
    std::vector<float> hm((size_t)n0 * 4);
    std::vector<uint32_t> list;
    for (uint32_t k = 1; k <= p->max_passes; k++) {
        if (cancel && *cancel) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (between passes)");
        HIPCHK(hipMemcpy(hm.data(), B.m, hm.size() * 4, hipMemcpyDeviceToHost));
        const std::vector<uint32_t> slots = mrt_internal_refine_slots(hm.data(), n0, p->atol, p->rtol);
        if (slots.empty()) break;
        list.resize(slots.size());
        for (size_t j = 0; j < slots.size(); j++) list[j] = px0[slots[j]];
        HIPCHK(hipMemcpy(B.slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
        const mrt_render_desc dk = mrt_internal_adaptive_pass(d, k, list.data(), (uint32_t)list.size());
        if ((st = pass(&dk, B.slots))) return st;
        const float nsf = (float)(dk.sqrt_samples * dk.sqrt_samples);
        if ((st = mrt_internal_merge_enqueue((const float*)s->d_out.p, (uint32_t)slots.size(), B.slots, B.C, N, nsf, nullptr))) return st;
        HIPCHK(hipStreamSynchronize(nullptr));  // (the next pass may regrow d_out; the slot map is rewritten)
        N = N + nsf;
    }
    std::vector<float> local((size_t)n0 * (moments_out ? 8 : 4));  // C, then m: one copy
    HIPCHK(hipMemcpy(local.data(), B.C, local.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < px0.size(); i++) memcpy(rgb_out + (size_t)px0[i] * 4, &local[i * 4], 16);
    if (moments_out)
        for (size_t i = 0; i < px0.size(); i++) memcpy(moments_out + (size_t)px0[i] * 4, &local[((size_t)n0 + i) * 4], 16);
    return MRT_OK;
}

extern "C" mrt_status mrt_render_adaptive(mrt_scene* s, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out,
                                          float* moments_out, uint64_t* rays_out, const volatile int* cancel) {
    if (mrt_status st = mrt_internal_adaptive_check(s, d, p, rgb_out)) return st;
    if (s->cpu) return mrt_cpu_render_adaptive(s->cpu, d, p, rgb_out, moments_out, rays_out, cancel);
    return render_adaptive_gpu(s, d, p, rgb_out, moments_out, rays_out, cancel);
}

// ---- first-hit feature buffers (include/mrt.h "feature buffers and denoise") ----
// what both entry points read of the desc; flags: 0 or MRT_RF_FAST (ignored: the buffers come from
// the exact arithmetic's hit code on both backends)
static mrt_status aux_check(const char* who, const mrt_scene* s, const mrt_render_desc* d, const void* normal, const void* albedo) {
    if (!s || !d || !normal || !albedo) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    if (d->width == 0 || d->height == 0 || d->sqrt_samples == 0 || (d->world && d->rank >= d->world))
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": bad desc").c_str());
    if (d->flags & ~MRT_RF_FAST)
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": flags other than MRT_RF_FAST").c_str());
    return mrt_internal_check_pixels(d);
}

extern "C" mrt_status mrt_render_aux_device(mrt_scene* s, const mrt_render_desc* d, float* d_normal, float* d_albedo, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_aux_device");
    mrt_status st = aux_check("mrt_render_aux_device", s, d, d_normal, d_albedo);
    if (st) return st;
    // the pixel table and the sample grid are the render's (mrt_prepare); nothing else of the
    // workspace is used, and no flag of the render path applies
    mrt_render_desc dc = *d;
    dc.flags = 0;
    if ((st = mrt_prepare(s, &dc))) return st;
    if (s->npix == 0) return MRT_OK;
    const aux_kernel_t fn = aux_kernel_table().kernel[s->variant];
    const PathLaunch& PL = s->pl[0];  // the exact build's stack sizes
    const PathParams P = launch_params(s, PL, d);
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipStream_t q = (hipStream_t)stream;
    hipLaunchKernelGGL(fn, dim3((s->npix + 63u) / 64u), dim3(64), lds_bytes, q, P, (float4*)d_normal, (float4*)d_albedo);
    HIPCHK(hipGetLastError());
    // a later change of the pixel table or the sample grid waits for this kernel (quiesce); not
    // while `stream` is being captured: nothing runs now, and a captured event cannot be waited for
    // on the host (the caller keeps the layout while it replays the graph)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (q) HIPCHK(hipStreamIsCapturing(q, &cap));
    if (cap == hipStreamCaptureStatusNone) {
        HIPCHK(hipEventRecord(s->ev_aux, q));
        s->ev_aux_pending = true;
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_render_aux(mrt_scene* s, const mrt_render_desc* d, float* normal_out, float* albedo_out) {
    mrt_status st = aux_check("mrt_render_aux", s, d, normal_out, albedo_out);
    if (st) return st;
    if (s->cpu) return mrt_cpu_render_aux(s->cpu, d, normal_out, albedo_out);
    mrt_render_desc dc = *d;
    dc.flags = 0;
    if ((st = mrt_prepare(s, &dc))) return st;
    const std::vector<uint32_t> px = mrt_internal_local_pixels(d);
    if (px.empty()) return MRT_OK;
    float* dev = nullptr;  // normal, then albedo: n_local float4 each
    if (hipMalloc((void**)&dev, px.size() * 32) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "mrt_render_aux: device buffers");
    std::vector<float> local(px.size() * 8);
    st = mrt_render_aux_device(s, d, dev, dev + px.size() * 4, nullptr);
    hipError_t e = hipSuccess;
    if (!st) e = hipMemcpy(local.data(), dev, local.size() * 4, hipMemcpyDeviceToHost);  // (waits for the kernel)
    (void)hipFree(dev);
    if (st) return st;
    if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
    s->ev_aux_pending = false;
    for (size_t i = 0; i < px.size(); i++) {
        memcpy(normal_out + (size_t)px[i] * 4, &local[i * 4], 16);
        memcpy(albedo_out + (size_t)px[i] * 4, &local[(px.size() + i) * 4], 16);
    }
    return MRT_OK;
}

// ---- ray queries (include/mrt.h "ray queries") ----
// One mrt_cast_kernel launch over device records: the scene's variant from the cast table, one-wave
// groups with the exact build's walk stacks (the aux launch's).  It reads the scene tables and the
// rays and writes the hits; nothing of the render workspace, so it needs no mrt_prepare, takes no
// part in quiesce() and leaves no event behind.
static mrt_status cast_launch(mrt_scene* s, const mrt_ray* d_rays, uint32_t n, uint64_t seed, mrt_hit* d_hits, hipStream_t q) {
    CastParams P{};
    P.sc = s->S;
    P.rays = (const CastRay*)d_rays;
    P.hits = (CastHit*)d_hits;
    P.seed = seed;
    P.n = n;
    P.lds_frames = s->lds_frames;
    P.lds_rays = s->lds_rays;
    P.lds_mesh = s->lds_mesh;
    P.lds_save = s->pl[0].lds_save;
    const cast_kernel_t fn = cast_kernel_table().kernel[s->variant];
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipLaunchKernelGGL(fn, dim3((uint32_t)(((uint64_t)n + 63u) / 64u)), dim3(64), lds_bytes, q, P);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

extern "C" mrt_status mrt_cast_rays_device(mrt_scene* s, const mrt_ray* d_rays, uint32_t n, uint64_t seed, mrt_hit* d_hits, void* stream) {
    MRT_GPU_ONLY(s, "mrt_cast_rays_device");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: null");
    if (n == 0) return MRT_OK;
    if (!d_rays || !d_hits) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: null");
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: records not 16-byte aligned");
    HIPCHK(hipSetDevice(s->device));
    return cast_launch(s, d_rays, n, seed, d_hits, (hipStream_t)stream);
}

extern "C" mrt_status mrt_cast_rays(mrt_scene* s, const mrt_ray* rays, uint32_t n, uint64_t seed, mrt_hit* hits) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays: null");
    if (n == 0) return MRT_OK;
    if (!rays || !hits) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays: null");
    if (s->cpu) return mrt_cpu_cast_rays(s->cpu, rays, n, seed, hits);
    HIPCHK(hipSetDevice(s->device));
    // staged in pieces of at most 2^20 rays (80 MiB of device records); piece k0 casts with seed + k0
    const uint32_t piece = std::min(n, 1u << 20);
    if (!s->cast_stream) HIPCHK(hipStreamCreateWithFlags(&s->cast_stream, hipStreamNonBlocking));
    const size_t need = (size_t)piece * (sizeof(mrt_ray) + sizeof(mrt_hit));
    if (s->d_cast_cap < need) {
        if (s->d_cast) (void)hipFree(s->d_cast);
        s->d_cast = nullptr;
        s->d_cast_cap = 0;
        if (hipMalloc(&s->d_cast, need) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "mrt_cast_rays: device records");
        s->d_cast_cap = need;
    }
    mrt_ray* const d_rays = (mrt_ray*)s->d_cast;
    mrt_hit* const d_hits = (mrt_hit*)((char*)s->d_cast + (size_t)piece * sizeof(mrt_ray));  // (48 * piece: 16-byte aligned)
    for (uint64_t k0 = 0; k0 < n; k0 += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - k0);
        HIPCHK(hipMemcpyAsync(d_rays, rays + k0, (size_t)m * sizeof(mrt_ray), hipMemcpyHostToDevice, s->cast_stream));
        if (mrt_status st = cast_launch(s, d_rays, m, seed + k0, d_hits, s->cast_stream)) return st;
        HIPCHK(hipMemcpyAsync(hits + k0, d_hits, (size_t)m * sizeof(mrt_hit), hipMemcpyDeviceToHost, s->cast_stream));
        HIPCHK(hipStreamSynchronize(s->cast_stream));
    }
    return MRT_OK;
}

// ---- radiance queries (include/mrt.h "radiance queries") ----
// The probe kernel's full grid in waves: kProbeWavesPerCU per CU of the scene's device, whatever the
// variant; a wave's level rows are 64 lanes x max(max_bounces, 1) float4.
static uint64_t probe_full_waves(const mrt_scene* s) { return (uint64_t)s->n_cu * kProbeWavesPerCU; }
static uint64_t probe_wave_bytes(uint32_t max_bounces) { return 64ull * std::max<uint32_t>(max_bounces, 1u) * 16ull; }

// One mrt_probe_kernel launch over device records: the scene's variant from the probe table, one-wave
// groups with the exact build's walk stacks (the cast launch's), `waves` of them, each lane striding
// over the records.  It reads the scene tables and the probes and writes the records and the level
// rows of its own lanes; nothing of the render workspace, so it needs no mrt_prepare, takes no part in
// quiesce() and leaves no event behind.
static mrt_status probe_launch(mrt_scene* s, const mrt_probe* d_probes, uint32_t n, uint32_t max_bounces, mrt_radiance* d_out, void* d_work,
                               uint32_t waves, hipStream_t q) {
    ProbeParams P{};
    P.sc = s->S;
    P.probes = (const ProbeRec*)d_probes;
    P.out = (ProbeOut*)d_out;
    P.lev = (float4*)d_work;
    P.n = n;
    P.max_bounces = max_bounces;
    P.lev_rows = std::max<uint32_t>(max_bounces, 1u);
    P.lds_frames = s->lds_frames;
    P.lds_rays = s->lds_rays;
    P.lds_mesh = s->lds_mesh;
    P.lds_save = s->pl[0].lds_save;
    const probe_kernel_t fn = probe_kernel_table().kernel[s->variant];
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipLaunchKernelGGL(fn, dim3(waves), dim3(64), lds_bytes, q, P);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

// the waves a launch over n records runs with `work_bytes` of level rows (0: fewer than one wave's)
static uint32_t probe_waves(const mrt_scene* s, uint32_t n, uint32_t max_bounces, uint64_t work_bytes) {
    const uint64_t have = work_bytes / probe_wave_bytes(max_bounces);
    return (uint32_t)std::min({have, probe_full_waves(s), ((uint64_t)n + 63u) / 64u});
}

extern "C" mrt_status mrt_trace_rays_workspace(const mrt_scene* s, uint32_t max_bounces, uint64_t* bytes_full, uint64_t* bytes_min) {
    MRT_GPU_ONLY(s, "mrt_trace_rays_workspace");
    if (!s || !bytes_full || !bytes_min) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_workspace: null");
    *bytes_min = probe_wave_bytes(max_bounces);
    *bytes_full = probe_full_waves(s) * probe_wave_bytes(max_bounces);
    return MRT_OK;
}

extern "C" mrt_status mrt_trace_rays_device(mrt_scene* s, const mrt_probe* d_probes, uint32_t n, uint32_t max_bounces, mrt_radiance* d_out,
                                            void* d_work, uint64_t work_bytes, void* stream) {
    MRT_GPU_ONLY(s, "mrt_trace_rays_device");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: null");
    if (n == 0) return MRT_OK;
    if (!d_probes || !d_out || !d_work) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: null");
    if (((uintptr_t)d_probes | (uintptr_t)d_out | (uintptr_t)d_work) & 15u)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: records or workspace not 16-byte aligned");
    if (work_bytes < probe_wave_bytes(max_bounces))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: workspace below one wave's level rows (mrt_trace_rays_workspace)");
    HIPCHK(hipSetDevice(s->device));
    return probe_launch(s, d_probes, n, max_bounces, d_out, d_work, probe_waves(s, n, max_bounces, work_bytes), (hipStream_t)stream);
}

extern "C" mrt_status mrt_trace_rays(mrt_scene* s, const mrt_probe* probes, uint32_t n, uint32_t max_bounces, mrt_radiance* out,
                                     uint64_t* rays_out) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays: null");
    if (n == 0) {
        if (rays_out) *rays_out = 0;
        return MRT_OK;
    }
    if (!probes || !out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays: null");
    if (s->cpu) {
        if (mrt_status st = mrt_cpu_trace_rays(s->cpu, probes, n, max_bounces, out)) return st;
    } else {
        HIPCHK(hipSetDevice(s->device));
        // staged in pieces of at most MRT_TRACE_PIECE records (64 MiB of device records); the level rows
        // of the waves a piece can occupy, at most the full grid's
        uint32_t piece_max = MRT_TRACE_PIECE;
        if (const char* e = getenv("MRT_TRACE_PIECE_RECORDS"))  // test hook: a small piece (tests/test_probe_gpu.py)
            if (*e) piece_max = std::max(1u, std::min((uint32_t)strtoul(e, nullptr, 0), MRT_TRACE_PIECE));
        const uint32_t piece = std::min(n, piece_max);
        if (!s->trace_stream) HIPCHK(hipStreamCreateWithFlags(&s->trace_stream, hipStreamNonBlocking));
        auto grow = [&](void** p, size_t* cap, size_t need, const char* what) {
            if (*cap >= need) return MRT_OK;
            if (*p) (void)hipFree(*p);
            *p = nullptr;
            *cap = 0;
            if (hipMalloc(p, need) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, what);
            *cap = need;
            return MRT_OK;
        };
        if (mrt_status st = grow(&s->d_trace, &s->d_trace_cap, (size_t)piece * (sizeof(mrt_probe) + sizeof(mrt_radiance)), "mrt_trace_rays: device records"))
            return st;
        const uint64_t waves = std::min<uint64_t>(probe_full_waves(s), ((uint64_t)piece + 63u) / 64u);
        const uint64_t work_bytes = waves * probe_wave_bytes(max_bounces);
        if (mrt_status st = grow(&s->d_trace_work, &s->d_trace_work_cap, (size_t)work_bytes, "mrt_trace_rays: level workspace")) return st;
        mrt_probe* const d_probes = (mrt_probe*)s->d_trace;
        mrt_radiance* const d_out = (mrt_radiance*)((char*)s->d_trace + (size_t)piece * sizeof(mrt_probe));  // (48 * piece: 16-byte aligned)
        for (uint64_t k0 = 0; k0 < n; k0 += piece) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - k0);
            HIPCHK(hipMemcpyAsync(d_probes, probes + k0, (size_t)m * sizeof(mrt_probe), hipMemcpyHostToDevice, s->trace_stream));
            if (mrt_status st = probe_launch(s, d_probes, m, max_bounces, d_out, s->d_trace_work, probe_waves(s, m, max_bounces, work_bytes), s->trace_stream))
                return st;
            HIPCHK(hipMemcpyAsync(out + k0, d_out, (size_t)m * sizeof(mrt_radiance), hipMemcpyDeviceToHost, s->trace_stream));
            HIPCHK(hipStreamSynchronize(s->trace_stream));
        }
    }
    if (rays_out) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; i++) total += out[i].rays;
        *rays_out = total;
    }
    return MRT_OK;
}

// the worker threads' join (main.cpp:490-493) as stream order: `stream` waits for the context's
// last render, including a fold on the context's own stream (MRT_RF_FOLD_ASYNC)
int mrt_internal_scene_device(const mrt_scene* s) { return s->cpu ? MRT_DEVICE_CPU : s->device; }

extern "C" mrt_status mrt_render_join(mrt_scene* s, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_join");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_join: null");
    if (!s->ev_done) return MRT_OK;  // no render yet
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, s->ev_done, 0));
    return MRT_OK;
}

// ---- the camera of an uploaded scene (include/mrt.h "camera and temporal accumulation") ----
// Every kernel reads the camera through DScene::camp at each path start (mrt_shade.h camera_ray);
// DScene::cam, the copy inside the struct (the host's s->S, handed to every launch by value, and the
// uploaded d_S), is read by no kernel and is kept equal to it.  Nothing else of an upload depends on
// the camera: the scene tables, the variant choice and the Cornell hit table do not read it.
static mrt_status camera_check(const char* who, const mrt_scene* s, const mrt_camera* cam) {
    if (!s || !cam) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    const float* f = (const float*)cam;
    for (size_t i = 0; i < sizeof(mrt_camera) / 4; i++)
        if (!std::isfinite(f[i])) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": a camera with a non-finite field").c_str());
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_set_camera(mrt_scene* s, const mrt_camera* cam) {
    if (mrt_status st = camera_check("mrt_scene_set_camera", s, cam)) return st;
    if (s->cpu) {
        mrt_cpu_set_camera(s->cpu, cam);
        return MRT_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    if (mrt_status st = quiesce(s)) return st;  // the context's last render (its fold included) and feature buffers
    HIPCHK(hipMemcpy(const_cast<mrt_camera*>(s->S.camp), cam, sizeof(mrt_camera), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char*)s->d_S + offsetof(DScene, cam), cam, sizeof(mrt_camera), hipMemcpyHostToDevice));
    s->S.cam = *cam;
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_set_camera_device(mrt_scene* s, const mrt_camera* cam, void* stream) {
    MRT_GPU_ONLY(s, "mrt_scene_set_camera_device");
    if (mrt_status st = camera_check("mrt_scene_set_camera_device", s, cam)) return st;
    HIPCHK(hipSetDevice(s->device));
    if (mrt_status st = mrt_internal_camera_store(cam, const_cast<mrt_camera*>(s->S.camp), (char*)s->d_S + offsetof(DScene, cam), stream)) return st;
    s->S.cam = *cam;
    return MRT_OK;
}

extern "C" mrt_status mrt_render_debug(mrt_scene* s, float* path_rgb, uint32_t* path_rays, uint64_t n_paths) {
    MRT_GPU_ONLY(s, "mrt_render_debug");
    if (!s || !(s->wdesc.flags & MRT_RF_PATH_DEBUG) || n_paths != s->last_paths)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_debug: no debug render of that size");
    HIPCHK(hipSetDevice(s->device));
    if (path_rgb) HIPCHK(hipMemcpy(path_rgb, s->d_rad.p, n_paths * 12, hipMemcpyDeviceToHost));
    if (path_rays) HIPCHK(hipMemcpy(path_rays, s->d_path_rays.p, n_paths * 4, hipMemcpyDeviceToHost));
    return MRT_OK;
}

// work_queue::getPercentDone (work_queue.cpp:142-175): paths handed out over all paths of the
// render, callable from another host thread while the render runs.  Needs no GPU work: a finished
// launch counts whole (its stop event), a running one by the snapshot of its work counter that
// the path kernel stores into host memory, a launch not yet started as 0.
extern "C" mrt_status mrt_progress(mrt_scene* s, float* pct) {
    if (!s || !pct) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_progress: null");
    *pct = 0.0f;
    if (s->cpu) return mrt_cpu_progress(s->cpu, pct);
    std::lock_guard<std::mutex> lk(s->prog_mu);
    const size_t n = s->n_chunks.load(std::memory_order_acquire);
    if (n == 0 || !s->h_prog || s->h_prog_cap < s->prog_base + n || s->ev.size() < 2 * n || s->h_seen.size() < n * MRT_NPART) return MRT_OK;  // not started
    double done = 0, total = 0;
    for (size_t k = 0; k < n; k++) {
        total += (double)s->chunk_paths[k];
        if (hipEventQuery(s->ev[2 * k + 1]) == hipSuccess) {
            done += (double)s->chunk_paths[k];
        } else if (hipEventQuery(s->ev[2 * k]) == hipSuccess) {
            // one snapshot per work partition (the paths it has handed out); snapshots from
            // different waves land out of order: report the largest seen so far
            const uint64_t np = s->chunk_paths[k];
            for (uint32_t j = 0; j < MRT_NPART; j++) {
                uint64_t c = __atomic_load_n(&s->h_prog[(s->prog_base + k) * MRT_NPART + j], __ATOMIC_RELAXED);
                c = std::max(c, s->h_seen[k * MRT_NPART + j]);
                s->h_seen[k * MRT_NPART + j] = c;
                done += (double)std::min<uint64_t>(c, np * (j + 1) / MRT_NPART - np * j / MRT_NPART);
            }
        }
    }
    *pct = total > 0 ? (float)std::min(100.0, done * 100.0 / total) : 0.0f;
    return MRT_OK;
}

// The UI thread's view of G_linearBackBuffer (main.cpp:387-444) without stopping the render: the
// newest snapshot whose sequence word was even, and unchanged, around the copy out of pinned memory.
extern "C" mrt_status mrt_preview(mrt_scene* s, float* rgb_out, uint32_t* samples_done) {
    if (!s || !rgb_out || !samples_done) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_preview: null");
    *samples_done = 0;
    if (s->cpu) return mrt_cpu_preview(s->cpu, rgb_out, samples_done);
    std::lock_guard<std::mutex> lk(s->prog_mu);
    if (!s->h_seq || !s->h_prev || s->prev_px.empty()) return MRT_OK;  // no preview render yet
    std::vector<float4> snap(s->prev_px.size());
    for (int tries = 0; tries < 1000; tries++) {
        const uint32_t a = __atomic_load_n(s->h_seq, __ATOMIC_ACQUIRE);
        if (a == 0) return MRT_OK;  // nothing folded yet
        if (a & 1u) {               // a copy is landing: the previous one is being overwritten
            usleep(50);
            continue;
        }
        const uint32_t n = __atomic_load_n(s->h_seq + 1, __ATOMIC_ACQUIRE);
        memcpy(snap.data(), s->h_prev, snap.size() * 16);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (__atomic_load_n(s->h_seq, __ATOMIC_ACQUIRE) != a) continue;  // torn: retry
        for (size_t i = 0; i < snap.size(); i++) memcpy(rgb_out + (size_t)s->prev_px[i] * 4, &snap[i], 16);
        *samples_done = n;
        return MRT_OK;
    }
    return MRT_OK;  // the render outran every attempt: report nothing rather than a torn image
}

extern "C" mrt_status mrt_set_worker_seeds(mrt_scene* s, uint32_t n_threads, const uint64_t* initstate, const uint64_t* initseq) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_set_worker_seeds: null");
    if (!s->cpu)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_set_worker_seeds: the reference's per-thread RNG order is a CPU-backend mode "
                                                  "(the GPU keys its PCG streams per path)");
    return mrt_cpu_set_worker_seeds(s->cpu, n_threads, initstate, initseq);
}

extern "C" mrt_status mrt_scene_kernel_info(const mrt_scene* s, mrt_kernel_info* out) {
    if (!s || !out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_kernel_info: null");
    out->features = s->features;
    if (s->cpu) {  // the host instantiation that runs it (mrt_cpu.hip), threads of the last render
        float ms;
        uint32_t threads = 0;
        mrt_cpu_last_ms(s->cpu, &ms, &threads);
        *out = mrt_kernel_info{};
        out->features = s->features;
        out->kernel_features = (s->features & FT_LIN) ? (FT_LIN | FT_ALL) : FT_ALL;
        out->grid = threads;
        return MRT_OK;
    }
    out->kernel_features = kVariants[s->variant];
    const PathLaunch& L = s->pl[s->last_numerics];
    out->lds_bytes = (uint32_t)L.lds_bytes;
    out->grid = s->last_grid ? s->last_grid : (uint32_t)L.grid;  // (an async launch with side slots: fewer groups)
    out->prog_ops = s->prog_ops;
    out->vgprs = L.vgprs;
    out->wg = L.wg;
    out->tree_nodes = L.tree_n;  // BvhWide nodes per workgroup
    out->build = s->last_numerics == 0 ? MRT_BUILD_EXACT
               : L.fn == kernel_table_fast_pex().kernel[s->variant] ? MRT_BUILD_PATH_EXACT
               : L.fn == kernel_table_fast_ftz().kernel[s->variant] ? MRT_BUILD_FAST_FTZ
                                                                     : MRT_BUILD_FAST;
    out->n_cu = s->n_cu;
    out->handed_over = 0;
    out->handover_lost = 0;
    if (s->d_counter) {
        // after the scene's last render, its fold included: ev_done is recorded on the render's
        // stream (or the context's fold stream), which the legacy null stream of a plain hipMemcpy
        // is not ordered after
        HIPCHK(hipSetDevice(s->device));
        if (s->ev_done_pending) HIPCHK(hipEventSynchronize(s->ev_done));
        uint64_t n[6] = {};
        if (hipMemcpy(n, s->d_counter, sizeof n, hipMemcpyDeviceToHost) != hipSuccess)
            return mrt_internal_fail(MRT_ERR_HIP, "mrt_scene_kernel_info: counter read");
        out->handed_over = n[0];
        out->handover_lost = n[5];
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_kernel_ms(mrt_scene* s, float* path_ms, uint32_t* launches) {
    if (!s || !path_ms) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_kernel_ms: null");
    if (s->cpu) {  // wall time of the last CPU render
        if (launches) *launches = 1;
        return mrt_cpu_last_ms(s->cpu, path_ms, nullptr);
    }
    HIPCHK(hipSetDevice(s->device));
    float total = 0;
    for (uint32_t k = 0; k < s->n_launch; k++) {
        HIPCHK(hipEventSynchronize(s->ev[2 * k + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]));
        total += ms;
    }
    *path_ms = total;
    if (launches) *launches = s->n_launch;
    return MRT_OK;
}
