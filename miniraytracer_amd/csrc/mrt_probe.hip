// mrt_probe.hip -- radiance queries on the device (include/mrt.h "radiance queries"), built once
// under the exact numerics contract (MRT_FAST=0, -ffp-contract=off): the records are bit-for-bit the
// CPU backend's (mrt_cpu.hip runs the same mrt_probe.h code on the host).
//
// mrt_probe_kernel<F>: one-wave groups with the per-lane LDS stacks of the walk (lds_frames,
// lds_rays, lds_mesh, lds_save), as the cast kernel.  With T lanes in the grid, lane l owns records
// l, l + T, l + 2T, ...  One loop; an iteration runs one trace_segment for every lane that holds a
// path.  A lane whose path ended stores its 16-byte record and loads its next one (three 16-byte
// loads) in the same iteration: it does not wait for the wave's longest path.  The loop ends when no
// lane of the wave holds a path (ballot).  A lane past its last record touches no memory.  No atomics,
// no barrier: nothing is shared between lanes, and the ray total is summed by the caller from the
// records.
//
// Fold levels: all of them in HBM (LevStore<0>), one row of max(max_bounces, 1) float4 per grid lane
// in the caller's workspace, slot = the lane's global index.  None in LDS: a row's length here is the
// caller's max_bounces, not a constant of the kernel, the generic machine's variant already spends
// its LDS on walk stacks for deep graphs, and the traffic is one 16-byte store per diffuse or metal
// bounce plus the fold's loads at the path's end (four in flight, mrt_shade.h fold_levels).
//
// mrt_radiance_fold_kernel: one lane per group of records (include/mrt_radiance.h).
#include <hip/hip_runtime.h>
#include <cstring>
#include <utility>

#include "mrt_internal.h"
#include "mrt_probe.h"
#include "../../include/mrt_radiance.h"

using namespace mrtd;

#ifndef MRT_PROBE_HOST_ONLY  // (tools/probe_check.cpp builds the host fold alone, without device code)
template <uint32_t F>
__global__ void __launch_bounds__(64) mrt_probe_kernel(ProbeParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = blockIdx.x * 64u + lane;
    const uint32_t T = gridDim.x * 64u;  // (the host keeps the grid below 2^26 lanes)
    const LStack Ls = lds_stacks(WaveLds{P.lds_frames, P.lds_rays, P.lds_mesh, P.lds_save}, lds, lane);
    const LevStore<0> lev{(MRT_GLOBAL_AS v4f*)P.lev, P.lev_rows, slot, 0u};
    const DScene& S = P.sc;
    uint32_t i = slot;  // this lane's record; i < P.n while `active`
    bool active = i < P.n;
    PathState ps;
    auto start = [&]() {
        const ProbeRec* __restrict__ src = P.probes + i;
        ProbeRec q;
        q.ot = src->ot;
        q.di = src->di;
        q.rng = src->rng;
        probe_begin(ps, q);
    };
    if (active) start();
    while (__builtin_amdgcn_ballot_w64(active) != 0) {
        if (active) {
            ProbeOut o;
            if (probe_step<F>(S, ps, P.max_bounces, lev, Ls, &o)) {
                P.out[i].lr = o.lr;
                // the next record of this lane's stride, if there is one (no sum that could wrap)
                active = P.n - i > T;
                if (active) {
                    i += T;
                    start();
                }
            }
        }
    }
}

template <size_t... I>
static ProbeTable make_probe_table(std::index_sequence<I...>) {
    return ProbeTable{{mrt_probe_kernel<kVariants[I]>...}};
}
const ProbeTable& mrtd::probe_kernel_table() {
    static const ProbeTable t = make_probe_table(std::make_index_sequence<kNumVariants>{});
    return t;
}

// ---- mrt_radiance_fold: draw()'s pixel over groups of records, host and device from one definition ----
__global__ void __launch_bounds__(256) mrt_radiance_fold_kernel(const mrt_rad4* __restrict__ rad, uint32_t n_groups, uint32_t group,
                                                                float max_luminance, mrt_rgb4* __restrict__ rgb) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const mrt_rad4* q = rad + (size_t)g * group;
    mrt_rgb4 c{0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < group; k++) c = mrt_radiance_add(c, q[k]);
    rgb[g] = mrt_radiance_final(c, group, max_luminance);
}

mrt_status mrtd::probe_fold_enqueue(const mrt_radiance* d_rad, uint32_t n_groups, uint32_t group, float max_luminance, float* d_rgb,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(mrt_radiance_fold_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, stream, (const mrt_rad4*)d_rad, n_groups, group,
                       max_luminance, (mrt_rgb4*)d_rgb);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MRT_OK : mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
}

#endif  // MRT_PROBE_HOST_ONLY

extern "C" mrt_status mrt_radiance_fold(const mrt_radiance* rad, uint32_t n_groups, uint32_t group, float max_luminance, float* rgb) {
    if (group == 0) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_radiance_fold: group == 0");
    if (n_groups == 0) return MRT_OK;
    if (!rad || !rgb) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_radiance_fold: null");
    for (uint32_t g = 0; g < n_groups; g++) {
        mrt_rgb4 c{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < group; k++) {
            mrt_rad4 r;
            memcpy(&r, rad + (size_t)g * group + k, sizeof r);
            c = mrt_radiance_add(c, r);
        }
        c = mrt_radiance_final(c, group, max_luminance);
        memcpy(rgb + (size_t)g * 4, &c, sizeof c);
    }
    return MRT_OK;
}

#ifndef MRT_PROBE_HOST_ONLY
extern "C" mrt_status mrt_radiance_fold_device(const mrt_radiance* d_rad, uint32_t n_groups, uint32_t group, float max_luminance, float* d_rgb,
                                               void* stream) {
    if (group == 0) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_radiance_fold_device: group == 0");
    if (n_groups == 0) return MRT_OK;
    if (!d_rad || !d_rgb) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_radiance_fold_device: null");
    if (((uintptr_t)d_rad | (uintptr_t)d_rgb) & 15u) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_radiance_fold_device: records not 16-byte aligned");
    return probe_fold_enqueue(d_rad, n_groups, group, max_luminance, d_rgb, (hipStream_t)stream);
}
#endif  // MRT_PROBE_HOST_ONLY
