// mrt_aux.hip -- the first-hit feature buffers on the device (include/mrt.h "feature buffers and
// denoise"), built once under the exact numerics contract (MRT_FAST=0, -ffp-contract=off): the
// buffers are bit-for-bit the CPU backend's (mrt_cpu.hip runs the same mrt_aux.h code on the host).
//
// mrt_aux_kernel<F>: one lane per local pixel; the lane runs the pixel's samples in order -- the
// path's own stream and camera ray (path_key_at, camera_ray, as mrt_retrace_kernel starts a path),
// then the scene's hit code once -- and keeps the eight sums in registers, so the fold order is
// fixed and nothing is atomic.  One-wave groups with the per-lane LDS stacks of the path kernels
// (lds_frames, lds_rays, lds_mesh, lds_save); two coalesced float4 stores per pixel.
#include <hip/hip_runtime.h>
#include <utility>

#include "mrt_aux.h"

using namespace mrtd;

template <uint32_t F>
__global__ void __launch_bounds__(64) mrt_aux_kernel(PathParams P, float4* __restrict__ normal, float4* __restrict__ albedo) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const LStack Ls = lds_stacks(WaveLds{P.lds_frames, P.lds_rays, P.lds_mesh, P.lds_save}, lds, lane);
    const DScene& S = P.sc;
    const uint32_t lp = blockIdx.x * 64u + lane;
    if (lp >= P.npix) return;
    AuxSum a = aux_zero();
    for (uint32_t s = 0; s < P.ns; s++) {
        PathState ps;
        float u, v;
        path_key_at(P, lp, s, ps.rng, &u, &v);
        ps.r = camera_ray(S, ps.rng, u, v);
        aux_first_hit<F>(S, ps, Ls, a);
    }
    float4 n4, a4;
    aux_finish(a, P.ns, &n4, &a4);
    normal[lp] = n4;
    albedo[lp] = a4;
}

template <size_t... I>
static AuxTable make_aux_table(std::index_sequence<I...>) {
    return AuxTable{{mrt_aux_kernel<kVariants[I]>...}};
}
const AuxTable& mrtd::aux_kernel_table() {
    static const AuxTable t = make_aux_table(std::make_index_sequence<kNumVariants>{});
    return t;
}
