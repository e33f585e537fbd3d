// mrt_cast.hip -- batched ray queries on the device (include/mrt.h "ray queries"), built once under
// the exact numerics contract (MRT_FAST=0, -ffp-contract=off): the records are bit-for-bit the CPU
// backend's (mrt_cpu.hip runs the same mrt_cast.h code on the host).
//
// mrt_cast_kernel<F>: one lane per ray.  The lane loads its 48-byte ray as three 16-byte words, runs
// the scene's hit code once (cast_one) and stores its 32-byte record as two 16-byte words; a wave
// reads 3 KiB and writes 2 KiB of consecutive memory.  One-wave groups with the per-lane LDS stacks of
// the path kernels (lds_frames, lds_rays, lds_mesh, lds_save); a lane past n leaves before it
// touches LDS or memory.  No atomics, no barrier.
#include <hip/hip_runtime.h>
#include <utility>

#include "mrt_cast.h"

using namespace mrtd;

template <uint32_t F>
__global__ void __launch_bounds__(64) mrt_cast_kernel(CastParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 64u + lane;
    if (i >= P.n) return;
    const LStack Ls = lds_stacks(WaveLds{P.lds_frames, P.lds_rays, P.lds_mesh, P.lds_save}, lds, lane);
    const CastRay* __restrict__ src = P.rays + i;
    CastRay q;
    q.ot = src->ot;
    q.dm = src->dm;
    q.fl = src->fl;
    const CastHit h = cast_one<F>(P.sc, q, P.seed + (uint64_t)i, Ls);
    CastHit* __restrict__ dst = P.hits + i;
    dst->tp = h.tp;
    dst->nm = h.nm;
}

template <size_t... I>
static CastTable make_cast_table(std::index_sequence<I...>) {
    return CastTable{{mrt_cast_kernel<kVariants[I]>...}};
}
const CastTable& mrtd::cast_kernel_table() {
    static const CastTable t = make_cast_table(std::make_index_sequence<kNumVariants>{});
    return t;
}
