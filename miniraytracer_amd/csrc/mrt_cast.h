// mrt_cast.h -- batched ray queries (include/mrt.h "ray queries"): what one caller ray yields,
// written once for the device kernel (mrt_cast.hip, mrt_cast_kernel<F>) and the CPU backend
// (mrt_cpu.hip, mrt_cpu_cast_rays), and the interface between mrt_cast.hip and the launch in
// mrt_query.hip.  Like the feature buffers (mrt_aux.h) the kernels live in a translation unit of
// their own, built under the exact numerics contract, with a table of their own: the path-kernel
// objects (mrt_kernels.hip, the KernelTable of mrt_launch.h) do not change with them.
#pragma once
#include "../../include/mrt.h"
#include "mrt_launch.h"

namespace mrtd {

// mrt_ray and mrt_hit as the kernel moves them: three and two 16-byte words
struct CastRay {
    float4 ot;  // o.xyz, time
    float4 dm;  // d.xyz, tmax
    uint4 fl;   // inside, reserved[3]
};
struct CastHit {
    uint4 tp;  // t, p.xyz (float bits)
    uint4 nm;  // n.xyz (float bits), mat
};
static_assert(sizeof(CastRay) == sizeof(mrt_ray) && sizeof(CastHit) == sizeof(mrt_hit), "the ABI's records");

// the miss record: (+inf, 0,0,0, 0,0,0, MRT_NO_HIT)
MRT_DFN CastHit cast_miss() { return CastHit{make_uint4(0x7F800000u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, MRT_NO_HIT)}; }

// Ray i of a batch: the reference's ray(o, d, time, inside) (ray.h:18-56: make_ray normalises d and
// takes the direction mask from the argument), objects->hit(r, 0.001f, FLT_MAX) through the scene's
// own hit code -- trace_segment's dispatch, the call aux_first_hit makes -- with a constant_volume on
// the way drawing from pcg32_srandom(seed_i, 4242), seed_i = seed + i (uint64 wrap), and the tmax
// rule: a hit is reported when it exists and t <= tmax (a NaN tmax compares false; t > 0.001 always).
template <uint32_t F>
MRT_DFN CastHit cast_one(const DScene& S, const CastRay& q, uint64_t seed_i, const LStack& Ls) {
    static_assert(!kBox6Walk<F>, "exact contract: no Cornell fast walk (its hit table is the path loop's)");
    PhaseClock ph{};
    Pcg rng;
    pcg_seed(rng, seed_i, 4242u);
    Ray r = make_ray(f3{q.ot.x, q.ot.y, q.ot.z}, f3{q.dm.x, q.dm.y, q.dm.z}, q.ot.w, q.fl.x != 0u ? 1 : 0);
    HitRec rec;
    bool hit;
    if constexpr (MRT_SIG_OF(F) != SIG_NONE) hit = scene_hit_sig<F>(S, r, 0.001f, rec, Ls);
    else if constexpr ((F & FT_LIN) != 0) hit = scene_hit_lin<F>(S, r, 0.001f, rec, Ls, rng, ph);
    else hit = scene_hit<F>(S, r, 0.001f, rec, rng, Ls);
    const float tmax = q.dm.w;
    if (!(hit && tmax > 0.001f && rec.t <= tmax)) return cast_miss();
    return CastHit{make_uint4(__float_as_uint(rec.t), __float_as_uint(rec.p.x), __float_as_uint(rec.p.y), __float_as_uint(rec.p.z)),
                   make_uint4(__float_as_uint(rec.n.x), __float_as_uint(rec.n.y), __float_as_uint(rec.n.z), rec.mat)};
}

// mrt_cast_kernel<F> per variant of kVariants (exact arithmetic): the scene first, as every kernel
// that runs the hit code takes it (kernarg memory, scalar-loaded)
struct CastParams {
    DScene sc;
    const CastRay* __restrict__ rays;  // n records, 16-byte aligned
    CastHit* __restrict__ hits;        // n records, 16-byte aligned
    uint64_t seed;
    uint32_t n;
    uint32_t lds_frames, lds_rays, lds_mesh, lds_save;  // LDS stack slots / words per lane, as PathParams
};
static_assert(offsetof(CastParams, sc) == kSceneArgOffset, "the scene opens the argument segment, as in PathParams");
typedef void (*cast_kernel_t)(CastParams);
struct CastTable {
    cast_kernel_t kernel[kNumVariants];
};
const CastTable& cast_kernel_table();

}  // namespace mrtd
