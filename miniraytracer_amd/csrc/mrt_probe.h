// mrt_probe.h -- radiance queries (include/mrt.h "radiance queries"): what one caller record yields,
// written once for the device kernel (mrt_probe.hip, mrt_probe_kernel<F>) and the CPU backend
// (mrt_cpu.hip, mrt_cpu_trace_rays), and the interface between mrt_probe.hip and the launches in
// mrt_query.hip.  Like the ray queries (mrt_cast.h) the kernels live in a translation unit of their
// own, built under the exact numerics contract, with a table of their own: the path-kernel objects
// (mrt_kernels.hip, the KernelTable of mrt_launch.h) do not change with them.
#pragma once
#include "../../include/mrt.h"
#include "mrt_launch.h"

namespace mrtd {

// mrt_probe and mrt_radiance as the kernel moves them: three 16-byte words and one
struct ProbeRec {
    float4 ot;  // o.xyz, time
    uint4 di;   // d.xyz (float bits), inside
    uint4 rng;  // rng_state lo, hi, rng_inc lo, hi
};
struct ProbeOut {
    uint4 lr;  // L.xyz (float bits), rays
};
static_assert(sizeof(ProbeRec) == sizeof(mrt_probe) && sizeof(ProbeOut) == sizeof(mrt_radiance), "the ABI's records");
static_assert(offsetof(mrt_probe, d) == 16 && offsetof(mrt_probe, inside) == 28 && offsetof(mrt_probe, rng_state) == 32 &&
                  offsetof(mrt_probe, rng_inc) == 40 && offsetof(mrt_radiance, rays) == 12,
              "the ABI's records, word for word");

// The start of record q's path: the reference's ray(o, d, time, inside) (ray.h:18-56: make_ray
// normalises d and takes the direction mask from the argument), the stream's two words as given,
// trace(r, 0)'s depth.
MRT_DFN void probe_begin(PathState& ps, const ProbeRec& q) {
    ps.r = make_ray(f3{q.ot.x, q.ot.y, q.ot.z}, f3{__uint_as_float(q.di.x), __uint_as_float(q.di.y), __uint_as_float(q.di.z)}, q.ot.w,
                    q.di.w != 0u ? 1 : 0);
    ps.rng.state = (uint64_t)q.rng.x | ((uint64_t)q.rng.y << 32);
    ps.rng.inc = (uint64_t)q.rng.z | ((uint64_t)q.rng.w << 32);
    ps.depth = 0;
    ps.nlev = 0;
#if MRT_FWD_FOLD
    ps.T = f3{1.0f, 1.0f, 1.0f};
#endif
}

// One trace() call of the path (one segment, the call the render's path loop makes).  Returns true
// when the path has ended; *out is then its record: the levels folded deepest-first as the recursion
// returns (end_path), rays = the segments run.
template <uint32_t F>
MRT_DFN bool probe_step(const DScene& S, PathState& ps, uint32_t max_bounces, const LevStore<0>& lev, const LStack& Ls, ProbeOut* out) {
    static_assert(!kBox6Walk<F>, "exact contract: no Cornell fast walk (its hit table is the path loop's)");
    PhaseClock ph{};
    f3 L{0.0f, 0.0f, 0.0f};
    if (!trace_segment<F, 0>(S, ps, max_bounces, lev, Ls, &L, ph)) return false;
    L = end_path(ps, lev, L);
    out->lr = make_uint4(__float_as_uint(L.x), __float_as_uint(L.y), __float_as_uint(L.z), ps.rays());
    return true;
}

// trace(r, 0) of record q (main.cpp:66-118): segments until the path ends, at most max_bounces + 1.
// `lev` holds max(max_bounces, 1) level rows of this lane.
template <uint32_t F>
MRT_DFN ProbeOut probe_one(const DScene& S, const ProbeRec& q, uint32_t max_bounces, const LevStore<0>& lev, const LStack& Ls) {
    PathState ps;
    probe_begin(ps, q);
    ProbeOut out;
    while (!probe_step<F>(S, ps, max_bounces, lev, Ls, &out)) {
    }
    return out;
}

// mrt_probe_kernel<F> per variant of kVariants (exact arithmetic): the scene first, as every kernel
// that runs the hit code takes it (kernarg memory, scalar-loaded)
struct ProbeParams {
    DScene sc;
    const ProbeRec* __restrict__ probes;  // n records, 16-byte aligned
    ProbeOut* __restrict__ out;           // n records, 16-byte aligned
    float4* __restrict__ lev;             // fold levels, lane-major: [grid lane][lev_rows]
    uint32_t n;
    uint32_t max_bounces;
    uint32_t lev_rows;                                  // levels per lane: max(max_bounces, 1)
    uint32_t lds_frames, lds_rays, lds_mesh, lds_save;  // LDS stack slots / words per lane, as PathParams
};
static_assert(offsetof(ProbeParams, sc) == kSceneArgOffset, "the scene opens the argument segment, as in PathParams");
typedef void (*probe_kernel_t)(ProbeParams);
struct ProbeTable {
    probe_kernel_t kernel[kNumVariants];
};
const ProbeTable& probe_kernel_table();

// waves per CU of the kernel's full grid (four per SIMD: what a 128-VGPR kernel keeps resident)
static constexpr uint32_t kProbeWavesPerCU = 16u;

// mrt_radiance_fold_device: one lane per group (include/mrt_radiance.h), enqueued on `stream`
mrt_status probe_fold_enqueue(const mrt_radiance* d_rad, uint32_t n_groups, uint32_t group, float max_luminance, float* d_rgb, hipStream_t stream);

}  // namespace mrtd
