// mrt_aux.h -- first-hit feature buffers (include/mrt.h "feature buffers and denoise"): what one
// camera ray contributes, written once for the device kernel (mrt_aux.hip, mrt_aux_kernel<F>) and
// the CPU backend (mrt_cpu.hip), and the interface between mrt_aux.hip and the launch in
// mrt_query.hip.  The kernels live in a translation unit of their own, built under the exact
// numerics contract, with a table of their own: the path-kernel objects (mrt_kernels.hip, the
// KernelTable of mrt_launch.h) do not change with them.
#pragma once
#include "mrt_launch.h"

namespace mrtd {

// The sums of one pixel's samples, in sample order
struct AuxSum {
    float n[3], cov, a[3], depth;
};
MRT_DFN AuxSum aux_zero() { return AuxSum{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f}; }

// One camera ray (ps.r, with ps.rng where camera_ray left it): the scene hit of the render's first
// segment -- trace_segment's dispatch, tmin 0.001, a constant_volume drawing from the same stream
// position -- added to the pixel's sums.
template <uint32_t F>
MRT_DFN void aux_first_hit(const DScene& S, PathState& ps, const LStack& Ls, AuxSum& a) {
    static_assert(!kBox6Walk<F>, "exact contract: no Cornell fast walk (its hit table is the path loop's)");
    PhaseClock ph{};
    HitRec rec;
    bool hit;
    if constexpr (MRT_SIG_OF(F) != SIG_NONE) hit = scene_hit_sig<F>(S, ps.r, 0.001f, rec, Ls);
    else if constexpr ((F & FT_LIN) != 0) hit = scene_hit_lin<F>(S, ps.r, 0.001f, rec, Ls, ps.rng, ph);
    else hit = scene_hit<F>(S, ps.r, 0.001f, rec, ps.rng, Ls);
    f3 alb{0.0f, 0.0f, 0.0f};
    bool shaded = !hit;
    if (hit) {
        const DMat M = S.mats[rec.mat];
        shaded = M.kind == MRT_M_LIGHT;
        if (M.kind == MRT_M_DIELECTRIC) alb = f3{1.0f, 1.0f, 1.0f};
        else if (!shaded) alb = mat_color<F>(S, M, rec);
        const bool front = dot(rec.n, ps.r.d) < 0.0f;
        a.n[0] += front ? rec.n.x : -rec.n.x;
        a.n[1] += front ? rec.n.y : -rec.n.y;
        a.n[2] += front ? rec.n.z : -rec.n.z;
        a.cov += 1.0f;
        a.depth += rec.t;
    } else {
        a.n[0] += 0.0f;
        a.n[1] += 0.0f;
        a.n[2] += 0.0f;
        a.cov += 0.0f;
        a.depth += 0.0f;
    }
    if (shaded) {
        // a light's emitted term or the miss radiance: shade_hit's own (it returns before the bounce
        // limit is read and before anything scatters)
        ps.depth = 0;
        ps.nlev = 0;
        const LevStore<0> lev{nullptr, 0u, 0u, 0u};
        (void)shade_hit<F, 0>(S, ps, 0u, lev, hit, rec, &alb, ph);
    }
    a.a[0] += alb.x;
    a.a[1] += alb.y;
    a.a[2] += alb.z;
}

// the pixel's two float4: the sums divided by (float)ns
MRT_DFN void aux_finish(const AuxSum& a, uint32_t ns, float4* normal, float4* albedo) {
    const float n = (float)ns;
    *normal = make_float4(a.n[0] / n, a.n[1] / n, a.n[2] / n, a.cov / n);
    *albedo = make_float4(a.a[0] / n, a.a[1] / n, a.a[2] / n, a.depth / n);
}

// mrt_aux_kernel<F> per variant of kVariants (exact arithmetic): PathParams as the path kernel reads
// them for path_key_at / the LDS stacks, and the two outputs (npix float4 each, local-pixel order)
typedef void (*aux_kernel_t)(PathParams, float4*, float4*);
struct AuxTable {
    aux_kernel_t kernel[kNumVariants];
};
const AuxTable& aux_kernel_table();

}  // namespace mrtd
