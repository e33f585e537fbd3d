/* mrt_adaptive.h -- per-pixel sample moments and the decisions of the adaptive render built on them
 * (mrt_moments, mrt_render_adaptive in mrt.h), written once for the host and the device kernels so
 * both produce the same bits: IEEE add / mul / div / sqrt in float32 without contraction
 * (-ffp-contract=off).
 *
 * Per pixel one float4  m = (sum l, sum l^2, n_finite, N_spent)  over the samples' luminance
 *   l = (L.x * 0.212655f + L.y * 0.715158f) + L.z * 0.072187f,
 * added in sample order.  A sample with a non-finite channel counts in N_spent only.  Raw sums, not
 * Welford's update: the state stays one float4 that resumes across launch chunks and passes; the
 * cancellation error of sum l^2 / n - mean^2 is about 1e-4 of the variance for the luminances of a
 * render, far below any useful tolerance.
 *
 *   mean = m.x / m.z
 *   var  = m.y / m.z - mean * mean, and 0 where that is < 0 (a NaN stays a NaN)
 *   se   = sqrtf(var / (m.z - 1))      -- the standard error of the mean; +inf if m.z < 2
 *   refine = !(se <= atol + rtol * mean)
 * so a NaN or infinite se (overflowed squares, fewer than two finite samples) refines.
 *
 * The adaptive render's merge of a refinement pass's finished pixel c (nsf = its sample count as a
 * float) into the running colour C over N samples:  C = C + (c - C) * (nsf / (N + nsf)), per channel.
 */
#ifndef MRT_ADAPTIVE_H
#define MRT_ADAPTIVE_H
#include "mrt_mathfn.h"

/* one pixel's moments (or colour): 16 bytes, loaded and stored whole (one 128-bit access on the
 * device, where the buffers are 16-byte aligned) */
#if defined(__HIP_DEVICE_COMPILE__)
typedef struct __attribute__((aligned(16))) mrt_m4 { float x, y, z, w; } mrt_m4;
#else
typedef struct mrt_m4 { float x, y, z, w; } mrt_m4;
#endif

MRT_HD int mrt_moments_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

MRT_HD mrt_m4 mrt_moments_add(mrt_m4 m, float Lx, float Ly, float Lz) {
    m.w = m.w + 1.0f;
    if (mrt_moments_finite(Lx) && mrt_moments_finite(Ly) && mrt_moments_finite(Lz)) {
        const float l = (Lx * 0.212655f + Ly * 0.715158f) + Lz * 0.072187f;
        m.x = m.x + l;
        m.y = m.y + l * l;
        m.z = m.z + 1.0f;
    }
    return m;
}

MRT_HD float mrt_moments_mean(mrt_m4 m) { return m.x / m.z; }

MRT_HD float mrt_moments_se(mrt_m4 m) {
    if (m.z < 2.0f) return __builtin_inff();
    const float mean = m.x / m.z;
    float var = m.y / m.z - mean * mean;
    if (var < 0.0f) var = 0.0f;
    return sqrtf(var / (m.z - 1.0f));
}

MRT_HD int mrt_moments_refine(mrt_m4 m, float atol, float rtol) {
    const float se = mrt_moments_se(m);
    return !(se <= atol + rtol * mrt_moments_mean(m));
}

/* one channel of the merge */
MRT_HD float mrt_adaptive_merge(float C, float c, float N, float nsf) { return C + (c - C) * (nsf / (N + nsf)); }

#endif
