/* mrt_denoise.h -- one pass of the edge-avoiding a-trous filter (Dammertz et al. 2010), written once
 * for the host (mrt_denoise) and the device kernel (mrt_atrous_kernel) so both produce the same
 * bits: IEEE add / mul / div / sqrt without contraction (-ffp-contract=off) and the exp / pow of the
 * numerics contract (mrt_mathfn.h).
 *
 * Pass i = 0 .. iterations-1 has step = 2^i.  For pixel p the taps are q = p + step * (dx, dy),
 * dy = -2..2 outer, dx = -2..2 inner (that order is the summation order); taps outside the image
 * are skipped.  With k = {3/8, 1/4, 1/16} and h = k[|dx|] * k[|dy|] (exact in float):
 *
 *   n^     = n.xyz / sqrt(n.x^2 + n.y^2 + n.z^2)            (normal buffer; "zero" = squared length 0)
 *   w_n    = 1 if both normals are zero, 0 if exactly one is, else
 *            mrt_powf(max(0, n^_p . n^_q), sigma_normal)    (a dot product of exactly 0 gives exactly 0)
 *   e_z    = |z_p - z_q| / (max(z_p, z_q) * sigma_depth)    (z = albedo.w, the depth; 0 if both are 0)
 *   e_a    = |a_p - a_q|^2 * RN(1 / sigma_albedo^2)         (a = albedo.xyz)
 *   e_c    = |c_p - c_q|^2 * RN(1 / (sigma_color 2^-i)^2)   (c = the pass's input colour xyz)
 *   w      = (h * w_n) * mrt_expf(-((e_z + e_a) + e_c))     (= h w_n w_z w_a w_c, one exponential)
 *
 * The centre tap's weight is exactly h (9/64).  A tap with w_n == 0 is skipped (its weight is 0).
 * out.xyz = (sum w c) / (sum w); out.w = the input's w.
 */
#ifndef MRT_DENOISE_H
#define MRT_DENOISE_H
#include "mrt_mathfn.h"

/* what a pass needs besides the frames: sigma_color already scaled for the pass */
typedef struct mrt_atrous_pass {
    unsigned int width, height, step;
    float sigma_normal;
    float sigma_depth;
    float inv_sigma_albedo2; /* 1 / sigma_albedo^2 */
    float inv_sigma_color2;  /* 1 / (sigma_color * 2^-i)^2 */
} mrt_atrous_pass;

MRT_HD void mrt_atrous_pass_setup(unsigned int width, unsigned int height, unsigned int i, float sigma_color, float sigma_normal,
                                  float sigma_albedo, float sigma_depth, mrt_atrous_pass* ps) {
    float sc = sigma_color;
    for (unsigned int k = 0; k < i; k++) sc = sc * 0.5f;
    ps->width = width;
    ps->height = height;
    ps->step = 1u << i;
    ps->sigma_normal = sigma_normal;
    ps->sigma_depth = sigma_depth;
    ps->inv_sigma_albedo2 = 1.0f / (sigma_albedo * sigma_albedo);
    ps->inv_sigma_color2 = 1.0f / (sc * sc);
}

MRT_HD float mrt_atrous_k(int d) {
    d = d < 0 ? -d : d;
    return d == 0 ? 0.375f : (d == 1 ? 0.25f : 0.0625f);
}

/* one pixel of a frame: 16 bytes, loaded and stored whole (one 128-bit access on the device, where
 * frames are 16-byte aligned) */
#if defined(__HIP_DEVICE_COMPILE__)
typedef struct __attribute__((aligned(16))) mrt_f4 { float x, y, z, w; } mrt_f4;
#else
typedef struct mrt_f4 { float x, y, z, w; } mrt_f4;
#endif

/* pixel (x, y) of one pass; frames are row-major, one mrt_f4 per pixel */
MRT_HD mrt_f4 mrt_atrous_pixel(const mrt_atrous_pass* ps, const mrt_f4* rgb, const mrt_f4* normal, const mrt_f4* albedo, unsigned int x,
                               unsigned int y) {
    const unsigned long long W = ps->width;
    const unsigned long long p = (unsigned long long)y * W + x;
    const mrt_f4 cp = rgb[p], ap = albedo[p];
    mrt_f4 np = normal[p];
    const float lp = (np.x * np.x + np.y * np.y) + np.z * np.z;
    if (lp != 0.0f) {
        const float l = sqrtf(lp);
        np.x = np.x / l;
        np.y = np.y / l;
        np.z = np.z / l;
    }
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const long long qy = (long long)y + (long long)dy * (long long)ps->step;
        if (qy < 0 || qy >= (long long)ps->height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const long long qx = (long long)x + (long long)dx * (long long)ps->step;
            if (qx < 0 || qx >= (long long)ps->width) continue;
            const float h = mrt_atrous_k(dx) * mrt_atrous_k(dy);
            const unsigned long long q = (unsigned long long)qy * W + (unsigned long long)qx;
            const mrt_f4 cq = rgb[q];
            float w = h;
            if (q != p) {
                mrt_f4 nq = normal[q];
                const float lq = (nq.x * nq.x + nq.y * nq.y) + nq.z * nq.z;
                float wn;
                if (lp == 0.0f || lq == 0.0f) {
                    wn = (lp == 0.0f && lq == 0.0f) ? 1.0f : 0.0f;
                } else {
                    const float l = sqrtf(lq);
                    nq.x = nq.x / l;
                    nq.y = nq.y / l;
                    nq.z = nq.z / l;
                    const float d = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
                    wn = d > 0.0f ? mrt_powf(d, ps->sigma_normal) : 0.0f;
                }
                if (!(wn != 0.0f)) continue; /* a zero (or NaN) normal weight: the tap carries nothing across */
                const mrt_f4 aq = albedo[q];
                const float zp = ap.w, zq = aq.w;
                const float zm = zp > zq ? zp : zq;
                const float dz = zp > zq ? zp - zq : zq - zp;
                const float ez = dz != 0.0f ? dz / (zm * ps->sigma_depth) : 0.0f;
                const float a0 = ap.x - aq.x, a1 = ap.y - aq.y, a2 = ap.z - aq.z;
                const float ea = ((a0 * a0 + a1 * a1) + a2 * a2) * ps->inv_sigma_albedo2;
                const float c0 = cp.x - cq.x, c1 = cp.y - cq.y, c2 = cp.z - cq.z;
                const float ec = ((c0 * c0 + c1 * c1) + c2 * c2) * ps->inv_sigma_color2;
                w = (h * wn) * mrt_expf(-((ez + ea) + ec));
            }
            s0 = s0 + w * cq.x;
            s1 = s1 + w * cq.y;
            s2 = s2 + w * cq.z;
            sw = sw + w;
        }
    }
    mrt_f4 o;
    o.x = s0 / sw;
    o.y = s1 / sw;
    o.z = s2 / sw;
    o.w = cp.w;
    return o;
}

#endif
