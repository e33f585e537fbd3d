/* mrt_radiance.h -- draw()'s pixel over a group of radiance records (mrt_radiance_fold in mrt.h),
 * written once for the host and the device kernel so both produce the same bits: IEEE add / mul / div
 * in float32 without contraction (-ffp-contract=off).  It restates the render's own mode-0 fold
 * (main.cpp:150-175), so a group that holds a pixel's paths in sample order gives mrt_render's pixel.
 *
 *   c = (0, 0, 0);  per record in order:  L = the record's radiance, or c where a channel of L is not
 *   finite (main.cpp:162-164: the running sum doubles);  c = c + L
 *   c = c / (float)group  (per channel);  l = (c.x * 0.212655f + c.y * 0.715158f) + c.z * 0.072187f
 *   if (l > max_luminance) c = c * (max_luminance / l)
 */
#ifndef MRT_RADIANCE_H
#define MRT_RADIANCE_H
#include <stdint.h>
#include "mrt_mathfn.h"

/* a float4 of the output / one mrt_radiance record as 16 bytes (one 128-bit access on the device) */
#if defined(__HIP_DEVICE_COMPILE__)
typedef struct __attribute__((aligned(16))) mrt_rad4 { float x, y, z; uint32_t rays; } mrt_rad4;
typedef struct __attribute__((aligned(16))) mrt_rgb4 { float x, y, z, w; } mrt_rgb4;
#else
typedef struct mrt_rad4 { float x, y, z; uint32_t rays; } mrt_rad4;
typedef struct mrt_rgb4 { float x, y, z, w; } mrt_rgb4;
#endif

MRT_HD int mrt_radiance_finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

/* one record into the running sum */
MRT_HD mrt_rgb4 mrt_radiance_add(mrt_rgb4 c, mrt_rad4 r) {
    float x = r.x, y = r.y, z = r.z;
    if (!(mrt_radiance_finite(x) && mrt_radiance_finite(y) && mrt_radiance_finite(z))) {
        x = c.x;
        y = c.y;
        z = c.z;
    }
    c.x = c.x + x;
    c.y = c.y + y;
    c.z = c.z + z;
    return c;
}

/* the pixel after its last record */
MRT_HD mrt_rgb4 mrt_radiance_final(mrt_rgb4 c, uint32_t group, float max_luminance) {
    const float n = (float)group;
    c.x = c.x / n;
    c.y = c.y / n;
    c.z = c.z / n;
    const float l = (c.x * 0.212655f + c.y * 0.715158f) + c.z * 0.072187f;
    if (l > max_luminance) {
        const float k = max_luminance / l;
        c.x = c.x * k;
        c.y = c.y * k;
        c.z = c.z * k;
    }
    c.w = 0.0f;
    return c;
}

#endif
