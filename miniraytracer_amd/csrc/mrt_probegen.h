// mrt_probegen.h -- the probe generators' arithmetic (include/mrt.h "ray queries" and "radiance
// queries"): what one generated record holds, written once for the device kernels and the host forms
// (mrt_probegen.hip), the per-record functions of the CPU backend's unit (mrt_cpu.hip:
// mrt_camera_path_probe, mrt_pano_probe) and mrt_camera_pixel_ray (mrt_common.cpp).  Everything is
// float32 in the order written; every unit that includes it is built without contraction.
//
// Two parts.  The pixel ray needs nothing but the ABI structs, so a plain host unit can take it alone
// (MRT_PROBEGEN_PIXEL_RAY_ONLY).  The path key, the camera and panorama starts and the surface probe
// use the hot path's own functions (mrt_shade.h: the PCG32 stream, camera_ray_args, onb_apply, the
// contract's roots and sincos); on the host they need MRT_HOST_BACKEND, as mrt_cpu.hip defines it.
#pragma once
#include <stdint.h>
#include "../../include/mrt.h"

#if defined(__HIP__)
#define MRT_PG_FN __host__ __device__ inline
#else
#define MRT_PG_FN inline
#endif

// A generated record as the kernels store it: three 16-byte words, the layout of mrt_ray and mrt_probe
// (mrt_cast.h CastRay, mrt_probe.h ProbeRec).
struct mrt_gen_rec {
    uint32_t w[12];
};
static_assert(sizeof(mrt_gen_rec) == sizeof(mrt_ray) && sizeof(mrt_gen_rec) == sizeof(mrt_probe), "the ABI's records");
MRT_PG_FN uint32_t mrt_gen_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

// mrt_camera_pixel_ray: the pinhole ray through the centre of pixel (x, y), row 0 = bottom
// (include/mrt_temporal.h step 2).  x < width, y < height.
MRT_PG_FN mrt_gen_rec mrt_gen_pixel_ray(const mrt_camera& cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y) {
    const float s = ((float)x + 0.5f) / (float)width, t = ((float)y + 0.5f) / (float)height;
    mrt_gen_rec r;
    for (int k = 0; k < 3; k++) {
        r.w[k] = mrt_gen_bits(cam.origin[k]);
        r.w[4 + k] = mrt_gen_bits(((cam.llcorner[k] + s * cam.horz[k]) + t * cam.vert[k]) - cam.origin[k]);
    }
    r.w[3] = mrt_gen_bits(cam.time0);
    r.w[7] = 0x7F800000u;  // tmax = +inf
    r.w[8] = r.w[9] = r.w[10] = r.w[11] = 0u;  // inside, reserved
    return r;
}

#ifndef MRT_PROBEGEN_PIXEL_RAY_ONLY
#include "mrt_shade.h"

namespace mrtd {

// What the path key reads of a render desc; ns = sqrt_samples^2 (below 2^64)
struct GenGrid {
    uint32_t width, height, sq;
    uint64_t ns, seed;
};
MRT_DFN GenGrid gen_grid(uint32_t width, uint32_t height, uint32_t sq, uint64_t seed) {
    return GenGrid{width, height, sq, (uint64_t)sq * sq, seed};
}

MRT_DFN mrt_gen_rec gen_probe_rec(f3 o, f3 dir, float time, const Pcg& rng) {
    mrt_gen_rec r;
    r.w[0] = __float_as_uint(o.x), r.w[1] = __float_as_uint(o.y), r.w[2] = __float_as_uint(o.z), r.w[3] = __float_as_uint(time);
    r.w[4] = __float_as_uint(dir.x), r.w[5] = __float_as_uint(dir.y), r.w[6] = __float_as_uint(dir.z), r.w[7] = 0u;  // inside
    r.w[8] = (uint32_t)rng.state, r.w[9] = (uint32_t)(rng.state >> 32);
    r.w[10] = (uint32_t)rng.inc, r.w[11] = (uint32_t)(rng.inc >> 32);
    return r;
}

// (pixel, sample) of a render -> the path's stream and its image coordinates, as render_tiles forms
// them: the sample grid of main.cpp:319-332 in float, u and v by IEEE division; the stream keyed by
// path_id = pixel * ns + sample.  pixel < width * height, sample < ns.
MRT_DFN void gen_path_key(const GenGrid& g, uint32_t pixel, uint32_t sample, Pcg& rng, float* u, float* v) {
    const uint32_t x = pixel % g.width, y = pixel / g.width;
    const uint32_t i = sample / g.sq, j = sample % g.sq;
    const float dx = ((float)i + 0.5f) / (float)g.sq, dy = ((float)j + 0.5f) / (float)g.sq;
    *u = ((float)x + dx) / (float)g.width;
    *v = ((float)y + dy) / (float)g.height;
    const uint64_t path_id = (uint64_t)pixel * g.ns + sample;
    pcg_seed(rng, splitmix64(g.seed ^ path_id), path_id);
}

// mrt_camera_path_probe: the key, then camera::get_ray's arithmetic (camera.h:38-44) -- the render's own
// camera_ray_args (mrt_shade.h), which reads the camera through a scene's camp and nothing else of the
// scene.  On the device `camp` is a uniform address that scalar loads can read (the kernel's argument
// segment or HBM).
MRT_DFN mrt_gen_rec gen_camera_probe(const mrt_camera* camp, const GenGrid& g, uint32_t pixel, uint32_t sample) {
    Pcg rng;
    float u, v;
    gen_path_key(g, pixel, sample, rng, &u, &v);
    DScene S{};
    S.camp = camp;
    f3 o, dir;
    float time;
    camera_ray_args(S, rng, u, v, &o, &dir, &time);
    return gen_probe_rec(o, dir, time, rng);
}

// mrt_pano_probe (the formulas: include/mrt.h): `frame` is mrt_make_camera's camera of the panorama's
// parameters, made once on the host; its origin, u, v, w, time0 and time1 are read.
MRT_DFN mrt_gen_rec gen_pano_probe(const mrt_camera& frame, const GenGrid& g, uint32_t pixel, uint32_t sample) {
    Pcg rng;
    float s, t;
    gen_path_key(g, pixel, sample, rng, &s, &t);
    const float phi = (s - 0.5f) * 6.2831855f, theta = (t - 0.5f) * 3.1415927f;
    const float ct = mrt_cosf(theta);
    const float a = ct * mrt_sinf(phi), b = mrt_sinf(theta), c = ct * mrt_cosf(phi);
    const f3 dir = sub(add(fmul(a, ld3(frame.u)), fmul(b, ld3(frame.v))), fmul(c, ld3(frame.w)));
    const float time = ref_fma(frame.time1 - frame.time0, randf(rng), frame.time0);  // camera.h:41
    return gen_probe_rec(ld3(frame.origin), dir, time, rng);
}

// mrt_surface_probes, record j = i * P + k (the formulas: include/mrt.h): stratum k of the
// sq x sq grid over a cosine-weighted hemisphere around the normal of hit i, from the stream keyed by
// `id` = first_id + j.  The hit as its two 16-byte words (mrt_cast.h CastHit); has_ray: the casting ray's
// direction `rd` turns the normal towards it, its time `rtime` is the record's.
MRT_DFN mrt_gen_rec gen_surface_probe(uint4 tp, uint4 nm, bool has_ray, f3 rd, float rtime, uint32_t sq, uint64_t seed, uint64_t id, uint32_t k) {
    Pcg rng;
    pcg_seed(rng, splitmix64(seed ^ id), id);
    const float u1 = randf(rng);
    const float u2 = randf(rng);  // (a miss draws as well: the stream never depends on the hit)
    if (nm.w == MRT_NO_HIT) return gen_probe_rec(f3{0.0f, 0.0f, 0.0f}, f3{0.0f, 0.0f, 0.0f}, 0.0f, rng);
    const uint32_t a = k / sq, b = k % sq;
    const float r1 = ((float)a + u1) / (float)sq, r2 = ((float)b + u2) / (float)sq;
    // a cosine-weighted direction: NOT random_cosine_direction_pre, whose x and y carry the
    // reference's factor 2 (pcg.cpp:92-93)
    const float z = sqrt_(1.0f - r2);
    const float s = sqrt_(r2);
    const float phi = (2 * PI_F) * r1;
    float sp, cp;
    sincos_(phi, &sp, &cp);
    const f3 vec{cp * s, sp * s, z};
    f3 w{__uint_as_float(nm.x), __uint_as_float(nm.y), __uint_as_float(nm.z)};
    if (has_ray && dot(w, rd) > 0.0f) w = f3{-w.x, -w.y, -w.z};  // (a NaN dot does not turn it)
    const f3 d = onb_apply(w, vec);
    return gen_probe_rec(f3{__uint_as_float(tp.y), __uint_as_float(tp.z), __uint_as_float(tp.w)}, d, has_ray ? rtime : 0.0f, rng);
}

}  // namespace mrtd
#endif  // MRT_PROBEGEN_PIXEL_RAY_ONLY
