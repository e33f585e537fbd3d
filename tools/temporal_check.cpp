// temporal_check -- the host forms of mrt_make_camera and mrt_reproject run stand-alone on the CPU,
// for a sanitizer build (`make temporal-check`: AddressSanitizer + UBSan over mrt_temporal.hip's host
// code, scene_builder.cpp and mrt_common.cpp; no GPU code runs, nothing preloaded).  It reprojects
// frames whose taps land on every side of the image -- odd sizes, 1 x 1, cameras far apart, behind
// each other, degenerate (zero) and huge (1e30) guide values -- and prints one line per case with the
// pixels that kept history; any out-of-bounds tap or undefined conversion stops the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mrt.h"

static mrt_camera camera(float px, float py, float pz, float lx, float ly, float lz, float vfov, float aspect) {
    mrt_camera_params p{};
    p.pos[0] = px; p.pos[1] = py; p.pos[2] = pz;
    p.lookat[0] = lx; p.lookat[1] = ly; p.lookat[2] = lz;
    p.up[1] = 1.0f;
    p.vfov_deg = vfov;
    p.aspect = aspect;
    p.focus_dist = 1.0f;
    p.time1 = 1.0f;
    mrt_camera c;
    if (mrt_make_camera(&p, &c) != MRT_OK) {
        fprintf(stderr, "make_camera: %s\n", mrt_last_error());
        exit(1);
    }
    return c;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

int main() {
    // degenerate frames are refused, not computed
    {
        mrt_camera_params p{};
        mrt_camera c;
        if (mrt_make_camera(&p, &c) != MRT_ERR_INVALID) return 1;
        p.pos[1] = 3.0f;
        p.up[1] = 1.0f;
        p.vfov_deg = 40.0f;
        p.aspect = p.focus_dist = 1.0f;
        if (mrt_make_camera(&p, &c) != MRT_ERR_INVALID) return 1;  // up parallel to the view
    }
    const uint32_t sizes[][2] = {{37, 23}, {1, 1}, {130, 5}, {3, 64}};
    mrt_temporal_params tp;
    mrt_default_temporal_params(&tp);
    uint32_t seed = 12345u;
    for (const auto& wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        const float aspect = (float)w / (float)h;
        const size_t n = (size_t)w * h * 4;
        const mrt_camera cur = camera(0, 0, 0, 0, 0, -1, 50, aspect);
        const mrt_camera prevs[] = {cur, camera(0.3f, -0.2f, 0.1f, 0.2f, -0.1f, -1, 50, aspect), camera(0, 0, -60, 0, 0, -61, 50, aspect),
                                    camera(-200, 400, -20, -199, 400, -20, 20, aspect), camera(5, 0, -4, 0, 0, -4, 120, aspect),
                                    camera(0, 0, 1e-3f, 0, 0, -1, 179, aspect)};
        for (int kind = 0; kind < 3; kind++) {  // plane guides; zero guides; huge guides
            std::vector<float> rgb(n), nrm(n), alb(n), hist(n), out(n, -1.0f);
            for (size_t i = 0; i < n; i += 4) {
                for (int k = 0; k < 3; k++) rgb[i + k] = unit(seed), hist[i + k] = unit(seed), alb[i + k] = 0.5f;
                hist[i + 3] = 1.0f + (float)((lcg(seed) >> 16) % 40u);
                nrm[i + 2] = 1.0f;
                nrm[i + 3] = ((lcg(seed) >> 16) % 8u) ? 1.0f : 0.5f;
                alb[i + 3] = kind == 0 ? 2.0f + 6.0f * unit(seed) : (kind == 1 ? 0.0f : 1e30f);
                if (kind == 1) nrm[i + 2] = 0.0f;
            }
            int c = 0;
            for (const mrt_camera& prev : prevs) {
                if (mrt_reproject(rgb.data(), nrm.data(), alb.data(), &cur, hist.data(), nrm.data(), alb.data(), &prev, w, h, &tp, out.data()) != MRT_OK) {
                    fprintf(stderr, "reproject: %s\n", mrt_last_error());
                    return 1;
                }
                size_t kept = 0;
                for (size_t i = 0; i < n; i += 4) {
                    if (!(out[i + 3] >= 1.0f && out[i + 3] <= tp.max_history)) return 1;
                    kept += out[i + 3] > 1.0f;
                }
                printf("%ux%u guides %d camera %d: %zu of %zu pixels kept history\n", w, h, kind, c++, kept, n / 4);
            }
            if (mrt_reproject(rgb.data(), nrm.data(), alb.data(), &cur, nullptr, nullptr, nullptr, nullptr, w, h, &tp, out.data()) != MRT_OK) return 1;
        }
    }
    return 0;
}
