// probegen_check -- the probe generators' host forms run stand-alone on the CPU, for a sanitizer build
// (`make probegen-check`: AddressSanitizer + UBSan over mrt_probegen.hip's host forms, the per-record
// functions of mrt_cpu.hip and mrt_common.cpp, and the scene builder; no GPU code runs, nothing
// preloaded).  The three range forms at ragged ranges into exact-size buffers against the per-record
// functions, under the cameras of scenes 5 and 0 (a lens); the surface probes on hand-made hits that
// include misses and non-finite normals, whole and cut in two.  A record written past its range, a
// read past the hits or an undefined conversion stops the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/mrt.h"

// (the CPU backend's adaptive render asks the moments unit for its refinement list; no render runs here
// and that unit holds device kernels, so it is not built in)
std::vector<uint32_t> mrt_internal_refine_slots(const float*, uint32_t, float, float) { return {}; }

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "probegen_check: %s (%s)\n", what, mrt_last_error());
        exit(1);
    }
}

int main() {
    const uint32_t W = 21, H = 13, sq = 3, ns = sq * sq;
    const uint64_t npath = (uint64_t)W * H * ns, npix = (uint64_t)W * H;
    for (uint32_t sid : {5u, 0u}) {
        mrt_scene_blob* blob = nullptr;
        need(mrt_select_scene(sid, (float)W / (float)H, nullptr, &blob) == MRT_OK, "select_scene");
        mrt_scene_view view;
        need(mrt_scene_blob_view(blob, &view) == MRT_OK, "blob_view");
        mrt_camera_params cp;
        need(mrt_scene_camera_params(blob, &cp) == MRT_OK, "camera_params");
        mrt_render_desc d{};
        d.width = W, d.height = H, d.sqrt_samples = sq, d.seed = 11350390909718046443ull;
        const uint64_t firsts[] = {0, 5, npath - 65, npath - 1};
        const uint32_t counts[] = {1, 63, 65, 1000, (uint32_t)npath};
        uint64_t checked = 0;
        for (uint64_t first : firsts)
            for (uint32_t n : counts) {
                if (first + n > npath) continue;
                std::vector<mrt_probe> cam(n), pano(n);  // exact size
                need(mrt_camera_path_probes(&view.camera, &d, first, n, cam.data()) == MRT_OK, "camera_path_probes");
                need(mrt_pano_probes(&cp, &d, first, n, pano.data()) == MRT_OK, "pano_probes");
                for (uint32_t j = 0; j < n; j++) {
                    const uint64_t q = first + j;
                    mrt_probe a, b;
                    need(mrt_camera_path_probe(&view.camera, &d, (uint32_t)(q / ns), (uint32_t)(q % ns), &a) == MRT_OK, "camera_path_probe");
                    need(mrt_pano_probe(&cp, &d, (uint32_t)(q / ns), (uint32_t)(q % ns), &b) == MRT_OK, "pano_probe");
                    need(memcmp(&a, &cam[j], sizeof a) == 0, "camera range differs from the per-record function");
                    need(memcmp(&b, &pano[j], sizeof b) == 0, "panorama range differs from the per-record function");
                }
                checked += n;
                if (first + n <= npix) {
                    std::vector<mrt_ray> rays(n);
                    need(mrt_camera_pixel_rays(&view.camera, W, H, first, n, rays.data()) == MRT_OK, "camera_pixel_rays");
                    for (uint32_t j = 0; j < n; j++) {
                        mrt_ray a;
                        need(mrt_camera_pixel_ray(&view.camera, W, H, (uint32_t)((first + j) % W), (uint32_t)((first + j) / W), &a) == MRT_OK, "camera_pixel_ray");
                        need(memcmp(&a, &rays[j], sizeof a) == 0, "pixel-ray range differs from the per-record function");
                    }
                }
            }
        mrt_probe one;
        need(mrt_camera_path_probes(&view.camera, &d, npath, 1, &one) == MRT_ERR_INVALID, "a range past the render accepted");
        need(mrt_pano_probes(&cp, &d, npath - 1, 2, &one) == MRT_ERR_INVALID, "a range past the render accepted");
        need(mrt_camera_pixel_rays(&view.camera, W, H, npix, 1, (mrt_ray*)&one) == MRT_ERR_INVALID, "a range past the image accepted");
        need(mrt_camera_path_probes(nullptr, nullptr, 0, 0, nullptr) == MRT_OK, "n == 0");
        printf("scene %u camera: %llu records of each range equal the per-record functions\n", sid, (unsigned long long)checked);
        mrt_scene_blob_free(blob);
    }

    // surface probes: hand-made hits -- unit, axis-aligned, zero, huge, denormal and non-finite normals,
    // misses in between -- with and without rays
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float normals[][3] = {{0, 1, 0}, {1, 0, 0}, {-0.95f, 0.3f, 0.1f}, {0.6f, 0, 0.8f}, {0, 0, 0}, {3e38f, 3e38f, 3e38f}, {1e-40f, 0, 0},
                                {nan, 0, 1}, {inf, 0, 0}, {0, -inf, nan}, {0.577f, 0.577f, 0.577f}};
    std::vector<mrt_hit> hits;
    std::vector<mrt_ray> rays;
    for (size_t i = 0; i < sizeof normals / sizeof normals[0]; i++)
        for (int miss = 0; miss < 2; miss++) {
            mrt_hit h{};
            h.t = miss ? inf : 1.5f;
            h.p[0] = (float)i, h.p[1] = -2.0f, h.p[2] = 1e6f;
            memcpy(h.n, normals[i], sizeof h.n);
            h.mat = miss ? MRT_NO_HIT : (uint32_t)i;
            hits.push_back(h);
            mrt_ray r{};
            r.d[0] = i & 1 ? 1.0f : -1.0f, r.d[1] = i == 3 ? nan : 0.5f, r.d[2] = 0.25f;
            r.time = 0.125f * (float)i;
            rays.push_back(r);
        }
    const uint32_t nh = (uint32_t)hits.size();
    for (uint32_t s : {1u, 2u, 5u}) {
        const uint32_t P = s * s;
        for (const mrt_ray* rp : {(const mrt_ray*)nullptr, (const mrt_ray*)rays.data()}) {
            std::vector<mrt_probe> whole((size_t)nh * P), a((size_t)7 * P), b((size_t)(nh - 7) * P);
            const uint64_t id0 = ~0ull - 20;  // the ids wrap
            need(mrt_surface_probes(hits.data(), rp, nh, s, 9, id0, whole.data()) == MRT_OK, "surface_probes");
            need(mrt_surface_probes(hits.data(), rp, 7, s, 9, id0, a.data()) == MRT_OK, "surface_probes (head)");
            need(mrt_surface_probes(hits.data() + 7, rp ? rp + 7 : nullptr, nh - 7, s, 9, id0 + 7ull * P, b.data()) == MRT_OK, "surface_probes (tail)");
            need(memcmp(whole.data(), a.data(), a.size() * sizeof(mrt_probe)) == 0, "a batch cut in two differs from the whole (head)");
            need(memcmp(whole.data() + a.size(), b.data(), b.size() * sizeof(mrt_probe)) == 0, "a batch cut in two differs from the whole (tail)");
            for (uint32_t j = 0; j < nh * P; j++) {
                const mrt_probe& q = whole[j];
                mrt_probe seeded;
                mrt_probe_seed(9, id0 + j, &seeded);
                need(q.rng_inc == seeded.rng_inc && q.inside == 0, "a record's stream or inside flag");
                if (hits[j / P].mat == MRT_NO_HIT) {
                    need(q.o[0] == 0 && q.o[1] == 0 && q.o[2] == 0 && q.d[0] == 0 && q.d[1] == 0 && q.d[2] == 0 && q.time == 0, "a miss is not the null record");
                } else {
                    need(q.o[0] == hits[j / P].p[0] && q.o[2] == 1e6f && q.time == (rp ? rp[j / P].time : 0.0f), "a record's origin or time");
                }
            }
        }
        printf("surface probes, sqrt_per_hit %u: %u records, whole and cut, with and without rays\n", s, nh * P);
    }
    mrt_probe q;
    need(mrt_surface_probes(hits.data(), nullptr, nh, 0, 0, 0, &q) == MRT_ERR_INVALID, "sqrt_per_hit 0 accepted");
    need(mrt_surface_probes(hits.data(), nullptr, 1u << 20, 64, 0, 0, &q) == MRT_ERR_INVALID, "2^32 records accepted");
    return 0;
}
