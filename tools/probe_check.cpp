// probe_check -- the host side of the radiance queries run stand-alone on the CPU, for a sanitizer
// build (`make probe-check`: AddressSanitizer + UBSan over the CPU backend's mrt_cpu_trace_rays, the
// probe helpers of mrt_cpu.hip, the scene compiler and the scene builder; no GPU code runs, nothing
// preloaded).  It traces camera-path, panorama and non-finite probes of scenes 5, 6 and 0 at
// max_bounces 0, 1 and 32 -- the level rows are max(max_bounces, 1) long -- whole and cut in two, and
// prints one line per case with the ray total; a store past a level row, a record past the batch or an
// undefined conversion stops the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/mrt.h"
#include "../miniraytracer_amd/csrc/mrt_cpu.h"

// (the CPU backend's adaptive render asks the moments unit for its refinement list; no adaptive render
// runs here and that unit holds device kernels, so it is not built in)
std::vector<uint32_t> mrt_internal_refine_slots(const float*, uint32_t, float, float) { return {}; }

static void need(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "probe_check: %s (%s)\n", what, mrt_last_error());
        exit(1);
    }
}

int main() {
    const uint32_t W = 21, H = 13, sq = 2, ns = sq * sq;
    for (uint32_t sid : {5u, 6u, 0u}) {
        mrt_scene_blob* blob = nullptr;
        need(mrt_select_scene(sid, (float)W / (float)H, nullptr, &blob) == MRT_OK, "select_scene");
        mrt_scene_view view;
        need(mrt_scene_blob_view(blob, &view) == MRT_OK, "blob_view");
        mrt_camera_params cp;
        need(mrt_scene_camera_params(blob, &cp) == MRT_OK, "camera_params");
        mrt_cpu_scene* sc = nullptr;
        need(mrt_cpu_scene_create(&view, &sc) == MRT_OK, "cpu_scene_create");
        mrt_render_desc d{};
        d.width = W, d.height = H, d.sqrt_samples = sq, d.seed = 11350390909718046443ull;
        // every path start of the frame, the same for the panorama, then non-finite and zero records
        std::vector<mrt_probe> probes;
        for (uint32_t pix = 0; pix < W * H; pix++)
            for (uint32_t s = 0; s < ns; s++) {
                mrt_probe q;
                need(mrt_camera_path_probe(&view.camera, &d, pix, s, &q) == MRT_OK, "camera_path_probe");
                probes.push_back(q);
                need(mrt_pano_probe(&cp, &d, pix, s, &q) == MRT_OK, "pano_probe");
                probes.push_back(q);
            }
        const float odd[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                             0.0f, 3e38f, 1e-40f};
        for (float v : odd)
            for (int k = 0; k < 6; k++) {
                mrt_probe q = probes[(size_t)k * 17];
                (k < 3 ? q.o[k] : q.d[k - 3]) = v;
                q.inside = (uint32_t)k;
                mrt_probe_seed(7, probes.size(), &q);
                if (k == 5) q.rng_inc &= ~1ull;  // an even increment is used as given
                probes.push_back(q);
            }
        mrt_probe zero;
        memset(&zero, 0, sizeof zero);
        probes.push_back(zero);
        mrt_probe out_of_range;
        need(mrt_camera_path_probe(&view.camera, &d, W * H, 0, &out_of_range) == MRT_ERR_INVALID, "pixel out of range accepted");
        need(mrt_pano_probe(&cp, &d, 0, ns, &out_of_range) == MRT_ERR_INVALID, "sample out of range accepted");
        const uint32_t n = (uint32_t)probes.size();
        for (uint32_t depth : {0u, 1u, 32u}) {
            // exact-size buffers: a record written past the batch is a heap overflow
            std::vector<mrt_radiance> whole(n), a(n / 3), b(n - n / 3);
            need(mrt_cpu_trace_rays(sc, probes.data(), n, depth, whole.data()) == MRT_OK, "trace_rays");
            need(mrt_cpu_trace_rays(sc, probes.data(), n / 3, depth, a.data()) == MRT_OK, "trace_rays (head)");
            need(mrt_cpu_trace_rays(sc, probes.data() + n / 3, n - n / 3, depth, b.data()) == MRT_OK, "trace_rays (tail)");
            uint64_t rays = 0;
            for (uint32_t i = 0; i < n; i++) {
                need(whole[i].rays >= 1 && whole[i].rays <= depth + 1, "a path ran more than max_bounces + 1 segments");
                const mrt_radiance& part = i < n / 3 ? a[i] : b[i - n / 3];
                need(memcmp(&part, &whole[i], sizeof part) == 0, "a batch cut in two differs from the whole");
                rays += whole[i].rays;
            }
            std::vector<float> rgb((size_t)(n / ns) * 4);
            need(mrt_radiance_fold(whole.data(), n / ns, ns, 1000.0f, rgb.data()) == MRT_OK, "radiance_fold");
            printf("scene %u depth %u: %u probes, %llu rays, first pixel %g %g %g\n", sid, depth, n, (unsigned long long)rays, (double)rgb[0], (double)rgb[1],
                   (double)rgb[2]);
        }
        mrt_cpu_scene_free(sc);
        mrt_scene_blob_free(blob);
    }
    return 0;
}
