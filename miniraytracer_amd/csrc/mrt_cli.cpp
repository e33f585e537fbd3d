// mrt_cli.cpp -- headless command-line driver with the reference's flags (cmdline_parser.cpp:78-123)
// in place of the SDL window loop of main() (main.cpp:283-498): builds the scene, renders it on the
// MI355X(s) through the C-ABI, prints the reference's "Trace: ... Mrays/s" line (main.cpp:403-406)
// and writes the image (-o out.pfm: linear; -o out.ppm: Drago tone map, main.cpp:416-444).
//
// -gpus N shards the work_queue tiles over N ranks (one host thread per rank, the tiles dealt in
// permuted rounds of N, mrt_local_pixels); 0 = every visible GPU.  Rank r renders on GPU r % (GPUs
// visible): with fewer GPUs than ranks several ranks share a device (the multi-rank assembly runs
// on one GPU as on eight); with -backend cpu each rank is a CPU-backend context of -threads workers.  -backend cpu renders on the host instead (the CPU backend: the
// same hot-path code compiled for the host, exact contract), with -threads worker threads as the
// reference's -threads (0 = every core).  -numerics exact|fast picks the GPU's arithmetic contract.
// -gather rccl|host: how a multi-GPU frame is assembled.  rccl (the default when every rank has a
// GPU of its own): each rank's mrt_render_gather renders its shard into device memory and one RCCL
// gather over xGMI plus a device scatter assemble the frame on GPU 0 (mrt_comm_init_all: one
// communicator per GPU in this process); host: each rank's mrt_render copies its own pixels into the
// shared host framebuffer (the only choice when ranks share a GPU, or with -backend cpu).
// -aux PREFIX writes the first-hit feature buffers (mrt_render_aux, at min(spp, 16) samples) as
// PREFIX_normal.pfm and PREFIX_albedo.pfm; -denoise N filters the image with N a-trous passes over
// those buffers (mrt_denoise, the library's default widths) before -o writes it.  Both work with
// every backend and -gpus count: each rank fills its own pixels of the shared host buffers.
// -adaptive N renders adaptively (mrt_render_adaptive): -samples is the base pass, then up to N (1 to
// 4) refinement passes over the pixels whose standard error misses -atol X + -rtol Y * mean (the
// library's defaults where not given); -samplemap FILE.pfm writes the samples spent per pixel, grey.
// A line after "Trace:" reports the mean samples per pixel and the pixels refined per pass.  It
// composes with -denoise, -aux, -backend cpu and -gpus N over the host assembly (every decision is
// per pixel, so each rank refines its own); the RCCL gather does not carry adaptive frames.
// -lookfrom x y z, -lookat x y z, -vfov D, -aperture A, -focus F replace the scene's camera (each
// defaults to the scene's own parameter: mrt_scene_camera_params, mrt_make_camera,
// mrt_scene_set_camera).  -frames N [-orbit DEG] renders a sequence into NAME_000.ext ...: frame k
// turns lookfrom about the vertical axis through lookat by k * DEG and uses the seed
// splitmix64(seed + k); -temporal accumulates the frames (mrt_reproject, feature buffers at
// min(spp, 16) samples); -denoise N then filters what is written, never the history.
// -pick X Y casts the ray through the centre of pixel (X, Y), row 0 at the bottom (mrt_camera_pixel_ray,
// mrt_cast_rays), under the final camera and prints "pick X Y: t=... p=(...) n=(...) mat=..." or
// "pick X Y: miss" before the "Trace:" line.  -focusat X Y casts that pixel's ray under the camera the
// other flags give and focuses the lens on what it hits: focus = t * -dot(d^, w) in float32, printed as
// "focusat X Y: focus=..." (%.9g: -focus with that number renders the same image); a miss prints
// "focusat X Y: miss" and leaves the focus alone.  With -frames it applies once, to frame 0's camera.
// -pano renders a 360 x 180 degree equirectangular frame from the camera's position through the
// radiance queries (mrt_pano_probes -> mrt_trace_rays -> mrt_radiance_fold, on a GPU scene their device
// forms on one stream with nothing but the pixels copied back; exact numerics, either backend), written
// and tone-mapped as usual: the camera flags give position, look-at (the image
// centre) and up; -aperture is ignored (no lens); -gpus above 1 is refused.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/mrt.h"

static int fail(const char* what, mrt_status s) {
    fprintf(stderr, "%s: %s (%s)\n", what, mrt_strerror(s), mrt_last_error());
    return 1;
}

// -o: .ppm = Drago tone map (main.cpp:416-444), anything else = linear PFM; W*H float4, row 0 = bottom
static int write_image(const char* path, const std::vector<float>& img, uint32_t w, uint32_t h) {
    std::string o = path;
    FILE* f = fopen(path, "wb");
    if (!f) return fail("open output", MRT_ERR_IO);
    if (o.size() > 4 && o.substr(o.size() - 4) == ".ppm") {
        std::vector<uint32_t> argb((size_t)w * h);
        mrt_tonemap_argb(img.data(), w, h, argb.data());
        fprintf(f, "P6\n%u %u\n255\n", w, h);
        for (int y = (int)h - 1; y >= 0; y--)  // display is flipped (platform_linux.cpp:84)
            for (uint32_t x = 0; x < w; x++) {
                uint32_t c = argb[(size_t)y * w + x];
                unsigned char px[3] = {(unsigned char)(c >> 16), (unsigned char)(c >> 8), (unsigned char)c};
                fwrite(px, 1, 3, f);
            }
    } else {
        fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
        for (size_t i = 0; i < (size_t)w * h; i++) fwrite(&img[i * 4], 4, 3, f);
    }
    fclose(f);
    return 0;
}

static uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one job per rank on its own host thread, as the single-frame path runs them
template <typename Fn>
static mrt_status on_ranks(int world, Fn fn) {
    std::vector<mrt_status> sts(world, MRT_OK);
    std::vector<std::thread> th;
    for (int r = 0; r < world; r++) th.emplace_back([&, r] { sts[r] = fn(r); });
    for (auto& t : th) t.join();
    for (mrt_status s : sts)
        if (s) return s;
    return MRT_OK;
}

// -frames N [-orbit DEG] [-temporal] [-denoise N]: frame k renders from the camera `cp` with its
// position turned about the vertical axis through its look-at point by k * DEG, under the seed
// splitmix64(seed + k), into NAME_00k.ext.  -temporal accumulates the frames through mrt_reproject
// (feature buffers at min(spp, 16) samples, the library's default parameters); -denoise filters the
// frame that is written, never the history.  Each rank renders its own pixels of the shared host
// frame (the host assembly), on either backend.
static int run_sequence(const mrt_params& p, std::vector<mrt_scene*>& scenes, std::vector<mrt_render_desc>& descs, const mrt_camera_params& cp,
                        int frames, double orbit_deg, bool temporal, int denoise, const char* out) {
    const int world = (int)scenes.size();
    const uint32_t W = p.buffer_width, H = p.buffer_height;
    const size_t npx = (size_t)W * H;
    const bool guides = temporal || denoise >= 0;
    std::vector<float> img(npx * 4), nrm(guides ? npx * 4 : 0), alb(guides ? npx * 4 : 0);
    std::vector<float> pnrm, palb, hist, hist_new(temporal ? npx * 4 : 0), shown;
    mrt_camera pcam{};
    mrt_temporal_params tp;
    mrt_default_temporal_params(&tp);
    const uint64_t seed0 = descs[0].seed;
    std::string stem = out ? out : "", ext;
    const size_t dot = stem.rfind('.');
    if (dot != std::string::npos && stem.find('/', dot) == std::string::npos) {
        ext = stem.substr(dot);
        stem.resize(dot);
    }
    for (int k = 0; k < frames; k++) {
        mrt_camera_params ck = cp;
        const double a = (double)k * orbit_deg * 3.14159265358979323846 / 180.0;
        const double dx = (double)cp.pos[0] - (double)cp.lookat[0], dz = (double)cp.pos[2] - (double)cp.lookat[2];
        ck.pos[0] = (float)((double)cp.lookat[0] + dx * cos(a) + dz * sin(a));
        ck.pos[2] = (float)((double)cp.lookat[2] - dx * sin(a) + dz * cos(a));
        mrt_camera cam;
        mrt_status st = mrt_make_camera(&ck, &cam);
        if (st) return fail("make_camera", st);
        std::fill(img.begin(), img.end(), 0.0f);
        std::vector<uint64_t> rays(world, 0);
        auto t0 = std::chrono::steady_clock::now();
        st = on_ranks(world, [&](int r) {
            if (mrt_status s = mrt_scene_set_camera(scenes[r], &cam)) return s;
            descs[r].seed = splitmix64(seed0 + (uint64_t)k);
            return mrt_render(scenes[r], &descs[r], img.data(), &rays[r], nullptr);
        });
        if (st) return fail("render", st);
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        uint64_t total = 0;
        for (uint64_t x : rays) total += x;
        if (guides) {
            std::fill(nrm.begin(), nrm.end(), 0.0f);
            std::fill(alb.begin(), alb.end(), 0.0f);
            st = on_ranks(world, [&](int r) {
                mrt_render_desc ad = descs[r];
                ad.sqrt_samples = std::min(ad.sqrt_samples, 4u);
                ad.flags = 0;
                return mrt_render_aux(scenes[r], &ad, nrm.data(), alb.data());
            });
            if (st) return fail("render_aux", st);
        }
        const std::vector<float>* frame = &img;
        size_t kept = 0;
        if (temporal) {
            st = mrt_reproject(img.data(), nrm.data(), alb.data(), &cam, k ? hist.data() : nullptr, k ? pnrm.data() : nullptr, k ? palb.data() : nullptr,
                               k ? &pcam : nullptr, W, H, &tp, hist_new.data());
            if (st) return fail("reproject", st);
            hist.swap(hist_new);
            if (hist_new.size() != hist.size()) hist_new.resize(hist.size());
            pnrm = nrm;
            palb = alb;
            pcam = cam;
            for (size_t i = 0; i < npx; i++) kept += hist[i * 4 + 3] > 1.0f;
            frame = &hist;
        }
        if (denoise >= 0) {  // for output only: the history stays unfiltered
            mrt_denoise_params dp;
            mrt_default_denoise_params(&dp);
            dp.iterations = (uint32_t)denoise;
            shown.resize(npx * 4);
            if ((st = mrt_denoise(frame->data(), nrm.data(), alb.data(), W, H, &dp, shown.data()))) return fail("denoise", st);
            frame = &shown;
        }
        printf("frame %03d: %.2f deg, %.3fs, rays %llu", k, (double)k * orbit_deg, secs, (unsigned long long)total);
        if (temporal) printf(", history at %.1f%% of the pixels", 100.0 * (double)kept / (double)npx);
        printf("\n");
        if (out) {
            char num[16];
            snprintf(num, sizeof num, "_%03d", k);
            if (write_image((stem + num + ext).c_str(), *frame, W, H)) return 1;
        }
    }
    return 0;
}

// -pano: the frame through the radiance queries instead of mrt_render -- every pixel's samples as
// equirectangular probes at the camera's position (the render's grid and keying), traced (exact
// contract, either backend) and folded per pixel, in pieces of whole pixels.
// CPU backend: mrt_pano_probes -> mrt_trace_rays -> mrt_radiance_fold on host records, pieces of at
// most about 2^16 records.
static mrt_status render_pano_host(mrt_scene* scene, const mrt_camera_params& cp, const mrt_render_desc& d, std::vector<float>& img, uint64_t* rays) {
    const uint64_t ns = (uint64_t)d.sqrt_samples * d.sqrt_samples, npx = (uint64_t)d.width * d.height;
    if (ns > 0xFFFFFFFFull || npx > 0xFFFFFFFFull) return MRT_ERR_INVALID;
    const uint64_t piece_px = std::max<uint64_t>(1, (1u << 16) / ns);
    std::vector<mrt_probe> probes((size_t)(std::min(piece_px, npx) * ns));
    std::vector<mrt_radiance> rad(probes.size());
    *rays = 0;
    for (uint64_t p0 = 0; p0 < npx; p0 += piece_px) {
        const uint32_t m = (uint32_t)std::min(piece_px, npx - p0);
        if (mrt_status st = mrt_pano_probes(&cp, &d, p0 * ns, (uint32_t)(m * ns), probes.data())) return st;
        uint64_t r = 0;
        if (mrt_status st = mrt_trace_rays(scene, probes.data(), (uint32_t)(m * ns), d.max_bounces, rad.data(), &r)) return st;
        *rays += r;
        if (mrt_status st = mrt_radiance_fold(rad.data(), m, (uint32_t)ns, d.max_luminance, img.data() + (size_t)p0 * 4)) return st;
    }
    return MRT_OK;
}

// GPU scene: the same records never leave the device.  Per piece of whole pixels (at most about
// MRT_TRACE_PIECE records) mrt_pano_probes_device -> mrt_trace_rays_device -> mrt_radiance_rays_device
// -> mrt_radiance_fold_device are enqueued on one stream, into buffers and a level workspace allocated
// once; the frame's pixels and the ray total are copied back once at the end.
static mrt_status render_pano_device(mrt_scene* scene, int device, const mrt_camera_params& cp, const mrt_render_desc& d, std::vector<float>& img,
                                     uint64_t* rays) {
    const uint64_t ns = (uint64_t)d.sqrt_samples * d.sqrt_samples, npx = (uint64_t)d.width * d.height;
    if (ns > 0xFFFFFFFFull || npx > 0xFFFFFFFFull) return MRT_ERR_INVALID;
    const uint64_t piece_px = std::min(npx, std::max<uint64_t>(1, MRT_TRACE_PIECE / ns));
    uint64_t work_bytes = 0, work_min = 0;
    if (mrt_status st = mrt_trace_rays_workspace(scene, d.max_bounces, &work_bytes, &work_min)) return st;
    void *d_probes = nullptr, *d_rad = nullptr, *d_img = nullptr, *d_work = nullptr, *d_rays = nullptr;
    hipStream_t q = nullptr;
    auto run = [&]() -> mrt_status {
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&q) != hipSuccess) return MRT_ERR_HIP;
        if (hipMalloc(&d_probes, piece_px * ns * sizeof(mrt_probe)) != hipSuccess || hipMalloc(&d_rad, piece_px * ns * sizeof(mrt_radiance)) != hipSuccess ||
            hipMalloc(&d_img, npx * 16) != hipSuccess || hipMalloc(&d_work, work_bytes) != hipSuccess || hipMalloc(&d_rays, 8) != hipSuccess)
            return MRT_ERR_OOM;
        if (hipMemsetAsync(d_rays, 0, 8, q) != hipSuccess) return MRT_ERR_HIP;
        for (uint64_t p0 = 0; p0 < npx; p0 += piece_px) {
            const uint32_t m = (uint32_t)std::min(piece_px, npx - p0), n = (uint32_t)(m * ns);
            if (mrt_status st = mrt_pano_probes_device(&cp, &d, p0 * ns, n, (mrt_probe*)d_probes, q)) return st;
            if (mrt_status st = mrt_trace_rays_device(scene, (const mrt_probe*)d_probes, n, d.max_bounces, (mrt_radiance*)d_rad, d_work, work_bytes, q)) return st;
            if (mrt_status st = mrt_radiance_rays_device((const mrt_radiance*)d_rad, n, (uint64_t*)d_rays, q)) return st;
            if (mrt_status st = mrt_radiance_fold_device((const mrt_radiance*)d_rad, m, (uint32_t)ns, d.max_luminance, (float*)d_img + (size_t)p0 * 4, q)) return st;
        }
        if (hipMemcpyAsync(img.data(), d_img, npx * 16, hipMemcpyDeviceToHost, q) != hipSuccess ||
            hipMemcpyAsync(rays, d_rays, 8, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
            return MRT_ERR_HIP;
        return MRT_OK;
    };
    const mrt_status st = run();
    for (void* b : {d_probes, d_rad, d_img, d_work, d_rays})
        if (b) (void)hipFree(b);
    if (q) (void)hipStreamDestroy(q);
    return st;
}

int main(int argc, char** argv) {
    mrt_params p;
    if (mrt_parse_argv(argc, argv, &p) != MRT_OK) return 0;  // -help
    const char* out = nullptr;
    const char* gather = nullptr;
    const char* aux = nullptr;
    int denoise = -1;
    int adaptive = -1;
    const char* samplemap = nullptr;
    mrt_adaptive_params ap;
    mrt_default_adaptive_params(&ap);
    for (int i = 1; i + 1 < argc; i++) {
        if (!strcmp(argv[i], "-adaptive")) adaptive = atoi(argv[i + 1]);
        if (!strcmp(argv[i], "-atol")) ap.atol = strtof(argv[i + 1], nullptr);
        if (!strcmp(argv[i], "-rtol")) ap.rtol = strtof(argv[i + 1], nullptr);
        if (!strcmp(argv[i], "-samplemap")) samplemap = argv[i + 1];
        if (!strcmp(argv[i], "-o")) out = argv[i + 1];
        if (!strcmp(argv[i], "-gather")) gather = argv[i + 1];
        if (!strcmp(argv[i], "-aux")) aux = argv[i + 1];
        if (!strcmp(argv[i], "-denoise")) denoise = atoi(argv[i + 1]);
    }
    // camera and sequence flags: each camera flag defaults to the scene's own parameter
    const char* lookfrom = nullptr;
    const char* lookat = nullptr;
    const char *vfov = nullptr, *aperture = nullptr, *focus = nullptr, *frames_s = nullptr;
    int lookfrom_i = 0, lookat_i = 0;
    double orbit_deg = 0.0;
    bool temporal = false, have_orbit = false, pano = false;
    int pick_xy[2] = {-1, -1}, focusat_xy[2] = {-1, -1};
    for (int i = 1; i < argc; i++) {
        const bool v1 = i + 1 < argc, v3 = i + 3 < argc;
        if (!strcmp(argv[i], "-temporal")) temporal = true;
        if (!strcmp(argv[i], "-pano")) pano = true;
        if (!strcmp(argv[i], "-lookfrom") && v3) lookfrom = argv[lookfrom_i = i + 1];
        if (!strcmp(argv[i], "-lookat") && v3) lookat = argv[lookat_i = i + 1];
        if (!strcmp(argv[i], "-vfov") && v1) vfov = argv[i + 1];
        if (!strcmp(argv[i], "-aperture") && v1) aperture = argv[i + 1];
        if (!strcmp(argv[i], "-focus") && v1) focus = argv[i + 1];
        if (!strcmp(argv[i], "-frames") && v1) frames_s = argv[i + 1];
        if (!strcmp(argv[i], "-pick") || !strcmp(argv[i], "-focusat")) {
            int* at = argv[i][1] == 'p' ? pick_xy : focusat_xy;
            char *e0 = nullptr, *e1 = nullptr;
            const long x = i + 2 < argc ? strtol(argv[i + 1], &e0, 10) : -1, y = i + 2 < argc ? strtol(argv[i + 2], &e1, 10) : -1;
            if (i + 2 >= argc || *e0 || *e1 || e0 == argv[i + 1] || e1 == argv[i + 2] || x < 0 || y < 0 || x >= (long)p.buffer_width ||
                y >= (long)p.buffer_height) {
                fprintf(stderr, "%s X Y: a pixel of the %u x %u image, row 0 at the bottom\n", argv[i], p.buffer_width, p.buffer_height);
                return 1;
            }
            at[0] = (int)x;
            at[1] = (int)y;
        }
        if (!strcmp(argv[i], "-orbit") && v1) {
            orbit_deg = strtod(argv[i + 1], nullptr);
            have_orbit = true;
        }
    }
    const bool have_cam = lookfrom || lookat || vfov || aperture || focus;
    const int frames = frames_s ? atoi(frames_s) : 0;
    if (frames_s && (frames < 1 || frames > 999)) {
        fprintf(stderr, "-frames: 1 to 999 frames\n");
        return 1;
    }
    if ((temporal || have_orbit) && !frames_s) {
        fprintf(stderr, "-temporal / -orbit: need -frames N\n");
        return 1;
    }
    if (denoise > 16) {
        fprintf(stderr, "-denoise: 0 to 16 passes\n");
        return 1;
    }
    bool have_adaptive = false;
    for (int i = 1; i < argc; i++) have_adaptive |= !strcmp(argv[i], "-adaptive");
    if (pano) {
        if (p.gpus > 1) {
            fprintf(stderr, "-pano: the radiance queries run on one scene context (-gpus 1)\n");
            return 1;
        }
        if (have_adaptive || frames_s || aux || denoise >= 0 || (gather && !strcmp(gather, "rccl"))) {
            fprintf(stderr, "-pano: renders one frame, without -adaptive, -frames, -aux, -denoise or -gather rccl\n");
            return 1;
        }
        p.gpus = 1;
        p.numerics = 0;  // mrt_trace_rays runs the exact contract
        aperture = nullptr;  // no lens
    }
    if (have_adaptive && (adaptive < 1 || adaptive > 4)) {
        fprintf(stderr, "-adaptive: 1 to 4 refinement passes\n");
        return 1;
    }
    if (!have_adaptive && samplemap) {
        fprintf(stderr, "-samplemap: needs -adaptive N\n");
        return 1;
    }
    if (have_adaptive && gather && !strcmp(gather, "rccl")) {
        fprintf(stderr, "-adaptive: the RCCL gather does not carry adaptive frames (use -gather host, the default with -adaptive)\n");
        return 1;
    }
    if (have_adaptive) {  // draw()'s per-pixel mean (mode 0) is what the passes merge: the default unless -mode asks for 1
        bool have_mode = false;
        for (int i = 1; i < argc; i++) have_mode |= !strcmp(argv[i], "-mode");
        if (have_mode && p.threading_mode != 0) {
            fprintf(stderr, "-adaptive: renders with draw() semantics only (-mode 0)\n");
            return 1;
        }
        p.threading_mode = 0;
    }
    ap.max_passes = have_adaptive ? (uint32_t)adaptive : 0u;
    if (gather && strcmp(gather, "rccl") && strcmp(gather, "host")) {
        fprintf(stderr, "-gather: rccl or host\n");
        return 1;
    }

    auto t_gen = std::chrono::steady_clock::now();
    mrt_scene_blob* blob = nullptr;
    mrt_status st = mrt_select_scene(p.scene_select, float(p.buffer_width) / float(p.buffer_height), nullptr, &blob);
    if (st) return fail("select_scene", st);
    double gen_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_gen).count();
    mrt_scene_view view;
    mrt_scene_blob_view(blob, &view);

    const bool cpu = p.backend == 1;
    int ndev = 0, world = p.gpus ? (int)p.gpus : 1;
    if (!cpu) {
        if ((st = mrt_init(&ndev))) return fail("mrt_init", st);
        if (ndev < 1) return fail("mrt_init", MRT_ERR_NO_DEVICE);
        if (!p.gpus) world = ndev;
        if (world > ndev) fprintf(stderr, "-gpus %d: %d rank(s) on %d visible GPU(s)\n", world, world, ndev);
    }

    std::vector<mrt_scene*> scenes(world, nullptr);
    std::vector<mrt_render_desc> descs(world);
    for (int r = 0; r < world; r++) {
        if ((st = mrt_scene_upload(cpu ? MRT_DEVICE_CPU : r % ndev, &view, &scenes[r]))) return fail("scene_upload", st);
        mrt_default_render_desc(&p, &descs[r]);
        descs[r].rank = (uint32_t)r;
        descs[r].world = (uint32_t)world;
        if (!cpu && (st = mrt_prepare(scenes[r], &descs[r]))) return fail("prepare", st);
    }
    if (descs[0].flags & MRT_RF_REF_ORDER) {  // main.cpp:338-366: the workers' (initstate, initseq)
        if (!cpu) {
            fprintf(stderr, "-order ref: the reference's per-thread RNG order runs on the CPU backend only (-backend cpu)\n");
            return 1;
        }
        if (world > 1) {
            fprintf(stderr, "-order ref: the reference's per-thread RNG order is one rank's (use -order path with -gpus)\n");
            return 1;
        }
        const uint32_t n = p.num_threads ? p.num_threads : std::max(1u, std::thread::hardware_concurrency());
        std::vector<uint64_t> is(n), iq(n);
        if ((st = mrt_worker_seeds(blob, n, is.data(), iq.data()))) return fail("worker_seeds", st);
        if ((st = mrt_set_worker_seeds(scenes[0], n, is.data(), iq.data()))) return fail("set_worker_seeds", st);
        descs[0].threads = n;
    }
    // the RCCL gather needs a GPU per rank (RCCL refuses two ranks on one device)
    const bool use_rccl = !have_adaptive && !cpu && world <= ndev && (gather ? !strcmp(gather, "rccl") : world > 1);
    if (gather && !strcmp(gather, "rccl") && !use_rccl) {
        fprintf(stderr, "-gather rccl: needs the GPU backend and a GPU per rank (%d ranks, %d GPUs)\n", world, ndev);
        return 1;
    }
    // the camera flags replace the uploaded scenes' camera (nothing is built or uploaded again)
    mrt_camera_params cp;
    if ((st = mrt_scene_camera_params(blob, &cp))) return fail("scene_camera_params", st);
    if (have_cam) {
        for (int k = 0; k < 3; k++) {
            if (lookfrom) cp.pos[k] = strtof(argv[lookfrom_i + k], nullptr);
            if (lookat) cp.lookat[k] = strtof(argv[lookat_i + k], nullptr);
        }
        if (vfov) cp.vfov_deg = strtof(vfov, nullptr);
        if (aperture) cp.aperture = strtof(aperture, nullptr);
        if (focus) cp.focus_dist = strtof(focus, nullptr);
        mrt_camera cam;
        if ((st = mrt_make_camera(&cp, &cam))) return fail("make_camera", st);
        for (int r = 0; r < world; r++)
            if ((st = mrt_scene_set_camera(scenes[r], &cam))) return fail("scene_set_camera", st);
    }
    // -focusat, then -pick: one ray through the pixel's centre under the camera as it stands
    mrt_camera cam_now = view.camera;
    if (have_cam && (st = mrt_make_camera(&cp, &cam_now))) return fail("make_camera", st);
    auto cast_pixel = [&](const int* xy, mrt_ray* ray, mrt_hit* hit) {
        mrt_status e = mrt_camera_pixel_ray(&cam_now, p.buffer_width, p.buffer_height, (uint32_t)xy[0], (uint32_t)xy[1], ray);
        return e ? e : mrt_cast_rays(scenes[0], ray, 1, 0, hit);
    };
    if (focusat_xy[0] >= 0) {
        mrt_ray ray;
        mrt_hit hit;
        if ((st = cast_pixel(focusat_xy, &ray, &hit))) return fail("focusat", st);
        if (hit.mat == MRT_NO_HIT) {
            printf("focusat %d %d: miss\n", focusat_xy[0], focusat_xy[1]);
        } else {
            // the hit's depth along the view axis: t * -dot(d^, w), float32
            const float dl = sqrtf((ray.d[0] * ray.d[0] + ray.d[1] * ray.d[1]) + ray.d[2] * ray.d[2]);
            const float dw = ((ray.d[0] / dl) * cam_now.w[0] + (ray.d[1] / dl) * cam_now.w[1]) + (ray.d[2] / dl) * cam_now.w[2];
            cp.focus_dist = hit.t * -dw;
            printf("focusat %d %d: focus=%.9g\n", focusat_xy[0], focusat_xy[1], (double)cp.focus_dist);
            if ((st = mrt_make_camera(&cp, &cam_now))) return fail("make_camera", st);
            for (int r = 0; r < world; r++)
                if ((st = mrt_scene_set_camera(scenes[r], &cam_now))) return fail("scene_set_camera", st);
        }
    }
    if (pick_xy[0] >= 0) {
        mrt_ray ray;
        mrt_hit hit;
        if ((st = cast_pixel(pick_xy, &ray, &hit))) return fail("pick", st);
        if (hit.mat == MRT_NO_HIT) printf("pick %d %d: miss\n", pick_xy[0], pick_xy[1]);
        else
            printf("pick %d %d: t=%.9g p=(%.9g %.9g %.9g) n=(%.9g %.9g %.9g) mat=%u\n", pick_xy[0], pick_xy[1], (double)hit.t, (double)hit.p[0],
                   (double)hit.p[1], (double)hit.p[2], (double)hit.n[0], (double)hit.n[1], (double)hit.n[2], hit.mat);
    }
    if (frames_s) {
        if (have_adaptive || aux || (gather && !strcmp(gather, "rccl"))) {
            fprintf(stderr, "-frames: a sequence renders over the host assembly, without -adaptive, -aux or -gather rccl\n");
            return 1;
        }
        const int rc = run_sequence(p, scenes, descs, cp, frames, orbit_deg, temporal, denoise, out);
        for (auto* s : scenes) mrt_scene_free(s);
        mrt_scene_blob_free(blob);
        return rc;
    }

    std::vector<mrt_comm*> comms(world, nullptr);
    if (use_rccl) {
        std::vector<int> devs(world);
        for (int r = 0; r < world; r++) devs[r] = r;
        if ((st = mrt_comm_init_all((uint32_t)world, devs.data(), comms.data()))) return fail("comm_init_all", st);
    }
    std::vector<float> img((size_t)p.buffer_width * p.buffer_height * 4, 0.0f);
    std::vector<float> mom(have_adaptive ? img.size() : 0, 0.0f);  // -adaptive: the moments frame (w = samples spent)
    std::vector<uint64_t> rays(world, 0);
    std::vector<mrt_status> sts(world, MRT_OK);

    auto t0 = std::chrono::steady_clock::now();  // main.cpp:375
    std::vector<std::thread> th;
    if (pano) sts[0] = cpu ? render_pano_host(scenes[0], cp, descs[0], img, &rays[0]) : render_pano_device(scenes[0], 0, cp, descs[0], img, &rays[0]);
    for (int r = 0; r < world && !pano; r++)
        th.emplace_back([&, r] {
            sts[r] = have_adaptive ? mrt_render_adaptive(scenes[r], &descs[r], &ap, img.data(), mom.data(), &rays[r], nullptr)
                     : use_rccl    ? mrt_render_gather(scenes[r], comms[r], &descs[r], r == 0 ? img.data() : nullptr, &rays[r])
                                   : mrt_render(scenes[r], &descs[r], img.data(), &rays[r], nullptr);
        });
    for (auto& t : th) t.join();
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int r = 0; r < world; r++)
        if (sts[r]) return fail("render", sts[r]);
    uint64_t total = 0;
    if (use_rccl) total = rays[0];  // (all-reduced over the ranks)
    else
        for (uint64_t x : rays) total += x;
    char where[64];
    if (cpu) {
        mrt_kernel_info ki{};
        mrt_scene_kernel_info(scenes[0], &ki);
        snprintf(where, sizeof where, "CPU, %d x %u threads", world, ki.grid);
    } else if (world <= ndev) {
        snprintf(where, sizeof where, use_rccl ? "%d x MI355X, RCCL gather" : "%d x MI355X", world);
    } else {
        snprintf(where, sizeof where, "%d ranks on %d x MI355X", world, ndev);
    }
    printf("MiniRayTracer - Scene: %.0fms - Trace: %.2fs - %.3f Mrays/s | %.3f us/ray  [%s, %u spp, %s numerics]\n", gen_ms,
           secs, (total * 0.000001) / secs, (secs * 1000000.0) / (double)total, where, descs[0].sqrt_samples * descs[0].sqrt_samples,
           p.numerics ? "fast" : "exact");
    if (have_adaptive) {
        // from the moments frame: a pixel refined in pass k has spent more than the passes before it
        const size_t npx = (size_t)p.buffer_width * p.buffer_height;
        double spent = 0;
        for (size_t i = 0; i < npx; i++) spent += mom[i * 4 + 3];
        printf("adaptive: %.2f spp mean, atol %g rtol %g, refined", spent / (double)npx, ap.atol, ap.rtol);
        double before = 0;
        for (int k = 0; k < adaptive; k++) {
            const double sq = (double)(descs[0].sqrt_samples << k);
            before += sq * sq;
            size_t n = 0;
            for (size_t i = 0; i < npx; i++) n += mom[i * 4 + 3] > before;
            printf(" %zu", n);
        }
        printf(" of %zu pixels\n", npx);
        if (samplemap) {
            FILE* f = fopen(samplemap, "wb");
            if (!f) return fail("open -samplemap output", MRT_ERR_IO);
            fprintf(f, "PF\n%u %u\n-1.0\n", p.buffer_width, p.buffer_height);
            for (size_t i = 0; i < npx; i++) {
                const float g[3] = {mom[i * 4 + 3], mom[i * 4 + 3], mom[i * 4 + 3]};
                fwrite(g, 4, 3, f);
            }
            fclose(f);
        }
    }
    printf("rays %llu\n", (unsigned long long)total);

    // -aux / -denoise: the first-hit feature buffers at min(spp, 16) samples -- every rank writes its
    // own pixels of the shared host buffers, as mrt_render does -- then the a-trous filter over the
    // assembled frame, in place of the image -o writes
    if (aux || denoise >= 0) {
        const size_t npx = (size_t)p.buffer_width * p.buffer_height;
        std::vector<float> nrm(npx * 4, 0.0f), alb(npx * 4, 0.0f);
        th.clear();
        for (int r = 0; r < world; r++)
            th.emplace_back([&, r] {
                mrt_render_desc ad = descs[r];
                ad.sqrt_samples = std::min(ad.sqrt_samples, 4u);
                ad.flags = 0;
                sts[r] = mrt_render_aux(scenes[r], &ad, nrm.data(), alb.data());
            });
        for (auto& t : th) t.join();
        for (int r = 0; r < world; r++)
            if (sts[r]) return fail("render_aux", sts[r]);
        if (aux) {
            const std::pair<const char*, const std::vector<float>*> files[2] = {{"_normal.pfm", &nrm}, {"_albedo.pfm", &alb}};
            for (const auto& fl : files) {
                FILE* f = fopen((std::string(aux) + fl.first).c_str(), "wb");
                if (!f) return fail("open -aux output", MRT_ERR_IO);
                fprintf(f, "PF\n%u %u\n-1.0\n", p.buffer_width, p.buffer_height);
                for (size_t i = 0; i < npx; i++) fwrite(&(*fl.second)[i * 4], 4, 3, f);
                fclose(f);
            }
        }
        if (denoise >= 0) {
            mrt_denoise_params dp;
            mrt_default_denoise_params(&dp);
            dp.iterations = (uint32_t)denoise;
            auto t1 = std::chrono::steady_clock::now();
            if ((st = mrt_denoise(img.data(), nrm.data(), alb.data(), p.buffer_width, p.buffer_height, &dp, img.data()))) return fail("denoise", st);
            printf("denoise: %d passes, %.1f ms\n", denoise, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
        }
    }

    if (out && write_image(out, img, p.buffer_width, p.buffer_height)) return 1;
    for (auto* c : comms) mrt_comm_free(c);
    for (auto* s : scenes) mrt_scene_free(s);
    mrt_scene_blob_free(blob);
    return 0;
}
