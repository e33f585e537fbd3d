/* mrt.h -- C-ABI of the MI355X render path (libmrt.so).  Plain C types only; return codes, never
 * exceptions; the library owns device memory, the caller owns all host memory.
 *
 * What each entry point replaces in the reference (Maraneshi/MiniRayTracer, no FFI of its own --
 * the seam is the worker-thread spawn in main(), main.cpp:347-382):
 *
 *   mrt_default_params / mrt_parse_argv   MRT_Params defaults + ParseArgv   cmdline_parser.h:5-18, cmdline_parser.cpp:78-107
 *   mrt_select_scene                      select_scene(scenes, aspect)      scene.cpp:25-49 (+ scene 9)
 *   mrt_scene_upload                      (new) scene -> HBM, once, outside the timed region (main.cpp:309 vs 375)
 *   mrt_render / mrt_render_device        std::thread(draw|draw2) x N over work_queue + trace()
 *                                         main.cpp:66-118, 138-243, 347-382; work_queue.cpp:133-175
 *   mrt_render_join                       the worker threads' join()             main.cpp:490-493
 *   mrt_progress                          work_queue::getPercentDone        work_queue.cpp:142-149, 168-175
 *   rays_out                              G_rayCounter                      main.cpp:55, 68, 403-405
 *   cancel                                G_isRunning                       main.cpp:54, 180, 235
 *   mrt_tonemap_argb                      Drago tone map + ARGB32            main.cpp:416-444, vec3.h:327-333
 *   mrt_lum_max_device/mrt_tonemap_device the same, on the device              main.cpp:421-442
 *   mrt_render_adaptive / mrt_moments     (new) draw()'s fixed sample loop, per pixel as long as its
 *                                         standard error asks                main.cpp:150-167
 *   mrt_make_camera / mrt_scene_set_camera camera's constructor, for a scene that is already
 *                                         uploaded                          camera.h:16-36
 *   mrt_reproject                         (new) carries a frame's samples into the next frame of a
 *                                         sequence; main() renders one still frame
 *   mrt_cast_rays / mrt_cast_rays_device  scene.objects->hit(r, 0.001f, FLT_MAX, rec) for a caller's
 *                                         own rays                          scene_object.h:22, main.cpp:71
 *   mrt_trace_rays / mrt_trace_rays_device trace(r, 0) for a caller's own rays  main.cpp:66-118
 *   mrt_radiance_fold                     draw()'s per-pixel sum, NaN rule and clamp  main.cpp:150-175
 *   mrt_camera_path_probes / mrt_pano_probes / mrt_camera_pixel_rays / mrt_surface_probes (+ _device)
 *                                         (new) whole ranges of ray and probe records made where they are
 *                                         traced; the camera ranges are camera::get_ray  camera.h:38-44
 *
 * Threading: one host thread per device; calls on distinct scenes are thread-safe, calls on the
 * same scene handle are not reentrant.
 */
#ifndef MRT_H
#define MRT_H
#include <stdint.h>
#include "mrt_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mrt_status {
    MRT_OK = 0,
    MRT_ERR_INVALID = 1,     /* bad argument / unsupported scene graph */
    MRT_ERR_NO_DEVICE = 2,   /* no gfx950 device visible */
    MRT_ERR_HIP = 3,         /* HIP runtime error */
    MRT_ERR_OOM = 4,
    MRT_ERR_IO = 5,          /* asset (OBJ / texels) not found or unreadable */
    MRT_ERR_CANCELLED = 6
} mrt_status;

/* MRT_Params (cmdline_parser.h:5-18), same defaults and field meaning. */
typedef struct mrt_params {
    uint32_t window_width, window_height;
    uint32_t buffer_width, buffer_height;
    uint32_t samples_per_pixel;
    uint32_t tile_size;
    uint32_t num_threads;     /* CPU worker threads, as in the reference (0 = all); the GPU backend has none */
    uint32_t max_bounces;
    uint32_t scene_select;
    uint32_t threading_mode;  /* 0 = draw() per-pixel mean, 1 = draw2() progressive average */
    float max_luminance;
    uint32_t delay;
    /* additions (not in the reference): */
    uint64_t seed;            /* path stream-key seed, default = the reference main seed */
    uint32_t gpus;            /* -gpus: GPUs to shard the work_queue tiles over (0 = every visible GPU) */
    uint32_t numerics;        /* -numerics: 0 exact contract, 1 tolerance contract (MRT_RF_FAST) */
    uint32_t backend;         /* -backend: 0 GPU (default), 1 CPU (MRT_DEVICE_CPU, -threads workers, exact) */
    uint32_t order;           /* -order: 0 = per-path stream keys (the GPU's; any thread / GPU count gives
                                 the same image), 1 = the reference's RNG order (one PCG stream per worker
                                 thread, work_queue order; CPU backend only, MRT_RF_REF_ORDER).  Default:
                                 1 with -backend cpu, 0 otherwise */
} mrt_params;

void mrt_default_params(mrt_params* p);
/* Same flags, ranges and warnings as ParseArgv; also -seed.  Returns MRT_OK (the reference never
 * fails on bad values: it warns and keeps the default). -help prints help and returns INVALID. */
mrt_status mrt_parse_argv(int argc, char** argv, mrt_params* p);

/* ---- host scene (select_scene) ------------------------------------------------------------ */
typedef struct mrt_scene_blob mrt_scene_blob;
/* asset_dir: directory holding bunny.obj / wt_teapot.obj (or their packed .tri forms) and
 * earthmap.rgb (stb-decoded texels); NULL = $MRT_ASSET_DIR or the package assets/ directory. */
mrt_status mrt_select_scene(uint32_t scene, float aspect, const char* asset_dir, mrt_scene_blob** out);
mrt_status mrt_scene_blob_view(const mrt_scene_blob* blob, mrt_scene_view* out);
/* JSON dump in the schema of oracle/ref/harness.cpp --h-mode scene (parity fixture check). */
mrt_status mrt_scene_blob_dump_json(const mrt_scene_blob* blob, char** json_out);
void mrt_free_string(char* s);
/* Store the parsed records of an OBJ file as a packed <name>.mesh asset (same parser as
 * mrt_select_scene; used when the .obj itself is not shipped). */
mrt_status mrt_pack_obj(const char* obj_path, const char* out_path);
void mrt_scene_blob_free(mrt_scene_blob* blob);
/* The (initstate, initseq) main() hands its worker threads (main.cpp:357-361): drawn from the main
 * thread's PCG after select_scene consumed what it needs.  Only renders in the reference's own RNG
 * order depend on them (the CPU backend's MRT_RF_REF_ORDER renders, via mrt_set_worker_seeds, and
 * the oracle's restatement); the GPU path keys its streams per path instead. */
mrt_status mrt_worker_seeds(const mrt_scene_blob* blob, uint32_t n_threads, uint64_t* initstate, uint64_t* initseq);

/* ---- device -------------------------------------------------------------------------------- */
mrt_status mrt_init(int* device_count);
typedef struct mrt_scene mrt_scene;
/* device: a HIP device index, or MRT_DEVICE_CPU for the CPU backend -- the same hot-path source
 * compiled for the host (exact numerics contract; worker threads over the work_queue tiles like
 * draw()/draw2(), main.cpp:347-382).  It is only ever chosen explicitly: with no gfx950 device the
 * GPU entry points fail (MRT_ERR_NO_DEVICE), they never fall back to the CPU. */
#define MRT_DEVICE_CPU (-1)
mrt_status mrt_scene_upload(int device, const mrt_scene_view* view, mrt_scene** out);
void mrt_scene_free(mrt_scene* scene);
/* CPU backend only: the drawArgs (initstate, initseq) of each worker thread (main.cpp:127-135,
 * 357-366; from mrt_worker_seeds) for renders with MRT_RF_REF_ORDER, which run n_threads workers. */
mrt_status mrt_set_worker_seeds(mrt_scene* s, uint32_t n_threads, const uint64_t* initstate, const uint64_t* initseq);

typedef struct mrt_render_desc {
    uint32_t width, height;
    uint32_t sqrt_samples;   /* spp = sqrt_samples^2, regular grid (main.cpp:319-332) */
    uint32_t max_bounces;
    float max_luminance;
    uint32_t mode;           /* 0 draw() semantics, 1 draw2() semantics */
    uint64_t seed;           /* stream key: path p -> pcg32_srandom(splitmix64(seed ^ p), p) */
    uint32_t tile_size;      /* work_queue tiles (work_queue.cpp:64-128) */
    uint32_t rank, world;    /* this call renders the tiles (inverted-Hilbert order) dealt to `rank`: rounds of
                                `world` consecutive tiles, each round in its own permutation of the ranks */
    uint32_t chunk_samples;  /* samples per launch (0 = auto, bounded by HBM budget) */
    uint32_t flags;          /* MRT_RF_* */
    uint32_t threads;        /* CPU backend: worker threads (0 = every core); the GPU backend ignores it */
    /* Optional pixel list (an addition; the reference always renders the whole buffer): when
     * non-NULL this call renders exactly these n_pixels row-major pixel indices (row 0 = bottom,
     * each < width*height, no repeats), in this order as its local pixels, instead of the tiles
     * dealt to `rank` -- every sample of each, the same per-path streams, so a listed pixel equals
     * the same pixel of a whole-image render bit for bit.  Caller-owned; read during the call. */
    const uint32_t* pixels;
    uint32_t n_pixels;
} mrt_render_desc;
#define MRT_RF_PATH_DEBUG 0x1u /* also keep per-path radiance + ray counts (mrt_render_debug) */
#define MRT_RF_FAST 0x2u       /* tolerance numerics contract: FMA contraction, hardware rcp/sqrt/rsq,
                                  f32 transcendentals; per-pixel RMSE < 1e-3 vs the reference as
                                  shipped (DESIGN.md "Numerics contracts").  Unset: the exact
                                  contract, bit-for-bit the reference built exact. */
#define MRT_RF_PREVIEW 0x4u    /* keep a progressive preview for mrt_preview: after every launch's
                                  fold, the running image (mode 1: the running average, draw2();
                                  mode 0: the mean of the samples so far) is copied to pinned host
                                  memory in stream order (G_linearBackBuffer as the UI thread reads
                                  it every 33 ms, main.cpp:387-444) */
#define MRT_RF_FOLD_BEHIND 0x8u /* mode 0: fold with a kernel lean enough (8 VGPRs) to run beside
                                   another context's persistent path kernel instead of after it --
                                   for callers that pipeline renders on several streams; slower
                                   when nothing else runs (same bits either way) */
#define MRT_RF_FOLD_ASYNC 0x40u /* GPU, no preview / debug / lean fold: each launch's fold runs on
                                   the context's own stream, beside the NEXT launch's (or render's)
                                   path kernel, instead of after its own (two radiance buffers used in
                                   turn).  The output is complete once mrt_render_join has ordered a
                                   stream after it (or the device is synchronised).  Same bits as the
                                   fold in stream order.  Not for stream capture (the fold's stream is
                                   the context's own).  (ABI 6: was 0x20, the bit of the removed
                                   MRT_RF_SPLIT; 0x20 and every other unknown bit are now rejected
                                   with MRT_ERR_INVALID instead of silently changing meaning.) */
#define MRT_RF_REF_ORDER 0x10u  /* CPU backend: the reference's own RNG order -- worker i draws from
                                   one PCG stream seeded by mrt_set_worker_seeds' i-th pair; mode 0 =
                                   draw() over work_queue_seq (tile -> pixel -> sample), mode 1 =
                                   draw2() over work_queue_dynamic ((tile, sample) items,
                                   work_queue.cpp:133-166).  One thread reproduces the reference's
                                   -threads 1 run bit for bit (its deterministic mode,
                                   cmdline_parser.h:15); world must be 1 */
#define MRT_RF_ALL (MRT_RF_PATH_DEBUG | MRT_RF_FAST | MRT_RF_PREVIEW | MRT_RF_FOLD_BEHIND | MRT_RF_REF_ORDER | MRT_RF_FOLD_ASYNC)

/* ABI version of this header: bumped whenever a flag's meaning or a struct layout changes (6: the
 * MRT_RF_FOLD_ASYNC bit moved to 0x40, mrt_kernel_info gained handover_lost, mrt_comm_* added).
 * A binding checks mrt_abi_version() == MRT_ABI_VERSION before its first call. */
#define MRT_ABI_VERSION 6u
uint32_t mrt_abi_version(void);

void mrt_default_render_desc(const mrt_params* p, mrt_render_desc* d);

/* Number of pixels this rank owns and their row-major indices (row 0 = bottom, like
 * G_linearBackBuffer main.cpp:58) in the order mrt_render_device writes them (d->pixels when set). */
mrt_status mrt_local_pixels(const mrt_render_desc* d, uint32_t* n_out, uint32_t* pixels_out /* may be NULL */);

/* Render into a host W*H*4 float buffer (x,y,z,0 per pixel; only owned pixels are written).
 * Both backends; on the CPU backend the call returns when the render is done (cancel is polled
 * per tile, as G_isRunning at main.cpp:180). */
mrt_status mrt_render(mrt_scene* s, const mrt_render_desc* d, float* rgb_out, uint64_t* rays_out,
                      const volatile int* cancel);
/* GPU backend only.  Render into device memory: d_local = n_local*4 floats in mrt_local_pixels order.  Enqueued on
 * `stream` (hipStream_t or NULL); rays are accumulated into the device uint64 *d_rays; nothing is
 * synchronised and nothing is allocated when the scene's workspace already fits (capturable). */
mrt_status mrt_render_device(mrt_scene* s, const mrt_render_desc* d, float* d_local, uint64_t* d_rays, void* stream);
/* GPU backend only.  Enqueue on `stream` a wait for the context's last mrt_render_device (its
 * fold, on the context's own stream under MRT_RF_FOLD_ASYNC): work enqueued on `stream` afterwards
 * sees its output.  (No-op order for renders whose fold ran on their own stream.) */
mrt_status mrt_render_join(mrt_scene* s, void* stream);
/* Allocate/grow the scene's workspace for d (call once before timing mrt_render_device). */
mrt_status mrt_prepare(mrt_scene* s, const mrt_render_desc* d);
/* Per-path radiance (n_local*spp*3 floats, sample-major: [s][local pixel]) and ray counts of the
 * last render made with MRT_RF_PATH_DEBUG (host copies). */
mrt_status mrt_render_debug(mrt_scene* s, float* path_rgb, uint32_t* path_rays, uint64_t n_paths);
mrt_status mrt_progress(mrt_scene* s, float* pct);
/* The newest preview of the running render, callable from another host thread while it runs: the
 * image after *samples_done samples of every pixel (W*H*4 floats, owned pixels only, as rgb_out of
 * mrt_render), never a mix of two passes (the snapshot is sequence-locked).  GPU backend: renders
 * made with MRT_RF_PREVIEW (samples_done = 0 until the first launch is folded); CPU backend: the
 * framebuffer as far as its tiles are done (every sample of a finished pixel; samples_done = spp
 * once the render is over, 0 before). */
mrt_status mrt_preview(mrt_scene* s, float* rgb_out, uint32_t* samples_done);
/* Device time of the path-kernel launches of the last render (HIP events recorded on the render's
 * stream around each mrt_path_kernel launch); waits for the last one. */
mrt_status mrt_kernel_ms(mrt_scene* s, float* path_ms, uint32_t* launches);

/* Which path kernel the scene runs: feature bits of the scene (FT_* of mrt_trace.h; bit 11 =
 * linear hit program, bit 14 = a volume bounded by a sub-program, DESIGN.md "Kernels"), dynamic LDS bytes per workgroup, grid size in
 * workgroups (of the last render's path-kernel launches; before any render, and for every blocking
 * render, the resident grid, a multiple of n_cu; an MRT_RF_FOLD_ASYNC render of a kernel that leaves
 * wave slots to its retrace and fold -- DESIGN.md round 14 -- runs that grid less a multiple of the
 * launch's 8 work partitions, which need not be a multiple of n_cu), threads per workgroup, the BVH nodes each workgroup keeps in LDS, and the build of
 * the kernel for the last render's numerics: MRT_BUILD_* (the tolerance contract runs the fast,
 * the denormal-flushing or the path-exact build per kernel variant). */
#define MRT_BUILD_EXACT 0u
#define MRT_BUILD_FAST 1u
#define MRT_BUILD_FAST_FTZ 2u
#define MRT_BUILD_PATH_EXACT 3u
typedef struct mrt_kernel_info {
    uint32_t features, kernel_features, lds_bytes, grid, prog_ops, vgprs, wg, tree_nodes, build;
    /* handed_over: paths the fast-arithmetic kernels listed for the exact arithmetic since the
       scene's upload (rounding-critical light samples); handover_lost: listed
       paths beyond a launch's list capacity (they keep their fast radiance; 0 in every BASELINE
       config).  Reading them waits for the scene's last render (its fold included).  n_cu: the compute
       units of the scene's device, which the resident grid is a multiple of (0 on the CPU backend) */
    uint32_t n_cu;
    uint64_t handed_over;
    uint64_t handover_lost;
} mrt_kernel_info;
mrt_status mrt_scene_kernel_info(const mrt_scene* s, mrt_kernel_info* out);

/* Drago adaptive-log tone map of a linear W*H*4 buffer to ARGB32 (main.cpp:416-444, no gamma). */
mrt_status mrt_tonemap_argb(const float* rgb, uint32_t width, uint32_t height, uint32_t* argb_out);
/* The same on the device, in two steps so ranks can combine L_wmax (all_reduce max) in between:
 *   mrt_lum_max_device  *d_lwmax = max(*d_lwmax, max luminance of the n float4 pixels) -- the
 *                       caller zeroes *d_lwmax first (main.cpp:424-429)
 *   mrt_tonemap_device  d_argb[i] = ARGB32(Drago(d_rgb[i]; *d_lwmax)) (main.cpp:430-442)
 * Pixel order is free (e.g. the local-pixel order of mrt_render_device); enqueued on `stream`. */
mrt_status mrt_lum_max_device(const float* d_rgb, uint32_t n, float* d_lwmax, void* stream);
mrt_status mrt_tonemap_device(const float* d_rgb, uint32_t n, const float* d_lwmax, uint32_t* d_argb, void* stream);

/* ---- feature buffers and denoise ---------------------------------------------------------------
 * (an addition; the reference returns the radiance image only.)  First-hit feature buffers for a
 * denoiser, and an edge-avoiding a-trous filter (Dammertz et al. 2010) that uses them.
 *
 * Per pixel, the mean over the desc's sqrt_samples^2 camera rays of the FIRST hit:
 *   normal = (n.x, n.y, n.z, coverage), albedo = (r, g, b, depth); float4 each.
 * Sample s of a pixel uses the render's own stream and camera ray for that (pixel, sample, spp) and
 * one scene hit with tmin 0.001 -- the hit the render's first segment finds.  Per hit: the normal
 * facing the ray (a miss: 0), coverage 1 (miss: 0), depth = the hit's t (miss: 0); albedo = the
 * material's colour (lambertian, isotropic, metal), (1,1,1) (dielectric), the emitted radiance
 * (light: 0 from the back), the miss radiance (sky or 0).  Each channel is the float32 sum over
 * s = 0 .. ns-1 in that order, divided by (float)ns.  Read from the desc: width, height,
 * sqrt_samples, seed, tile_size, rank, world, pixels / n_pixels; flags may be 0 or MRT_RF_FAST
 * (accepted and ignored: the buffers always come from the exact arithmetic, so they are
 * bit-identical on both backends); any other flag bit is MRT_ERR_INVALID. */
mrt_status mrt_render_aux(mrt_scene* s, const mrt_render_desc* d, float* normal_out, float* albedo_out);
        /* host W*H*4 each, owned pixels only, like mrt_render; both backends */
mrt_status mrt_render_aux_device(mrt_scene* s, const mrt_render_desc* d, float* d_normal, float* d_albedo, void* stream);
        /* GPU; n_local float4 each in mrt_local_pixels order; enqueued on `stream`, nothing
           synchronised, nothing allocated once mrt_prepare ran for d (capturable) */

/* The filter: `iterations` passes i = 0.. of the 5x5 B3 kernel at step 2^i, each tap weighted by
 * normal, depth, albedo and colour agreement with the centre; sigma_color is halved every pass.
 * The exact formulas: include/mrt_denoise.h (one source for host and device: same bits).
 * Defaults (mrt_default_denoise_params; chosen on the Cornell box at 16 spp):
 *   iterations 3, sigma_color 8, sigma_normal 32, sigma_albedo 0.3, sigma_depth 0.02
 * Valid: iterations <= 16; sigma_color, sigma_albedo, sigma_depth > 0; sigma_normal >= 0. */
typedef struct mrt_denoise_params { uint32_t iterations; float sigma_color, sigma_normal, sigma_albedo, sigma_depth; } mrt_denoise_params;
void mrt_default_denoise_params(mrt_denoise_params* p);
mrt_status mrt_denoise(const float* rgb, const float* normal, const float* albedo, uint32_t width, uint32_t height,
                       const mrt_denoise_params* p, float* rgb_out);          /* host buffers, row-major W*H*4 */
mrt_status mrt_denoise_device(const float* d_rgb, const float* d_normal, const float* d_albedo, uint32_t width, uint32_t height,
                              const mrt_denoise_params* p, float* d_out, float* d_tmp, void* stream);
        /* whole row-major frames (e.g. after mrt_gather_frame, which moves any float4 shard); d_rgb is not
           written; d_out, d_tmp: W*H float4 each; enqueued, no sync, no allocation */

/* ---- sample moments and the adaptive render ----------------------------------------------------
 * (an addition; the reference spends the same samples on every pixel.)  Per pixel one float4 of
 * moments m = (sum l, sum l^2, n_finite, N_spent) over its samples' luminance l, added in sample
 * order in float32; the standard error of the pixel's mean and the refinement test built on it are
 * include/mrt_adaptive.h's mrt_moments_se and mrt_moments_refine (one source for host and device:
 * same bits).
 *
 * mrt_moments adds a radiance chunk in the render's per-path layout ([s][local pixel] float3, as
 * mrt_render_debug returns it) to moments[slot], slot = slots[local pixel] (no repeats), or the
 * local pixel itself when slots is NULL.  The caller zeroes `moments` first; a second call
 * accumulates on top of the first, so the halves of a pixel's samples may come in two calls.
 * MRT_ERR_INVALID: a null path_rgb / moments, or n_pixels * n_samples == 0. */
mrt_status mrt_moments(const float* path_rgb, uint32_t n_pixels, uint32_t n_samples, const uint32_t* slots, float* moments);
mrt_status mrt_moments_device(const float* d_path_rgb, uint32_t n_pixels, uint32_t n_samples, const uint32_t* d_slots, float* d_moments,
                              void* stream);
        /* GPU; device pointers (d_moments 16-byte aligned); enqueued on `stream`, nothing synchronised,
           nothing allocated (capturable) */
/* Host: refine_out[i] = mrt_moments_refine(moments[i], atol, rtol) (1 or 0) and, when se_out is not
 * NULL, se_out[i] = mrt_moments_se(moments[i]) for n float4 moments -- the adaptive render's own
 * decision, for callers that schedule samples themselves.  Either output may be NULL, not both. */
mrt_status mrt_moments_decide(const float* moments, uint32_t n, float atol, float rtol, uint8_t* refine_out, float* se_out);

/* The adaptive render.  Pass 0 is mrt_render of d as it stands (the same streams, kernels and
 * fold), which also gathers every pixel's moments.  Pass k = 1 .. max_passes renders again, as a
 * pixel list in ascending pass-0 local order, the pixels whose mrt_moments_refine(m, atol, rtol)
 * holds -- on a grid twice as fine each pass (sqrt_samples * 2^k) and with the seed
 * splitmix64(d->seed + k) (uint64 wrap), everything else from d -- and merges each finished pixel c
 * of ns_k samples into the running colour C over N samples:
 *   C = C + (c - C) * ((float)ns_k / (N + (float)ns_k)),  N = N + (float)ns_k   (float32, per channel)
 * while the pixel's moments gain the pass's samples.  It stops early when no pixel refines.  A pixel
 * that is never refined equals mrt_render's pixel bit for bit; max_passes = 0 is mrt_render plus the
 * moments.  Every decision is per pixel, so ranks (d->rank / world) and pixel lists need nothing from
 * each other, and both backends decide alike: their exact-contract results are the same bits.
 *
 * rgb_out, moments_out (may be NULL): W*H*4 floats, owned pixels only, like mrt_render;
 * moments_out's w is the samples spent on the pixel.  rays_out: the sum over the passes.  cancel is
 * handed to every pass and read between them.  Blocks like mrt_render; the host decides between the
 * passes, so there is no device form and the call cannot be captured.
 * Valid: max_passes <= 4; atol, rtol >= 0 and finite; d->mode == 0; d->flags 0 or MRT_RF_FAST; every
 * pass's sqrt_samples^2 below 2^32.
 * Defaults (mrt_default_adaptive_params; chosen on the Cornell box at a 16-spp base):
 *   max_passes 2, atol 0.03, rtol 0 */
typedef struct mrt_adaptive_params { uint32_t max_passes; float atol, rtol; } mrt_adaptive_params;
void mrt_default_adaptive_params(mrt_adaptive_params* p);
mrt_status mrt_render_adaptive(mrt_scene* s, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out,
                               float* moments_out /* may be NULL */, uint64_t* rays_out, const volatile int* cancel);

/* ---- camera and temporal accumulation ----------------------------------------------------------
 * (an addition; the reference renders one still frame from the camera select_scene bakes in.)
 *
 * The camera.  mrt_camera (mrt_scene.h) holds the derived vectors the camera ctor computes
 * (camera.h:16-36); mrt_make_camera is that arithmetic, the one definition the scene builders use
 * too, so mrt_make_camera(mrt_scene_camera_params(blob)) equals the blob view's camera byte for byte.
 * MRT_ERR_INVALID for a degenerate frame: a non-finite field, pos == lookat, up parallel to the view
 * direction, vfov_deg outside (0, 180), aspect <= 0, focus_dist <= 0, aperture < 0. */
typedef struct mrt_camera_params {
    float pos[3], lookat[3], up[3];
    float vfov_deg, aspect, aperture, focus_dist, time0, time1;
} mrt_camera_params;
mrt_status mrt_make_camera(const mrt_camera_params* p, mrt_camera* out);
/* the parameters the scene's builder used (the blob keeps them) */
mrt_status mrt_scene_camera_params(const mrt_scene_blob* blob, mrt_camera_params* out);
/* Replace the camera of an uploaded scene; nothing else of the upload depends on it (the scene
 * tables, the kernel variant and its tables do not read the camera), so no re-upload is needed.
 * Both backends.  Blocks: waits for the scene's pending work (its last mrt_render_device, the fold
 * included, and mrt_render_aux_device), then replaces the camera; renders and feature buffers made
 * afterwards equal those of a scene uploaded with `cam` in its view bit for bit.
 * MRT_ERR_INVALID: null, or a camera with a non-finite field. */
mrt_status mrt_scene_set_camera(mrt_scene* s, const mrt_camera* cam);
/* GPU backend only.  The same in stream order: a one-wave kernel enqueued on `stream` takes *cam by
 * value (read during the call) and stores the record; nothing is synchronised and nothing is
 * allocated (capturable: a replay sets the captured camera again).  Work enqueued on `stream` earlier
 * sees the old camera, later work the new one.  The caller orders it against work on other streams
 * -- that includes the context's own fold stream under MRT_RF_FOLD_ASYNC: call it after
 * mrt_render_join(s, stream). */
mrt_status mrt_scene_set_camera_device(mrt_scene* s, const mrt_camera* cam, void* stream);

/* Temporal reprojection: the new history frame (accumulated rgb, history length N) from the current
 * frame's colour and feature buffers (mrt_render_aux: normal = (n, coverage), albedo = (a, depth))
 * under `cam`, and the previous history frame with the feature buffers and camera it was made with.
 * Each fully covered pixel's world point (pinhole ray through the pixel centre, the mean depth) is
 * projected into the previous camera; the four bilinear taps around it that agree in normal, depth
 * and albedo give the history, which the current colour joins as sample N + 1 (N capped at
 * max_history); a pixel without agreeing taps starts again from (c, 1).  The exact formulas and the
 * operation order: include/mrt_temporal.h (one source for host and device: same bits).
 * Whole row-major W*H float4 frames, row 0 = bottom; hist == NULL is the first frame (prev_normal,
 * prev_albedo and prev_cam are not read): hist_out = (rgb.xyz, 1).  hist_out is a frame of its own
 * (none of the inputs); the inputs are not written.
 * Approximations: the lens is a pinhole at the camera's origin; time0 / time1 are ignored (moving
 * spheres rely on the depth, normal and albedo tests); the depth is the feature buffers' mean t.
 * Defaults (mrt_default_temporal_params; the CPU prototype's, measured again on the Cornell orbit,
 * DESIGN.md): max_history 32, normal_min 0.9, depth_tol 0.02, albedo_tol 0.1, min_weight 0.25
 * Valid: max_history >= 1; normal_min in [-1, 1]; depth_tol, albedo_tol > 0; min_weight in (0, 1];
 * width, height in 1 .. 65536; finite cameras. */
typedef struct mrt_temporal_params { float max_history, normal_min, depth_tol, albedo_tol, min_weight; } mrt_temporal_params;
void mrt_default_temporal_params(mrt_temporal_params* p);
mrt_status mrt_reproject(const float* rgb, const float* normal, const float* albedo, const mrt_camera* cam, const float* hist,
                         const float* prev_normal, const float* prev_albedo, const mrt_camera* prev_cam, uint32_t width, uint32_t height,
                         const mrt_temporal_params* p, float* hist_out);       /* host buffers */
mrt_status mrt_reproject_device(const float* d_rgb, const float* d_normal, const float* d_albedo, const mrt_camera* cam, const float* d_hist,
                                const float* d_prev_normal, const float* d_prev_albedo, const mrt_camera* prev_cam, uint32_t width,
                                uint32_t height, const mrt_temporal_params* p, float* d_hist_out, void* stream);
        /* GPU; device frames (16-byte aligned), host cameras and params (read during the call, passed
           to the kernel by value); enqueued on `stream`, no sync, no allocation (capturable) */

/* ---- ray queries ----------------------------------------------------------------------------------
 * (an addition to this ABI; the reference's scene_object::hit is public to its callers,
 * scene_object.h:22.)  The closest hit of caller rays against an uploaded scene, through the hit
 * code the renders run: picking, focusing, visibility between two points, occlusion bakes.
 *
 * Ray i of a batch (i = 0 .. n-1):
 *   the ray     ray(o, d, time, inside) (ray.h:18-56): d need not be of unit length, the constructor
 *               normalises it (ray.h:30) and takes the direction mask from the argument (ray.h:51);
 *               inside is 0 or 1 (dielectric.h's flag; anything non-zero counts as 1); reserved is
 *               ignored.
 *   the hit     objects->hit(r, 0.001f, FLT_MAX) (main.cpp:71): the render's own first-segment hit
 *               under the exact numerics contract, the call the feature buffers make; tmin is the
 *               reference's 0.001, fixed.
 *   the stream  a constant_volume on the way (volumes.cpp:24) draws from
 *               pcg32_srandom(seed + i, 4242) (uint64 wrap): a batch cut at k is two calls with
 *               `seed` and `seed + k`.
 *   a hit       when the closest hit exists and t <= tmax: hits[i] = (t, p, n, mat) -- t in units of
 *               the normalised direction, n as hit_record::n holds it (not turned towards the ray),
 *               mat the index into mrt_scene_view.materials.
 *   otherwise   hits[i] = (+inf, 0,0,0, 0,0,0, MRT_NO_HIT), exactly those bits.  A tmax that is NaN
 *               or <= 0.001 is a miss; tmax = +inf is the plain closest hit.
 * No ray is rejected: a non-finite o or d yields what the reference's arithmetic yields, a miss
 * included, and the call never faults.  Both backends return the same bits.
 * n == 0: MRT_OK, nothing read, written or enqueued.  MRT_ERR_INVALID: a null pointer; a device
 * pointer that is not 16-byte aligned; mrt_cast_rays_device on a CPU-backend scene. */
typedef struct mrt_ray { float o[3], time; float d[3], tmax; uint32_t inside, reserved[3]; } mrt_ray;   /* 48 B */
typedef struct mrt_hit { float t, p[3]; float n[3]; uint32_t mat; } mrt_hit;                           /* 32 B */
#define MRT_NO_HIT 0xFFFFFFFFu
/* Host records, both backends; returns when hits[] is written.  On a GPU scene it stages through
 * device buffers of its own on a stream of its own and waits only for that work. */
mrt_status mrt_cast_rays(mrt_scene* s, const mrt_ray* rays, uint32_t n, uint64_t seed, mrt_hit* hits);
/* GPU backend only; device records.  Enqueued on `stream`: nothing is synchronised and nothing is
 * allocated (capturable: a replay casts whatever d_rays then holds).  It reads the scene tables and
 * d_rays and writes d_hits, nothing else -- nothing a render writes, so it may sit between two
 * mrt_render_device calls on one stream without changing either -- and needs no mrt_prepare. */
mrt_status mrt_cast_rays_device(mrt_scene* s, const mrt_ray* d_rays, uint32_t n, uint64_t seed, mrt_hit* d_hits, void* stream);
/* The pinhole ray through the centre of pixel (x, y), row 0 = bottom, in the arithmetic of
 * include/mrt_temporal.h step 2 (float32, no contraction, this order):
 *   s = ((float)x + 0.5f) / (float)width, t = ((float)y + 0.5f) / (float)height
 *   o = origin, d = ((llcorner + s horz) + t vert) - origin
 *   time = cam->time0, tmax = +inf, inside = 0, reserved = 0
 * MRT_ERR_INVALID: null, x >= width, y >= height, a zero size. */
mrt_status mrt_camera_pixel_ray(const mrt_camera* cam, uint32_t width, uint32_t height, uint32_t x, uint32_t y, mrt_ray* out);
/* A range of them: record j (j = 0 .. n-1) is mrt_camera_pixel_ray(cam, width, height, pixel % width,
 * pixel / width) bit for bit, pixel = first + j, row-major with row 0 at the bottom;
 * first + n <= width * height.  The host form writes out[0..n).  The device form is enqueued on
 * `stream`: nothing is synchronised and nothing is allocated (capturable); *cam is read at the call
 * and travels in the kernel arguments, so a replay uses the captured camera; it writes d_out[0..n)
 * (16-byte aligned) and nothing else, and takes no scene.
 * n == 0: MRT_OK, nothing read, written or enqueued (null pointers are fine then).  MRT_ERR_INVALID:
 * a null pointer, a misaligned d_out, a zero size, a range that ends past the image. */
mrt_status mrt_camera_pixel_rays(const mrt_camera* cam, uint32_t width, uint32_t height, uint64_t first, uint32_t n, mrt_ray* out);
mrt_status mrt_camera_pixel_rays_device(const mrt_camera* cam, uint32_t width, uint32_t height, uint64_t first, uint32_t n, mrt_ray* d_out,
                                        void* stream);

/* ---- radiance queries -----------------------------------------------------------------------------
 * (an addition to this ABI; the reference's trace(r, 0), main.cpp:66, is what draw() calls per
 * sample.)  Path-traced radiance along caller rays: light and irradiance probes, lightmap texels,
 * radiance caches, cameras that are not the reference's (panorama, fisheye, orthographic, a measured
 * lens), "how bright is it at the point I just picked".
 *
 * Record i of a batch (i = 0 .. n-1):
 *   the ray     ray(o, d, time, inside) exactly as in the ray queries: d need not be of unit length,
 *               make_ray normalises it and takes the direction mask from the argument; inside
 *               non-zero counts as 1.
 *   the stream  the path draws from the PCG32 whose two words are rng_state and rng_inc, used as
 *               given: not re-seeded, and an even rng_inc is not an error.  mrt_probe_seed fills them
 *               as pcg32_srandom(splitmix64(seed ^ path_id), path_id) leaves them: the render's keying.
 *   the path    trace(r, 0) of main.cpp:66-118 under the exact numerics contract: segments until the
 *               path ends, at most max_bounces + 1 of them, folded deepest-first as the recursion
 *               returns.
 *   the result  L = the folded radiance as trace() returns it -- the NaN rule and the luminance clamp
 *               are draw()'s, not trace()'s, and are not applied (mrt_radiance_fold applies them);
 *               rays = the path's trace() calls (its segments).
 * No record is rejected: a non-finite o or d yields what the arithmetic yields, and the call never
 * faults.  Both backends return the same bits, and a batch cut in two is the whole.
 * n == 0: MRT_OK, nothing read, written or enqueued.  MRT_ERR_INVALID: a null pointer; a device
 * pointer that is not 16-byte aligned; a device form on a CPU-backend scene. */
typedef struct mrt_probe { float o[3], time; float d[3]; uint32_t inside; uint64_t rng_state, rng_inc; } mrt_probe;   /* 48 B */
typedef struct mrt_radiance { float L[3]; uint32_t rays; } mrt_radiance;                                           /* 16 B */
void mrt_probe_seed(uint64_t seed, uint64_t path_id, mrt_probe* p);
/* Host records, both backends; returns when out[] is written.  rays_out (may be NULL): the sum of
 * out[i].rays, added up on the host.  On a GPU scene it stages through device buffers, a level
 * workspace and a stream of its own, in pieces of at most MRT_TRACE_PIECE records, and waits only for
 * that work. */
#define MRT_TRACE_PIECE (1u << 20)
mrt_status mrt_trace_rays(mrt_scene* s, const mrt_probe* probes, uint32_t n, uint32_t max_bounces, mrt_radiance* out, uint64_t* rays_out);
/* GPU backend only.  The bytes of fold-level storage mrt_trace_rays_device takes for the kernel's
 * full grid and for one wave: lanes * max(max_bounces, 1) * 16, lanes = 64 for one wave.  Both depend
 * only on the scene's device and max_bounces. */
mrt_status mrt_trace_rays_workspace(const mrt_scene* s, uint32_t max_bounces, uint64_t* bytes_full, uint64_t* bytes_min);
/* GPU backend only; device records, 16-byte aligned (d_work too).  Enqueued on `stream`: nothing is
 * synchronised and nothing is allocated (capturable: a replay traces whatever d_probes then holds).
 * It reads the scene tables and d_probes, writes d_out[0..n) and uses d_work[0..work_bytes) as
 * scratch, nothing else -- nothing of the render workspace, so it needs no mrt_prepare and may sit
 * between two mrt_render_device calls on one stream without changing either.  The grid comes from
 * work_bytes: as many whole waves as the workspace has level rows for, capped at the full grid (and at
 * the waves n records can occupy); fewer bytes than one wave needs is MRT_ERR_INVALID.  The result
 * does not depend on the grid. */
mrt_status mrt_trace_rays_device(mrt_scene* s, const mrt_probe* d_probes, uint32_t n, uint32_t max_bounces, mrt_radiance* d_out, void* d_work,
                                 uint64_t work_bytes, void* stream);
/* draw()'s pixel (main.cpp:150-175) over groups of consecutive records: out[g] (a float4, w = 0) is
 * the mode-0 fold of records g*group .. g*group + group - 1 in record order -- a sample with a
 * non-finite channel is replaced by the running sum (main.cpp:162-164) -- divided by `group` and
 * clamped to max_luminance.  One definition for host and device (include/mrt_radiance.h): the same
 * bits, and the bits of mrt_render's pixel when the records are the pixel's paths in sample order.
 * MRT_ERR_INVALID: a null pointer, group == 0, a device pointer that is not 16-byte aligned;
 * n_groups == 0 is MRT_OK.  The device form is enqueued on `stream` (no sync, no allocation). */
mrt_status mrt_radiance_fold(const mrt_radiance* rad, uint32_t n_groups, uint32_t group, float max_luminance, float* rgb /* n_groups float4 */);
mrt_status mrt_radiance_fold_device(const mrt_radiance* d_rad, uint32_t n_groups, uint32_t group, float max_luminance,
                                    float* d_rgb /* n_groups float4 */, void* stream);
/* The ray total of device records in stream order: *d_rays += the sum of d_rad[i].rays, i = 0 .. n-1 (a
 * device uint64 the caller zeroes, as mrt_render_device's d_rays) -- what mrt_trace_rays' rays_out is
 * for host records, so a device chain copies back pixels and one total, not the records.  Enqueued on
 * `stream`, no sync, no allocation (capturable).  n == 0: MRT_OK, nothing enqueued.  MRT_ERR_INVALID: a
 * null pointer, d_rad not 16-byte aligned, d_rays not 8-byte aligned. */
mrt_status mrt_radiance_rays_device(const mrt_radiance* d_rad, uint32_t n, uint64_t* d_rays, void* stream);
/* One record on the host (ranges, on the host or the device: mrt_camera_path_probes below).  The start
 * of the render's path (pixel, sample) under `cam` and d: the stream keyed by
 * path_id = pixel * ns + sample under d->seed (ns = sqrt_samples^2), the sample-grid offsets of
 * main.cpp:319-332 (sample = i * sqrt_samples + j: ((i + 0.5) / sq, (j + 0.5) / sq)), then
 * camera::get_ray's arithmetic (camera.h:38-44): o, the UN-normalised direction argument, time,
 * inside = 0, and the stream's two words as they stand AFTER the camera's draws.  mrt_trace_rays of
 * it is the render's path: same radiance bits, same ray count.  Reads d->width, height,
 * sqrt_samples and seed.  MRT_ERR_INVALID: null, a zero size, pixel >= width * height,
 * sample >= ns. */
mrt_status mrt_camera_path_probe(const mrt_camera* cam, const mrt_render_desc* d, uint32_t pixel, uint32_t sample, mrt_probe* out);
/* One record on the host (ranges: mrt_pano_probes below).  The same grid and keying for an
 * equirectangular camera at p->pos: 360 by 180 degrees,
 * the image centre looks at p->lookat, p->up is up; no lens (aperture, vfov, aspect and focus_dist
 * are not read).  With (u, v, w) the camera frame of p (camera.h:27-29: w = normalize(pos - lookat),
 * u = normalize(cross(up, w)), v = cross(w, u)), (x, y) the pixel (row 0 = bottom) and (dx, dy) the
 * sample's grid offsets, in float32 without contraction, in this order:
 *   s = ((float)x + dx) / (float)width,  t = ((float)y + dy) / (float)height
 *   phi = (s - 0.5f) * 6.2831855f,  theta = (t - 0.5f) * 3.1415927f
 *   a = cos(theta) * sin(phi),  b = sin(theta),  c = cos(theta) * cos(phi)     (mrt_mathfn.h mrt_sinf / mrt_cosf)
 *   d = ((a * u + b * v) - c * w),  o = pos
 *   time = fma(time1 - time0, randf, time0) with the path's first draw (camera.h:41), inside = 0
 * and the stream's words after that one draw.  MRT_ERR_INVALID: as mrt_camera_path_probe, or a
 * degenerate frame (mrt_make_camera's rule for pos, lookat, up, time0, time1). */
mrt_status mrt_pano_probe(const mrt_camera_params* p, const mrt_render_desc* d, uint32_t pixel, uint32_t sample, mrt_probe* out);

/* ---- probe generators -----------------------------------------------------------------------------
 * Whole ranges of the records above, made on the host or -- the _device forms -- where they are traced:
 * generate -> mrt_trace_rays_device -> mrt_radiance_fold_device is a chain of enqueues on one stream,
 * and so is mrt_camera_pixel_rays_device -> mrt_cast_rays_device -> mrt_surface_probes_device -> trace
 * -> fold.  Host and device forms return the same bits (one definition, csrc/mrt_probegen.h).
 *
 * Every device form: enqueued on `stream`; nothing is synchronised and nothing is allocated
 * (capturable); cam, p and d are host structs, read at the call, that travel in the kernel arguments --
 * a replay uses the captured values; it writes d_out[0..n) and nothing else; d_out and the other
 * device pointers are 16-byte aligned.  No form takes a scene.
 * Both forms: n == 0 (n_hits == 0) is MRT_OK -- nothing is read, written or enqueued, null pointers are
 * fine then.  MRT_ERR_INVALID: a null pointer, a misaligned device pointer, a zero size, a range that
 * ends past the render, and the per-record forms' own rules (a degenerate panorama frame, an image
 * above 2^32 pixels: pixel indices are 32-bit).
 *
 * The two probe ranges.  Record j (j = 0 .. n-1) is path q = first + j of the render d, counted
 * pixel-major: pixel = q / ns, sample = q % ns, ns = sqrt_samples^2, pixels row-major with row 0 at the
 * bottom; first + n <= width * height * ns.  Record j of mrt_camera_path_probes equals
 * mrt_camera_path_probe(cam, d, pixel, sample) bit for bit, record j of mrt_pano_probes equals
 * mrt_pano_probe(p, d, pixel, sample).  A range of whole pixels in this order is what
 * mrt_radiance_fold takes with group = ns. */
mrt_status mrt_camera_path_probes(const mrt_camera* cam, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* out);
mrt_status mrt_camera_path_probes_device(const mrt_camera* cam, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* d_out,
                                         void* stream);
mrt_status mrt_pano_probes(const mrt_camera_params* p, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* out);
mrt_status mrt_pano_probes_device(const mrt_camera_params* p, const mrt_render_desc* d, uint64_t first, uint32_t n, mrt_probe* d_out,
                                  void* stream);
/* Surface probes: cosine-distributed directions leaving the points of hit records (mrt_cast_rays'
 * output) -- irradiance probes, lightmap texels, ambient occlusion with a sky.  With
 * sq = sqrt_per_hit >= 1, P = sq^2 and n_hits * P < 2^32, record j = i * P + k belongs to hit i and
 * stratum k of a sq x sq grid, in float32 without contraction, in this order:
 *   a = k / sq,  b = k % sq
 *   the stream  mrt_probe_seed(seed, first_id + j) (uint64 wrap), then u1 = randf, then u2 = randf; the
 *               record holds the two words as they stand after the two draws.  A miss takes the draws
 *               as well: the stream never depends on the hit, and a batch cut at c is two calls with
 *               first_id and first_id + c * P.
 *   r1 = ((float)a + u1) / (float)sq,  r2 = ((float)b + u2) / (float)sq            (IEEE division)
 *   z = sqrt(1 - r2),  s = sqrt(r2)   (correctly rounded),   phi = (2 * 3.1415927f) * r1
 *   vec = (cos(phi) * s, sin(phi) * s, z)                    (the sincos of mrt_mathfn.h mrt_sincos_d)
 *   w = hits[i].n; with `rays` given, w = -n when dot(n, rays[i].d) > 0 (the normal faces the ray; a
 *       NaN dot does not turn it)
 *   d = onb(w) * vec  (onb.h:19-27),  o = hits[i].p,  time = rays ? rays[i].time : 0,  inside = 0
 * The direction is cosine-weighted about w, so pi * mean(L) over a hit's P records estimates the
 * irradiance there.  This is deliberately NOT the reference's random_cosine_direction, whose x and y
 * carry a factor 2 (pcg.cpp:92-93) that the ray constructor then normalises into a distribution that
 * is not cosine-weighted.  The reference's fixed tmin = 0.001 keeps the path off its own surface, as in
 * every scatter.
 * A miss (hits[i].mat == MRT_NO_HIT) gives o = d = 0, time = 0, inside = 0 and the stream's words;
 * tracing that record returns what the arithmetic yields for a null direction (one segment, no fault).
 * Callers mask by mat.  `rays` may be NULL; d_hits, d_rays and d_out are 16-byte aligned.
 * MRT_ERR_INVALID also for sqrt_per_hit == 0 and n_hits * P >= 2^32. */
mrt_status mrt_surface_probes(const mrt_hit* hits, const mrt_ray* rays /* may be NULL */, uint32_t n_hits, uint32_t sqrt_per_hit, uint64_t seed,
                              uint64_t first_id, mrt_probe* out);
mrt_status mrt_surface_probes_device(const mrt_hit* d_hits, const mrt_ray* d_rays /* may be NULL */, uint32_t n_hits, uint32_t sqrt_per_hit,
                                     uint64_t seed, uint64_t first_id, mrt_probe* d_out, void* stream);

/* ---- the contract's transcendentals as array calls --------------------------------------------
 * The functions of include/mrt_mathfn.h that the formulas above are written in (and the tone map's
 * and the filter's), on arrays: out[i] = f(a[i]) or f(a[i], b[i]), each one evaluation in double and
 * one rounding to float, the same bits on the host and on the device.  The trigonometric functions
 * are defined for |x| < 2^20 (and +-inf and NaN, which give NaN); a finite argument past that is
 * outside the contract.  `b` is read by MRT_FN_ATAN2 and MRT_FN_POW only and may be NULL otherwise.
 * mrt_mathfn_device is enqueued on `stream` (a hipStream_t), allocates and synchronises nothing, can
 * be captured, runs one thread per element and writes exactly n results.  MRT_ERR_INVALID for a null
 * pointer or an unknown `which`; n == 0 is a no-op. */
enum {
    MRT_FN_SIN = 0, MRT_FN_COS = 1, MRT_FN_TAN = 2, MRT_FN_LOG = 3, MRT_FN_LOG10 = 4, MRT_FN_ASIN = 5, MRT_FN_EXP = 6,
    MRT_FN_POW5 = 7,  /* x^5 */
    MRT_FN_ATAN2 = 8, /* atan2(a, b) */
    MRT_FN_POW = 9    /* pow(a, b): a^5 by MRT_FN_POW5's products when b == 5 */
};
mrt_status mrt_mathfn(uint32_t which, uint32_t n, const float* a, const float* b, float* out);
mrt_status mrt_mathfn_device(uint32_t which, uint32_t n, const float* d_a, const float* d_b, float* d_out, void* stream);
/* The double cores those functions round, called exactly as the header defines them, on double
 * arrays: mrt_sincos_d (out = sin, out2 = cos; |a| < 2^20), mrt_log_d, mrt_exp_d, mrt_atan2_d(a, b).
 * `out2` is written by MRT_FND_SINCOS only and may be NULL otherwise, `b` is read by MRT_FND_ATAN2
 * only.  The same contract as above: host and device give the same bits. */
enum { MRT_FND_SINCOS = 0, MRT_FND_LOG = 1, MRT_FND_EXP = 2, MRT_FND_ATAN2 = 3 };
mrt_status mrt_mathfn_d(uint32_t which, uint32_t n, const double* a, const double* b, double* out, double* out2);
mrt_status mrt_mathfn_d_device(uint32_t which, uint32_t n, const double* d_a, const double* d_b, double* d_out, double* d_out2, void* stream);

/* ---- multi-GPU: the framebuffer gather over RCCL (xGMI) ---------------------------------------
 * The reference's seam is main.cpp:347-382 (the worker threads over one work_queue) writing
 * G_linearBackBuffer (main.cpp:58): here each rank renders the work_queue tiles dealt to it
 * (mrt_render_desc.rank / world) on its own GPU, and ONE RCCL gather of the equal-size padded shards
 * to the root plus one device scatter assembles the W*H framebuffer on the root's GPU; ray counts
 * are summed with one all-reduce.  RCCL is loaded at mrt_comm_init_* (librccl.so.1: the copy already
 * in the process, else the loader's search path, else /opt/rocm/lib; $MRT_RCCL_LIB overrides);
 * without it those calls fail with MRT_ERR_NO_DEVICE.  Collective calls (mrt_gather_frame,
 * mrt_render_gather) are made by every rank of the communicator, one host thread (or process) per
 * rank. */
typedef struct mrt_comm mrt_comm;
#define MRT_COMM_ID_BYTES 128
/* one process per GPU: rank 0 makes the id (ncclGetUniqueId) and hands it to the others out of band */
mrt_status mrt_comm_unique_id(uint8_t id[MRT_COMM_ID_BYTES]);
mrt_status mrt_comm_init_rank(int device, uint32_t world, uint32_t rank, const uint8_t id[MRT_COMM_ID_BYTES], mrt_comm** out);
/* one process driving `world` GPUs (ncclCommInitAll): comms_out[r] is rank r on devices[r] */
mrt_status mrt_comm_init_all(uint32_t world, const int* devices, mrt_comm** comms_out);
void mrt_comm_free(mrt_comm* c);
/* Pixels of the largest rank shard of d's tile deal (the gather's padded shard, in pixels). */
mrt_status mrt_gather_shard_pixels(const mrt_render_desc* d, uint32_t* n_out);
/* Collective, enqueued on `stream` (the caller has ordered it after its render, mrt_render_join):
 * this rank's d_local (mrt_render_device output: n_local float4 in mrt_local_pixels order, d.rank
 * = the communicator's rank, d.world = its size, no pixel list) goes to the root with one
 * ncclGather of the padded shards; on the root the shards are scattered into d_frame (W*H float4,
 * row-major, row 0 = bottom, like G_linearBackBuffer; other ranks pass NULL).  d_rays (device
 * uint64, may be NULL) is summed over the ranks in place (ncclAllReduce), in the same group. */
mrt_status mrt_gather_frame(mrt_comm* c, const mrt_render_desc* d, const float* d_local, float* d_frame, uint64_t* d_rays,
                            void* stream);
/* The drop-in for one worker thread of main.cpp:347-382 on its own GPU: renders this rank's tiles
 * (mrt_render_device into the communicator's buffers), gathers the frame to the root over RCCL and,
 * on the root, copies it to rgb_out (W*H*4 floats, every pixel; other ranks may pass NULL).  The ray
 * total of all ranks goes to *rays_out on every rank (may be NULL).  Returns when this rank's part is
 * done. */
mrt_status mrt_render_gather(mrt_scene* s, mrt_comm* c, const mrt_render_desc* d, float* rgb_out, uint64_t* rays_out);

const char* mrt_strerror(mrt_status s);
const char* mrt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
