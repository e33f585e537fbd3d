// mrt_context.h -- the scene context behind the C-ABI's mrt_scene handle, as the host units share it:
// mrt_upload.hip fills it, mrt_render.hip sizes its workspace and renders with it, mrt_query.hip runs
// the aux, cast and trace launches on it.  Plain aggregates, no accessors; no kernel is named here.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <mutex>
#include <string>
#include <vector>

#include "mrt_internal.h"  // (HIPCHK)
#include "mrt_launch.h"
#include "mrt_cpu.h"

#define MRT_GPU_ONLY(s, what) \
    if ((s) && (s)->cpu) return mrt_internal_fail(MRT_ERR_INVALID, what " is a GPU-backend entry point (scene on MRT_DEVICE_CPU)")

// Wave slots an MRT_RF_FOLD_ASYNC launch leaves free for its own retrace and fold (DESIGN.md, round
// 14): the Cornell walk kernel (box6_walk), whose one-wave groups take all eight wave slots of every
// SIMD and which is bound by VALU issue, not by its wave count, is launched with kSideSlots fewer
// groups (a multiple of MRT_NPART: every work partition gives up as many waves), and the retrace
// and the fold, both one-wave groups of at most kSideVgprs registers, run in those slots on the
// context's own stream while the next launch's path kernel already runs on the caller's.  Every
// other kernel keeps its grid: the exact contract's Cornell kernel (seven waves per SIMD) lost 5 %
// and the room + mesh kernel 1.5 % with the same slots gone (profiles/r14_ab.txt section 5).
// 768 of the MI355X's 8192: the Cornell kernel is VALU-issue bound and runs no slower without them,
// while the fold of a 3 GB launch in 512 slots outlasted the kernel beside it (profiles/r14_ab.txt).
static constexpr int kSideSlots = 768;
static constexpr int kSideVgprs = 64;
// Beside the path kernel the fold lasts about as long as that kernel does (6.2 of 6.35 ms at depth 32),
// and the launch after next waits for it: with a depth limit of 1 / 2 / 3 the kernel is short enough
// for the step to become the fold's (+3.8 % / +1.0 % / -0.2 % against the full grid, -1.0 % from 4 on),
// so launches of fewer than 4 bounces keep the full grid and the retrace on the render's stream.
static constexpr uint32_t kSideMinBounces = 4;
// rounding-critical paths listed per launch (mrt_shade.h light_critical; a full list loses the rest,
// which keep their fast radiance): measured ~1e-5 per path in the Cornell scenes
static constexpr uint32_t kRtCap = 1u << 20;
// one-wave groups of the retrace kernel: 16384 lanes, a path each (more loop); its time is the longest
// listed path's, plus the launch
static constexpr uint32_t kRetraceGroups = 256;
// (Round 6: the retrace of an MRT_RF_FOLD_ASYNC launch beside the next launch's path kernel -- on the
// context's fold stream, and there in one-wave slots the next kernel left free -- measured slower:
// the previous launch's fold uses the GPU during the retrace's gap on the render's stream, and behind
// the retrace on the fold stream it got only the free slots, profiles/r06_ab.txt sections 2 and 7.
// Round 14 does it with slots for both, a fold of one-wave groups and a retrace of at most 64
// registers: kSideSlots.)

// one numerics build of the scene's path kernel (exact / fast): kernel, grid, registers
struct PathLaunch {
    mrtd::path_kernel_t fn = nullptr;
    int grid = 0;
    int side = 0;  // one-wave groups an MRT_RF_FOLD_ASYNC launch leaves out of the grid: wave slots for its retrace and fold (kSideSlots)
    size_t lds_bytes = 0;
    uint32_t vgprs = 0;
    uint32_t wg = 64;     // threads per workgroup
    uint32_t tree_n = 0;  // BvhWide nodes kept in each workgroup's LDS (treelet kernels)
    uint32_t lds_save = 0;  // LDS words per lane slot for the query ray parked during instances
    bool rewrite = false;   // the kernel runs the tolerance-contract program rewrite (s->prog_fast)
    mrtd::path_kernel_t retrace = nullptr;  // the exact arithmetic for its rounding-critical paths (mrt_retrace_kernel)
    bool handover = false;  // the kernel hands its rounding-critical paths to it (fast arithmetic)
    bool retrace_side = false;  // the retrace kernel fits a side slot (at most kSideVgprs registers)
    uint32_t walk_min = 32;  // resumable mesh walk threshold of this build (PathParams::walk_min)
};

// Before the workspace is rewritten or reallocated: wait for the last enqueued render of this
// context (it may still run on a caller stream that the synchronous uploads do not order against).
// (Library-internal like launch_params below: neither is an exported symbol.)
__attribute__((visibility("hidden"))) mrt_status quiesce(mrt_scene* s);

// A buffer on the device, grown on demand and freed with its scene.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // the bytes asked for
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // a workspace buffer (mrt_prepare): at least `bytes` (a zero-byte request gets 16); before it
    // reallocates, waits for the scene's last enqueued render (quiesce)
    mrt_status grow(mrt_scene* s, size_t bytes) {
        if (cap >= bytes && p) return MRT_OK;
        if (mrt_status st = quiesce(s)) return st;
        return regrow(bytes, "workspace allocation failed");
    }
    // a blocking query's staging buffer: no quiesce (the call synchronises its own stream before it returns)
    mrt_status grow_own(size_t bytes, const char* what) { return cap >= bytes && p ? MRT_OK : regrow(bytes, what); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }

private:
    mrt_status regrow(size_t bytes, const char* what) {
        release();
        hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 16);
        if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, what);
        cap = bytes;
        return MRT_OK;
    }
};

// The 64-byte device scratch of a scene, zeroed at upload.  The retrace kernels reach its words through
// RetraceList (mrt_shade.h) and mrt_scene_kernel_info copies it whole: the byte offsets are fixed.
struct RenderScratch {
    unsigned long long handed_over;  // paths handed to the exact arithmetic since upload
    uint32_t rt_count0, pad0_;       // parity 0: rounding-critical paths listed by the launch
    unsigned long long rays;         // ray total of mrt_render
    uint32_t rt_done0, pad1_;        // parity 0: retrace groups done
    uint64_t cancel;                 // cancel flag (the path kernel polls its low word as an int)
    unsigned long long lost;         // listed beyond the cap since upload
    uint32_t rt_count1, rt_done1;    // parity 1: the list's count and retrace groups done
    uint64_t pad2_;
};
static_assert(sizeof(RenderScratch) == 64, "the device scratch is 64 bytes");
static_assert(offsetof(RenderScratch, handed_over) == 0 && offsetof(RenderScratch, rt_count0) == 8 && offsetof(RenderScratch, rays) == 16 &&
                  offsetof(RenderScratch, rt_done0) == 24 && offsetof(RenderScratch, cancel) == 32 && offsetof(RenderScratch, lost) == 40 &&
                  offsetof(RenderScratch, rt_count1) == 48 && offsetof(RenderScratch, rt_done1) == 52,
              "the scratch words keep their device byte offsets");

// the render workspace: what mrt_prepare sizes for a desc
struct RenderWorkspace {
    mrt_render_desc wdesc{};
    std::vector<uint32_t> wpixels;   // the pixel list of wdesc (mrt_render_desc.pixels), copied
    bool have = false;
    uint32_t npix = 0, chunk = 0;
    DevBuf<uint2> d_pixels;
    DevBuf<float2> d_sdist;
    uint32_t sdist_sq = 0;
    DevBuf<float> d_rad;
    DevBuf<uint32_t> d_path_rays;
    DevBuf<float4> d_acc;
    DevBuf<float4> d_lev;
    uint32_t lev_rows = 0;
    DevBuf<float4> d_out;            // mrt_render's device framebuffer (local-pixel order)
    DevBuf<uint32_t> d_rt;           // rounding-critical paths listed for the retrace kernel (path indices)
    DevBuf<uint64_t> d_counters;     // one work counter per chunk launch (progress reads them)
    uint32_t slot_half = 0;  // launch slots per set (renders use set rpar at rpar * slot_half; mrt_prepare)
};

// progress of the current render (mrt_progress, mrt_kernel_ms) and the cancel flag's plumbing
struct RenderProgress {
    std::vector<uint64_t> chunk_paths;
    hipStream_t pstream = nullptr;   // non-blocking stream for the cancel-flag copy
    // host-coherent pinned memory: per-launch snapshots of the work counters, stored by the path
    // kernel itself (mrt_progress reads them with no GPU work), and the cancel flag's source
    uint64_t* h_prog = nullptr;
    size_t h_prog_cap = 0;
    std::vector<uint64_t> h_seen;  // largest snapshot read per launch (waves store out of order)
    int* h_one = nullptr;
    std::atomic<uint32_t> n_chunks{0};  // launches of the current render (0 until all are enqueued)
    // mrt_progress may run on another host thread: it and every change to the launch bookkeeping
    // (h_prog, h_seen, ev, chunk_paths) and to the preview below hold this lock
    std::mutex mu;
    uint32_t base = 0;  // launch slot of the current render's counters and progress snapshots
    std::vector<hipEvent_t> ev;  // [2*k]: start/stop of path-kernel launch k of the last render
    uint32_t n_launch = 0;
};

// progressive preview (MRT_RF_PREVIEW): device staging image, pinned host copy guarded by a
// sequence word the render's stream writes around each copy (odd = copy in flight) and the
// sample count the copy holds
struct RenderPreview {
    DevBuf<float4> d_prev;
    float4* h_prev = nullptr;
    size_t h_prev_cap = 0;
    uint32_t* h_seq = nullptr;       // [0] sequence, [1] samples folded into h_prev
    uint32_t epoch = 0;
    std::vector<uint32_t> px;        // local pixel -> row-major pixel of the previewed render
    uint32_t w = 0, h = 0;
};

// MRT_RF_FOLD_ASYNC: launches alternate between two radiance buffers (parity lpar), renders
// between two sets of counter slots (rpar); the fold of parity p runs on fstream and ev_fold[p]
// marks its end, which the next path kernel writing parity p's radiance buffer waits for (folds
// run in order on fstream, so it also orders every earlier fold)
struct AsyncFold {
    hipStream_t fstream = nullptr;
    hipEvent_t ev_kern = nullptr;
    hipEvent_t ev_fold[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    uint32_t lpar = 0, rpar = 0;
    DevBuf<float> d_rad2;
};

// The blocking mrt_cast_rays / mrt_trace_rays on a GPU scene: a stream and staging records of their
// own (rays, then hits; probes, then radiance, and the fold-level workspace of the trace launches),
// so a call waits for its own work only; kept until the scene is freed
struct QueryStaging {
    hipStream_t cast_stream = nullptr;
    DevBuf<char> d_cast;
    hipStream_t trace_stream = nullptr;
    DevBuf<char> d_trace;
    DevBuf<char> d_trace_work;
};

struct mrt_scene {
    int device = 0;
    mrt_cpu_scene* cpu = nullptr;  // MRT_DEVICE_CPU: the CPU backend's scene (mrt_cpu.hip); nothing below is used
    mrtd::DScene S{};
    mrtd::DScene* d_S = nullptr;
    std::vector<void*> allocs;
    uint32_t n_nodes = 0;
    const mrtd::LinOp* prog_fast = nullptr;  // the tolerance contract's program for the interpreter (lin_rewrite_fast)
    RenderScratch* d_scratch = nullptr;
    RenderWorkspace ws;
    RenderProgress prog;
    RenderPreview prev;
    AsyncFold fold;
    QueryStaging query;
    // recorded at the end of every mrt_render_device on the caller's stream: workspace changes
    // (relayout uploads, reallocation) wait for it, so a render still running on another stream
    // never sees its buffers rewritten or freed
    hipEvent_t ev_done = nullptr;
    bool ev_done_pending = false;
    // the same for the last mrt_render_aux_device (it reads the pixel table and the sample grid)
    hipEvent_t ev_aux = nullptr;
    bool ev_aux_pending = false;
    uint32_t n_cu = 0;
    uint32_t features = 0, variant = 0;
    uint32_t lds_frames = 0, lds_rays = 0, lds_mesh = 0, lds_save = 0;
    uint32_t walk_min = 32;  // resumable mesh walk threshold (PathParams::walk_min)
    PathLaunch pl[2];            // [0] exact contract, [1] tolerance contract (MRT_RF_FAST)
    size_t max_threads = 0;  // largest path-kernel grid in threads (per-lane level rows)
    uint64_t last_paths = 0;
    uint32_t last_numerics = 0;
    uint32_t last_grid = 0;  // path-kernel groups of the last render's launches (0: none yet)
    uint32_t prog_ops = 0;  // linear hit program length (0: generic machine)
    // the adaptive render's moments sink (internal, mrt_render_adaptive): while mom is set, every
    // launch chunk's radiance is also added to mom[mom_slots ? mom_slots[lp] : lp] (mrt_moments_kernel)
    // on the render's stream, after the chunk's fold and before the next launch reuses the buffer
    float* mom = nullptr;
    const uint32_t* mom_slots = nullptr;
    // its refinement passes' pixel lists come from mrt_internal_refine_slots over checked pixels (in
    // range, no repeats): mrt_prepare skips the list check (a sort) for them
    bool trust_pixels = false;
};

// The LDS of a one-wave launch that only walks (the retrace and aux kernels): the generic machine's
// frames and transformed rays, the mesh / bvh_node walk's stack, `lds_save` words for the query ray
// parked during instances (mrt_launch.h WaveLds, which the kernels index it by).
static inline mrtd::WaveLds walk_lds(const mrt_scene* s, uint32_t lds_save) {
    return mrtd::WaveLds{s->lds_frames, s->lds_rays, s->lds_mesh, lds_save};
}
// ... and the same four words in a launch's parameters (PathParams, CastParams, ProbeParams)
template <typename Params>
static inline void set_walk_lds(Params& P, const mrt_scene* s, uint32_t lds_save) {
    P.lds_frames = s->lds_frames;
    P.lds_rays = s->lds_rays;
    P.lds_mesh = s->lds_mesh;
    P.lds_save = lds_save;
}

// What a render launch and the aux launch share of PathParams (after mrt_prepare): the scene, the
// build's LDS stack words, the pixel table and the sample grid, the image and the path streams.
__attribute__((visibility("hidden"))) mrtd::PathParams launch_params(const mrt_scene* s, const PathLaunch& PL, const mrt_render_desc* d);
