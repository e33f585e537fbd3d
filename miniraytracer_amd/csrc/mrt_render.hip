// mrt_render.hip -- the render entry points of the MI355X backend behind the C-ABI (include/mrt.h):
// mrt_prepare sizes the scene context's workspace (mrt_context.h) for a desc, mrt_render_device
// enqueues a render's launches -- per chunk the path kernel (mrt_kernels.hip), the retrace of its
// rounding-critical paths, the fold (mrt_fold.h) and, previewed, a snapshot -- and mrt_render, the
// adaptive driver, camera, progress and preview sit on top of it.  The launch arithmetic is
// mrt_plan.h's; no kernel is defined here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <unistd.h>

#include "mrt_context.h"
#include "mrt_fold.h"
#include "mrt_plan.h"
#include "mrt_moments.h"

using namespace mrtd;

static bool same_layout(const mrt_render_desc& a, const std::vector<uint32_t>& a_px, const mrt_render_desc& b) {
    if (a.width != b.width || a.height != b.height || (a.pixels != nullptr) != (b.pixels != nullptr)) return false;
    if (b.pixels) return a_px.size() == b.n_pixels && std::equal(a_px.begin(), a_px.end(), b.pixels);
    return a.tile_size == b.tile_size && a.rank == b.rank && a.world == b.world;
}

// Before the workspace is rewritten or reallocated: wait for the last enqueued render of this
// context (it may still run on a caller stream that the synchronous uploads do not order against).
mrt_status quiesce(mrt_scene* s) {
    if (s->ev_done_pending) {
        HIPCHK(hipEventSynchronize(s->ev_done));
        s->ev_done_pending = false;
    }
    if (s->ev_aux_pending) {
        HIPCHK(hipEventSynchronize(s->ev_aux));
        s->ev_aux_pending = false;
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_prepare(mrt_scene* s, const mrt_render_desc* d) {
    MRT_GPU_ONLY(s, "mrt_prepare");
    if (!s || !d || d->width == 0 || d->height == 0 || d->sqrt_samples == 0 || (d->world && d->rank >= d->world))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_prepare: bad desc");
    // the path kernel's u = (x + dx) / W by one reciprocal is exact up to 2^24 (mrt_kernels.hip)
    if (d->width > (1u << 24) || d->height > (1u << 24))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_prepare: width / height above 2^24 pixels");
    // every GPU entry point renders in per-path stream order (mrt_render_device and mrt_render come here)
    if (d->flags & MRT_RF_REF_ORDER)
        return mrt_internal_fail(MRT_ERR_INVALID, "MRT_RF_REF_ORDER is a CPU-backend mode (the GPU keys its PCG streams per path)");
    mrt_status st;
    if (!s->trust_pixels && (st = mrt_internal_check_pixels(d))) return st;
    HIPCHK(hipSetDevice(s->device));
    bool relayout = !s->ws.have || !same_layout(s->ws.wdesc, s->ws.wpixels, *d);
    uint32_t ns = d->sqrt_samples * d->sqrt_samples;
    if (relayout) {
        std::vector<uint32_t> px = mrt_internal_local_pixels(d);
        std::vector<uint2> xy(px.size());
        for (size_t i = 0; i < px.size(); i++) xy[i] = make_uint2(px[i] % d->width, px[i] / d->width);
        if ((st = quiesce(s))) return st;
        if ((st = s->ws.d_pixels.grow(s, xy.size() * 8))) return st;
        HIPCHK(hipMemcpy(s->ws.d_pixels.p, xy.data(), xy.size() * 8, hipMemcpyHostToDevice));
        s->ws.npix = (uint32_t)px.size();
    }
    if (s->ws.sdist_sq != d->sqrt_samples) {  // sample grid of main.cpp:319-332, in float like the reference
        const uint32_t sq = d->sqrt_samples;
        std::vector<float2> sd((size_t)sq * sq);
        for (uint32_t i = 0; i < sq; i++)
            for (uint32_t j = 0; j < sq; j++)
                sd[(size_t)i * sq + j] = make_float2(((float)i + 0.5f) / (float)sq, ((float)j + 0.5f) / (float)sq);
        if ((st = quiesce(s))) return st;
        if ((st = s->ws.d_sdist.grow(s, sd.size() * 8))) return st;
        HIPCHK(hipMemcpy(s->ws.d_sdist.p, sd.data(), sd.size() * 8, hipMemcpyHostToDevice));
        s->ws.sdist_sq = sq;
    }
    const uint32_t chunk = plan_chunk(s->ws.npix, ns, d->chunk_samples, d->flags);
    if (chunk == 0) return mrt_internal_fail(MRT_ERR_INVALID, "image too large for one launch");
    if (chunk != s->ws.chunk && (st = quiesce(s))) return st;  // the fold of a running render reads `chunk` rows
    s->ws.chunk = chunk;
    size_t paths = (size_t)s->ws.npix * s->ws.chunk;
    if ((st = s->ws.d_rad.grow(s, paths * 12))) return st;
    if (d->flags & MRT_RF_FOLD_ASYNC) {
        if (d->flags & (MRT_RF_PREVIEW | MRT_RF_PATH_DEBUG | MRT_RF_FOLD_BEHIND))
            return mrt_internal_fail(MRT_ERR_INVALID, "MRT_RF_FOLD_ASYNC: no preview, debug or lean fold");
        if ((st = s->fold.d_rad2.grow(s, paths * 12))) return st;
        if (!s->fold.fstream) HIPCHK(hipStreamCreateWithFlags(&s->fold.fstream, hipStreamNonBlocking));
        if (!s->fold.ev_kern) HIPCHK(hipEventCreateWithFlags(&s->fold.ev_kern, hipEventDisableTiming));
        for (hipEvent_t& e : s->fold.ev_fold)
            if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // (two lists: one per radiance parity of the async fold)
    if ((d->flags & MRT_RF_FAST) && !(d->flags & MRT_RF_PATH_DEBUG) && s->pl[1].handover &&
        (st = s->ws.d_rt.grow(s, (size_t)2 * kRtCap * sizeof(uint32_t))))
        return st;
    if ((st = s->ws.d_acc.grow(s, (size_t)s->ws.npix * 16))) return st;
    if ((st = s->ws.d_out.grow(s, (size_t)s->ws.npix * 16 + 16))) return st;
    if (d->flags & MRT_RF_PREVIEW) {
        if ((st = s->prev.d_prev.grow(s, (size_t)s->ws.npix * 16 + 16))) return st;
        std::lock_guard<std::mutex> lk(s->prog.mu);
        if (s->prev.h_prev_cap < s->ws.npix) {
            if ((st = quiesce(s))) return st;
            if (s->prev.h_prev) (void)hipHostFree(s->prev.h_prev);
            s->prev.h_prev = nullptr;
            s->prev.h_prev_cap = 0;
            HIPCHK(hipHostMalloc((void**)&s->prev.h_prev, (size_t)s->ws.npix * 16 + 16, hipHostMallocPortable));
            s->prev.h_prev_cap = s->ws.npix;
        }
        if (!s->prev.h_seq) {
            HIPCHK(hipHostMalloc((void**)&s->prev.h_seq, 64, hipHostMallocPortable | hipHostMallocCoherent));
            memset(s->prev.h_seq, 0, 64);
        }
        if (relayout || s->prev.px.size() != s->ws.npix) {
            s->prev.px = mrt_internal_local_pixels(d);
        }
        s->prev.w = d->width;
        s->prev.h = d->height;
    }
    if (d->flags & MRT_RF_PATH_DEBUG)
        if ((st = s->ws.d_path_rays.grow(s, paths * 4))) return st;
    s->ws.lev_rows = std::max<uint32_t>(d->max_bounces, 1);
    if ((st = s->ws.d_lev.grow(s, (size_t)s->ws.lev_rows * s->max_threads * 16))) return st;
    // two sets of counter slots / progress snapshots at fixed offsets (mrt_plan.h SlotPlan)
    const SlotPlan slots = plan_slots(ns, s->ws.chunk, s->ws.slot_half);
    const uint32_t half = slots.half, launches = slots.launches;
    const size_t cnt_words = (size_t)MRT_CNT_SLOTS * MRT_COUNTER_STRIDE;  // per launch
    {
        const size_t bytes = (size_t)launches * cnt_words * 8;
        const bool kept = s->ws.d_counters.p && s->ws.d_counters.cap >= bytes;
        if ((st = s->ws.d_counters.grow(s, bytes))) return st;
        // zeroed once at allocation; afterwards every render's final kernel leaves them zero
        if (!kept) HIPCHK(hipMemset(s->ws.d_counters.p, 0, s->ws.d_counters.cap));
    }
    if (!s->prog.pstream) HIPCHK(hipStreamCreateWithFlags(&s->prog.pstream, hipStreamNonBlocking));
    if (!s->ev_done) HIPCHK(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    if (!s->ev_aux) HIPCHK(hipEventCreateWithFlags(&s->ev_aux, hipEventDisableTiming));
    {
        std::lock_guard<std::mutex> lk(s->prog.mu);
        if (s->prog.h_prog_cap < (size_t)launches) {
            if ((st = quiesce(s))) return st;
            if (s->prog.h_prog) (void)hipHostFree(s->prog.h_prog);
            s->prog.h_prog = nullptr;
            s->prog.h_prog_cap = 0;
            HIPCHK(hipHostMalloc((void**)&s->prog.h_prog, (size_t)launches * MRT_NPART * 8, hipHostMallocPortable | hipHostMallocCoherent));
            memset(s->prog.h_prog, 0, (size_t)launches * MRT_NPART * 8);  // later: reset by each render's final kernel
            s->prog.h_prog_cap = launches;
        }
        s->ws.slot_half = half;  // (both buffers now hold 2 * half launches)
        if (s->prog.h_seen.size() < (size_t)launches * MRT_NPART) s->prog.h_seen.resize((size_t)launches * MRT_NPART, 0);
        if (s->prog.chunk_paths.size() < launches) s->prog.chunk_paths.resize(launches, 0);
        while (s->prog.ev.size() < 2 * (size_t)launches) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            s->prog.ev.push_back(e);
        }
    }
    if (!s->prog.h_one) {
        HIPCHK(hipHostMalloc((void**)&s->prog.h_one, sizeof(int), hipHostMallocPortable));
        *s->prog.h_one = 1;
    }
    if (relayout) s->ws.wpixels = d->pixels ? std::vector<uint32_t>(d->pixels, d->pixels + d->n_pixels) : std::vector<uint32_t>();
    s->ws.wdesc = *d;
    s->ws.wdesc.pixels = nullptr;  // (the caller's list is not kept; wpixels holds a copy)
    if (d->pixels) s->ws.wdesc.pixels = s->ws.wpixels.data();
    s->ws.have = true;
    return MRT_OK;
}

// What a render launch and the aux launch share of PathParams (after mrt_prepare): the scene, the
// build's LDS stack words, the pixel table and the sample grid, the image and the path streams.
PathParams launch_params(const mrt_scene* s, const PathLaunch& PL, const mrt_render_desc* d) {
    PathParams P{};
    P.sc = s->S;
    set_walk_lds(P, s, PL.lds_save);
    P.pixels = s->ws.d_pixels.p;
    P.sdist = s->ws.d_sdist.p;
    P.npix = s->ws.npix;
    P.inv_npix = 1.0 / (double)std::max<uint32_t>(s->ws.npix, 1);
    P.width = d->width;
    P.height = d->height;
    P.inv_w = 1.0f / (float)d->width;
    P.inv_h = 1.0f / (float)d->height;
    P.fast_uv = 1;  // checked by mrt_prepare (and sq < 2^16 since sq^2 fits in 32 bits)
    P.sq = d->sqrt_samples;
    P.ns = d->sqrt_samples * d->sqrt_samples;
    P.seed = d->seed;
    return P;
}

// ---- mrt_render_device: a render as a loop over launch chunks ----
// What the steps below share of one call.  The sequence each stream sees: per chunk, on the caller's
// stream q, [wait for the parity's last fold] start event, path kernel, stop event, [retrace]; then the
// fold on q (with the moments sink and the preview snapshot behind it) or, MRT_RF_FOLD_ASYNC, on fstream
// once fstream follows q -- with the retrace behind that point too when it fits a side slot.
struct RenderRun {
    mrt_scene* s;
    const mrt_render_desc* d;
    const PathLaunch* PL;
    hipStream_t q;              // the caller's stream
    float4* out;                // the caller's output, local-pixel order
    unsigned long long* rays;   // the ray total the launches add to
    uint32_t ns, launches;
    bool preview, async, lean;
    bool handover;              // the launches list rounding-critical paths for the retrace
    int side, grid;             // one-wave groups left out of the path kernel's grid, and the grid
    bool rside;                 // the retrace runs in side slots, on fstream
    unsigned long long *d_cnt, *h_prog;  // the render's set of counter slots and progress snapshots
    uint32_t seq;               // preview snapshots so far
};

// Progress bookkeeping, the render's set of counter slots, the wait for pending folds, the preview's reset.
// No clearing fills enqueued here: the first fold chunk starts from +0 instead of reading the
// accumulator, and the work counters and progress snapshots were left zero by the previous
// render's final kernel (stream order; zeroed at allocation before the first).  The cancel flag
// is clear unless a cancelled mrt_render set it, and that clears it again before returning.
static mrt_status render_begin(RenderRun& R) {
    mrt_scene* const s = R.s;
    {
        std::lock_guard<std::mutex> lk(s->prog.mu);
        for (uint32_t k = 0; k < R.launches; k++) {
            s->prog.chunk_paths[k] = (uint64_t)s->ws.npix * (std::min(R.ns, (k + 1) * s->ws.chunk) - k * s->ws.chunk);
            // the host's running maxima only: a snapshot is read only once this render's launch k
            // has started (its start event), i.e. after the previous render's final kernel reset it
            for (uint32_t j = 0; j < MRT_NPART; j++) s->prog.h_seen[(size_t)k * MRT_NPART + j] = 0;
        }
    }
    s->prog.n_launch = 0;
    s->last_numerics = (R.d->flags & MRT_RF_FAST) ? 1u : 0u;
    // MRT_RF_FOLD_ASYNC: each launch writes the radiance buffer of its parity, whose last fold (on
    // fstream) must have ended first; the render uses the counter slots of its parity (the previous
    // render's folds may still reset theirs).  Any other render waits for every pending fold.
    const uint32_t rpar = R.async ? s->fold.rpar : 0u;
    if (R.async) s->fold.rpar ^= 1u;
    if (!R.async)
        for (uint32_t p = 0; p < 2; p++)
            if (s->fold.pending[p]) HIPCHK(hipStreamWaitEvent(R.q, s->fold.ev_fold[p], 0));
    {
        std::lock_guard<std::mutex> lk(s->prog.mu);
        s->prog.base = rpar * s->ws.slot_half;
    }
    R.d_cnt = (unsigned long long*)(s->ws.d_counters.p + (size_t)rpar * s->ws.slot_half * MRT_CNT_SLOTS * MRT_COUNTER_STRIDE);
    R.h_prog = (unsigned long long*)(s->prog.h_prog + (size_t)rpar * s->ws.slot_half * MRT_NPART);
    R.seq = 0;
    if (R.preview) {  // a new render: no snapshot yet (sequence 0), in stream order
        std::lock_guard<std::mutex> lk(s->prog.mu);
        HIPCHK(hipStreamWriteValue32(R.q, s->prev.h_seq + 1, 0u, 0));
        HIPCHK(hipStreamWriteValue32(R.q, s->prev.h_seq, 0u, 0));
        s->prev.epoch++;
    }
    s->last_grid = (uint32_t)R.grid;
    return MRT_OK;
}

// the radiance parity of the next launch; an async launch waits for the last fold out of its buffer
static mrt_status chunk_parity(RenderRun& R, uint32_t* par) {
    mrt_scene* const s = R.s;
    *par = R.async ? s->fold.lpar : 0u;
    if (R.async) {
        s->fold.lpar ^= 1u;
        if (s->fold.pending[*par]) HIPCHK(hipStreamWaitEvent(R.q, s->fold.ev_fold[*par], 0));
    }
    return MRT_OK;
}

// the parameters of the launch of samples [s0, s1) into the radiance buffer of parity par
static PathParams chunk_params(const RenderRun& R, uint32_t s0, uint32_t s1, uint32_t par) {
    mrt_scene* const s = R.s;
    const mrt_render_desc* const d = R.d;
    const PathLaunch& PL = *R.PL;
    PathParams P = launch_params(s, PL, d);
    // the interpreter's tolerance-contract program (rooms and box.h lists as slab tests); the
    // shape-specialised walks read the program as compiled
    if ((d->flags & MRT_RF_FAST) && s->prog_fast && PL.rewrite) P.sc.prog = s->prog_fast;
    P.walk_min = PL.walk_min;
    P.tree_src = reinterpret_cast<const float4*>(s->S.bwide);
    P.tree_n = PL.tree_n;
    P.s0 = s0;
    plan_partitions(P, s->ws.npix * (s1 - s0), R.grid, PL.wg / 64u);
    P.max_bounces = d->max_bounces;
    P.rad = par ? s->fold.d_rad2.p : s->ws.d_rad.p;
    P.path_rays = (d->flags & MRT_RF_PATH_DEBUG) ? s->ws.d_path_rays.p : nullptr;
    P.counter = R.d_cnt + (size_t)s->prog.n_launch * MRT_CNT_SLOTS * MRT_COUNTER_STRIDE;
    P.hprog = R.h_prog + (size_t)s->prog.n_launch * MRT_NPART;
    P.cancel = (const int*)&s->d_scratch->cancel;
    P.rays = R.rays;
    P.lev = s->ws.d_lev.p;
    P.lev_rows = s->ws.lev_rows;
    // the list of the launch's radiance parity: entries at par * kRtCap, its count and its groups-done word
    if (R.handover) {
        RenderScratch* const X = s->d_scratch;
        P.rt = RetraceList{s->ws.d_rt.p + (size_t)par * kRtCap, par ? &X->rt_count1 : &X->rt_count0, kRtCap,
                           par ? &X->rt_done1 : &X->rt_done0, &X->handed_over, &X->lost};
    }
    return P;
}

// the path kernel between the start and stop events of its launch slot
static mrt_status enqueue_path(RenderRun& R, const PathParams& P) {
    mrt_scene* const s = R.s;
    HIPCHK(hipEventRecord(s->prog.ev[2 * s->prog.n_launch], R.q));
    hipLaunchKernelGGL(R.PL->fn, dim3(R.grid), dim3(R.PL->wg), R.PL->lds_bytes, R.q, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->prog.ev[2 * s->prog.n_launch + 1], R.q));
    s->prog.n_launch++;
    return MRT_OK;
}

// fstream goes on behind what the caller's stream holds so far
static mrt_status fstream_follows(RenderRun& R) {
    HIPCHK(hipEventRecord(R.s->fold.ev_kern, R.q));
    HIPCHK(hipStreamWaitEvent(R.s->fold.fstream, R.s->fold.ev_kern, 0));
    return MRT_OK;
}

// This launch's rounding-critical paths, exact, into the radiance buffer before its fold (the
// exact arithmetic walks the program as compiled: the tolerance contract's rewrite has ops -- a
// room's slab test, one-step box instances -- only the fast builds compile).
// (With side slots: on fstream in front of the fold, so the caller's stream goes straight on to
// the next launch; the list it empties is its parity's, which the launch after next fills only
// after ev_fold[par].)
static mrt_status enqueue_retrace(RenderRun& R, const PathParams& P) {
    mrt_scene* const s = R.s;
    PathParams PR = P;
    PR.sc.prog = s->S.prog;
    PR.lds_save = s->lds_save;  // (the exact arithmetic parks a ray where the Cornell walk does not)
    hipLaunchKernelGGL(R.PL->retrace, dim3(kRetraceGroups), dim3(64), walk_lds(s, PR.lds_save).bytes(), R.rside ? s->fold.fstream : R.q, PR);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

// The fold of the chunk [s0, s1) out of d_rad.  The last chunk's full fold finishes the render (no
// preview: no snapshot of acc needed; the 8-VGPR lean fold cannot take the division as well: a final
// kernel follows it); an MRT_RF_FOLD_ASYNC render has neither preview nor lean fold (mrt_prepare).
// Async: on the fold stream, beside the next launch's path kernel (with side slots: one-wave groups,
// as many as the launch left free -- a 256-thread group needs a free slot on all four SIMDs of a CU
// at once).  Otherwise on the caller's stream, the adaptive render's moments sink behind it.
static mrt_status enqueue_fold(RenderRun& R, const float* d_rad, uint32_t s0, uint32_t s1, uint32_t par) {
    mrt_scene* const s = R.s;
    const mrt_render_desc* const d = R.d;
    const bool last = s1 == R.ns && !R.preview && !R.lean;
    const FoldEnd fe{last ? R.out : nullptr, R.ns, last ? R.d_cnt : nullptr, last ? R.h_prog : nullptr,
                     last ? R.launches * MRT_CNT_SLOTS : 0u, last ? R.launches * MRT_NPART : 0u};
    if (R.async) {
        if (mrt_status st = mrt_fold_enqueue(R.side ? FoldShape::AsyncSide : FoldShape::Async, R.side ? (uint32_t)R.side : s->n_cu, d_rad,
                                             s->ws.d_acc.p, s->ws.npix, s0, s1, d->mode, d->max_luminance, fe, s->fold.fstream))
            return st;
        HIPCHK(hipEventRecord(s->fold.ev_fold[par], s->fold.fstream));
        s->fold.pending[par] = true;
        return MRT_OK;
    }
    if (mrt_status st = mrt_fold_enqueue(R.lean ? FoldShape::Lean : FoldShape::Full, 0u, d_rad, s->ws.d_acc.p, s->ws.npix, s0, s1, d->mode,
                                         d->max_luminance, fe, R.q))
        return st;
    if (s->mom) return mrt_internal_moments_enqueue(d_rad, s->ws.npix, s1 - s0, s->mom_slots, s->mom, R.q);
    return MRT_OK;
}

// the image after s1 samples, copied to the host under the sequence lock
static mrt_status enqueue_preview(RenderRun& R, uint32_t s1) {
    mrt_scene* const s = R.s;
    if (mrt_status st = mrt_final_enqueue(s->ws.d_acc.p, s->prev.d_prev.p, s->ws.npix, s1, R.d->mode, R.d->max_luminance, nullptr, nullptr, 0u, 0u, R.q))
        return st;
    HIPCHK(hipStreamWriteValue32(R.q, s->prev.h_seq, 2 * R.seq + 1, 0));
    HIPCHK(hipMemcpyAsync(s->prev.h_prev, s->prev.d_prev.p, (size_t)s->ws.npix * 16, hipMemcpyDeviceToHost, R.q));
    HIPCHK(hipStreamWriteValue32(R.q, s->prev.h_seq + 1, s1, 0));
    HIPCHK(hipStreamWriteValue32(R.q, s->prev.h_seq, 2 * R.seq + 2, 0));
    R.seq++;
    return MRT_OK;
}

// the trailing final kernel of a previewed or lean-folded render (otherwise the last fold wrote the
// output and reset the counters), and the event that marks the render's end
static mrt_status render_end(RenderRun& R) {
    mrt_scene* const s = R.s;
    if (R.preview || R.lean)
        if (mrt_status st = mrt_final_enqueue(s->ws.d_acc.p, R.out, s->ws.npix, R.ns, R.d->mode, R.d->max_luminance, R.d_cnt, R.h_prog,
                                              R.launches * MRT_CNT_SLOTS, R.launches * MRT_NPART, R.q))
            return st;
    HIPCHK(hipEventRecord(s->ev_done, R.async ? s->fold.fstream : R.q));
    s->ev_done_pending = true;
    s->prog.n_chunks.store(R.launches, std::memory_order_release);  // progress reads start once every launch and its events are enqueued
    return MRT_OK;
}

extern "C" mrt_status mrt_render_device(mrt_scene* s, const mrt_render_desc* d, float* d_local, uint64_t* d_rays, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_device");
    if (!s || !d || !d_local) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_device: null");
    s->prog.n_chunks.store(0, std::memory_order_release);  // progress: a new render, not started
    mrt_status st = mrt_prepare(s, d);
    if (st) return st;
    RenderRun R{};
    R.s = s;
    R.d = d;
    R.PL = &s->pl[(d->flags & MRT_RF_FAST) ? 1 : 0];
    R.q = (hipStream_t)stream;
    R.out = (float4*)d_local;
    R.rays = d_rays ? (unsigned long long*)d_rays : &s->d_scratch->rays;
    R.ns = d->sqrt_samples * d->sqrt_samples;
    R.launches = (R.ns + s->ws.chunk - 1) / s->ws.chunk;
    R.preview = (d->flags & MRT_RF_PREVIEW) != 0;
    R.async = (d->flags & MRT_RF_FOLD_ASYNC) != 0;
    R.lean = (d->flags & MRT_RF_FOLD_BEHIND) && d->mode == 0;
    // the rounding-critical paths' hand-over: tolerance contract, not the per-path debug output
    // (whose radiance is the fast kernel's own)
    R.handover = R.PL->handover && !(d->flags & MRT_RF_PATH_DEBUG);
    // MRT_RF_FOLD_ASYNC on a kernel that fills every SIMD: PL.side groups fewer, whose wave slots the
    // launch's retrace and fold take on fstream (kSideSlots).  Per-path streams: which wave runs a
    // path changes neither the image nor the ray total.
    // (not below kSideMinBounces: a shallow launch's kernel is shorter than its fold runs beside it)
    R.side = R.async && d->max_bounces >= kSideMinBounces ? R.PL->side : 0;
    R.grid = R.PL->grid - R.side;
    R.rside = R.side && R.PL->retrace_side;
    if ((st = render_begin(R))) return st;
    for (uint32_t s0 = 0; s0 < R.ns; s0 += s->ws.chunk) {
        const uint32_t s1 = std::min(R.ns, s0 + s->ws.chunk);
        uint32_t par;
        if ((st = chunk_parity(R, &par))) return st;
        const PathParams P = chunk_params(R, s0, s1, par);
        if ((st = enqueue_path(R, P))) return st;
        // the retrace on the caller's stream, or behind the point where fstream follows it
        if (R.handover && !R.rside && (st = enqueue_retrace(R, P))) return st;
        if (R.async && (st = fstream_follows(R))) return st;
        if (R.handover && R.rside && (st = enqueue_retrace(R, P))) return st;
        if ((st = enqueue_fold(R, P.rad, s0, s1, par))) return st;
        if (R.preview && (st = enqueue_preview(R, s1))) return st;
        s->last_paths = P.n_paths;
    }
    return render_end(R);
}

// mrt_render on the GPU up to the end of the wait: the render of d into the scene's device
// framebuffer (d_out, local-pixel order; s->ws.npix pixels) and its ray total (d_rays), both complete
// when it returns.  *cancelled: the caller's flag stopped it (a partial image).
static mrt_status render_wait(mrt_scene* s, const mrt_render_desc* d, const volatile int* cancel, bool* was_cancelled) {
    *was_cancelled = false;
    s->prog.n_chunks.store(0, std::memory_order_release);
    if (cancel && *cancel) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled");
    mrt_render_desc dc = *d;  // a cancellable render runs as >= 16 launches; cancel lands between them
    const uint32_t ns = d->sqrt_samples * d->sqrt_samples;
    // (so does a previewed one: each launch adds a snapshot)
    if ((cancel || (dc.flags & MRT_RF_PREVIEW)) && dc.chunk_samples == 0 && !(dc.flags & MRT_RF_PATH_DEBUG))
        dc.chunk_samples = std::max(1u, ns / 16);
    d = &dc;
    mrt_status st = mrt_prepare(s, d);
    if (st) return st;
    HIPCHK(hipMemset(&s->d_scratch->rays, 0, 8));
    st = mrt_render_device(s, d, (float*)s->ws.d_out.p, (uint64_t*)&s->d_scratch->rays, nullptr);
    if (st) return st;
    // wait, forwarding the caller's cancel flag to the device flag the path kernel polls
    bool cancelled = false;
    if (!cancel) {
        HIPCHK(hipEventSynchronize(s->ev_done));
    } else {
        for (;;) {
            const hipError_t q = hipEventQuery(s->ev_done);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(q));
            if (*cancel && !cancelled) {
                HIPCHK(hipMemcpyAsync(&s->d_scratch->cancel, s->prog.h_one, sizeof(int), hipMemcpyHostToDevice, s->prog.pstream));
                HIPCHK(hipStreamSynchronize(s->prog.pstream));
                cancelled = true;
            }
            usleep(200);
        }
    }
    s->ev_done_pending = false;
    if (cancelled) HIPCHK(hipMemset(&s->d_scratch->cancel, 0, 8));  // the render is over: clear the flag for the next one
    *was_cancelled = cancelled;
    return MRT_OK;
}

extern "C" mrt_status mrt_render(mrt_scene* s, const mrt_render_desc* d, float* rgb_out, uint64_t* rays_out, const volatile int* cancel) {
    if (!s || !d || !rgb_out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render: null");
    if (s->cpu) return mrt_cpu_render(s->cpu, d, rgb_out, rays_out, cancel);
    bool cancelled = false;
    if (mrt_status st = render_wait(s, d, cancel, &cancelled)) return st;
    std::vector<float> local((size_t)s->ws.npix * 4);
    std::vector<uint32_t> px = mrt_internal_local_pixels(d);
    HIPCHK(hipMemcpy(local.data(), s->ws.d_out.p, local.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < px.size(); i++) memcpy(rgb_out + (size_t)px[i] * 4, &local[i * 4], 16);
    uint64_t rays = 0;
    HIPCHK(hipMemcpy(&rays, &s->d_scratch->rays, 8, hipMemcpyDeviceToHost));
    if (rays_out) *rays_out = rays;
    if (cancelled) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (partial image)");
    return MRT_OK;
}

// ---- the adaptive render (include/mrt.h "sample moments and the adaptive render") ----
// The call's own device buffers: the running colour C and the moments m of the pass-0 local pixels
// (one slot each) and the slot map of the current refinement pass.  Every pass is a render_wait --
// mrt_render's own path, stream-ordered fold included -- with the moments sink set; a refinement
// pass lands in the scene's d_out in list order and mrt_merge_kernel folds it into C through the
// slot map.  The decision runs on the host from a copy of the moments.
namespace {
struct AdaptiveBufs {  // one allocation: C, then m (n float4 each), then the slot map
    float *C = nullptr, *m = nullptr;
    uint32_t* slots = nullptr;
    mrt_scene* s = nullptr;
    ~AdaptiveBufs() {
        if (s) s->mom = nullptr, s->mom_slots = nullptr, s->trust_pixels = false;
        if (C) (void)hipFree(C);
    }
};
}  // namespace

static mrt_status render_adaptive_gpu(mrt_scene* s, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out, float* moments_out,
                                      uint64_t* rays_out, const volatile int* cancel) {
    HIPCHK(hipSetDevice(s->device));
    const std::vector<uint32_t> px0 = mrt_internal_local_pixels(d);
    const uint32_t n0 = (uint32_t)px0.size();
    AdaptiveBufs B;
    if (hipMalloc((void**)&B.C, (size_t)n0 * 36 + 16) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "mrt_render_adaptive: device buffers");
    B.m = B.C + (size_t)n0 * 4;
    B.slots = (uint32_t*)(B.m + (size_t)n0 * 4);
    HIPCHK(hipMemset(B.m, 0, (size_t)n0 * 16));
    B.s = s;  // (from here on the sink is unset on every way out)
    uint64_t total = 0;
    if (rays_out) *rays_out = 0;
    // one pass: the render with the sink set; its pixels are then in d_out, its rays added to the total
    auto pass = [&](const mrt_render_desc* dk, const uint32_t* d_slots) -> mrt_status {
        s->mom = B.m;
        s->mom_slots = d_slots;
        s->trust_pixels = d_slots != nullptr;  // a refinement pass: the list is this call's own
        bool cancelled = false;
        const mrt_status st = render_wait(s, dk, cancel, &cancelled);
        s->mom = nullptr;
        s->mom_slots = nullptr;
        s->trust_pixels = false;
        if (st) return st;
        uint64_t rays = 0;
        HIPCHK(hipMemcpy(&rays, &s->d_scratch->rays, 8, hipMemcpyDeviceToHost));
        total += rays;
        if (rays_out) *rays_out = total;
        if (cancelled) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (partial image)");
        return MRT_OK;
    };
    mrt_status st = pass(d, nullptr);
    if (st) return st;
    HIPCHK(hipMemcpy(B.C, s->ws.d_out.p, (size_t)n0 * 16, hipMemcpyDeviceToDevice));
    float N = (float)(d->sqrt_samples * d->sqrt_samples);
    std::vector<float> hm((size_t)n0 * 4);
    std::vector<uint32_t> list;
    for (uint32_t k = 1; k <= p->max_passes; k++) {
        if (cancel && *cancel) return mrt_internal_fail(MRT_ERR_CANCELLED, "cancelled (between passes)");
        HIPCHK(hipMemcpy(hm.data(), B.m, hm.size() * 4, hipMemcpyDeviceToHost));
        const std::vector<uint32_t> slots = mrt_internal_refine_slots(hm.data(), n0, p->atol, p->rtol);
        if (slots.empty()) break;
        list.resize(slots.size());
        for (size_t j = 0; j < slots.size(); j++) list[j] = px0[slots[j]];
        HIPCHK(hipMemcpy(B.slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
        const mrt_render_desc dk = mrt_internal_adaptive_pass(d, k, list.data(), (uint32_t)list.size());
        if ((st = pass(&dk, B.slots))) return st;
        const float nsf = (float)(dk.sqrt_samples * dk.sqrt_samples);
        if ((st = mrt_internal_merge_enqueue((const float*)s->ws.d_out.p, (uint32_t)slots.size(), B.slots, B.C, N, nsf, nullptr))) return st;
        HIPCHK(hipStreamSynchronize(nullptr));  // (the next pass may regrow d_out; the slot map is rewritten)
        N = N + nsf;
    }
    std::vector<float> local((size_t)n0 * (moments_out ? 8 : 4));  // C, then m: one copy
    HIPCHK(hipMemcpy(local.data(), B.C, local.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < px0.size(); i++) memcpy(rgb_out + (size_t)px0[i] * 4, &local[i * 4], 16);
    if (moments_out)
        for (size_t i = 0; i < px0.size(); i++) memcpy(moments_out + (size_t)px0[i] * 4, &local[((size_t)n0 + i) * 4], 16);
    return MRT_OK;
}

extern "C" mrt_status mrt_render_adaptive(mrt_scene* s, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out,
                                          float* moments_out, uint64_t* rays_out, const volatile int* cancel) {
    if (mrt_status st = mrt_internal_adaptive_check(s, d, p, rgb_out)) return st;
    if (s->cpu) return mrt_cpu_render_adaptive(s->cpu, d, p, rgb_out, moments_out, rays_out, cancel);
    return render_adaptive_gpu(s, d, p, rgb_out, moments_out, rays_out, cancel);
}

// the worker threads' join (main.cpp:490-493) as stream order: `stream` waits for the context's
// last render, including a fold on the context's own stream (MRT_RF_FOLD_ASYNC)
int mrt_internal_scene_device(const mrt_scene* s) { return s->cpu ? MRT_DEVICE_CPU : s->device; }

extern "C" mrt_status mrt_render_join(mrt_scene* s, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_join");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_join: null");
    if (!s->ev_done) return MRT_OK;  // no render yet
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, s->ev_done, 0));
    return MRT_OK;
}

// ---- the camera of an uploaded scene (include/mrt.h "camera and temporal accumulation") ----
// Every kernel reads the camera through DScene::camp at each path start (mrt_shade.h camera_ray);
// DScene::cam, the copy inside the struct (the host's s->S, handed to every launch by value, and the
// uploaded d_S), is read by no kernel and is kept equal to it.  Nothing else of an upload depends on
// the camera: the scene tables, the variant choice and the Cornell hit table do not read it.
static mrt_status camera_check(const char* who, const mrt_scene* s, const mrt_camera* cam) {
    if (!s || !cam) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    const float* f = (const float*)cam;
    for (size_t i = 0; i < sizeof(mrt_camera) / 4; i++)
        if (!std::isfinite(f[i])) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": a camera with a non-finite field").c_str());
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_set_camera(mrt_scene* s, const mrt_camera* cam) {
    if (mrt_status st = camera_check("mrt_scene_set_camera", s, cam)) return st;
    if (s->cpu) {
        mrt_cpu_set_camera(s->cpu, cam);
        return MRT_OK;
    }
    HIPCHK(hipSetDevice(s->device));
    if (mrt_status st = quiesce(s)) return st;  // the context's last render (its fold included) and feature buffers
    HIPCHK(hipMemcpy(const_cast<mrt_camera*>(s->S.camp), cam, sizeof(mrt_camera), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char*)s->d_S + offsetof(DScene, cam), cam, sizeof(mrt_camera), hipMemcpyHostToDevice));
    s->S.cam = *cam;
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_set_camera_device(mrt_scene* s, const mrt_camera* cam, void* stream) {
    MRT_GPU_ONLY(s, "mrt_scene_set_camera_device");
    if (mrt_status st = camera_check("mrt_scene_set_camera_device", s, cam)) return st;
    HIPCHK(hipSetDevice(s->device));
    if (mrt_status st = mrt_internal_camera_store(cam, const_cast<mrt_camera*>(s->S.camp), (char*)s->d_S + offsetof(DScene, cam), stream)) return st;
    s->S.cam = *cam;
    return MRT_OK;
}

extern "C" mrt_status mrt_render_debug(mrt_scene* s, float* path_rgb, uint32_t* path_rays, uint64_t n_paths) {
    MRT_GPU_ONLY(s, "mrt_render_debug");
    if (!s || !(s->ws.wdesc.flags & MRT_RF_PATH_DEBUG) || n_paths != s->last_paths)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_render_debug: no debug render of that size");
    HIPCHK(hipSetDevice(s->device));
    if (path_rgb) HIPCHK(hipMemcpy(path_rgb, s->ws.d_rad.p, n_paths * 12, hipMemcpyDeviceToHost));
    if (path_rays) HIPCHK(hipMemcpy(path_rays, s->ws.d_path_rays.p, n_paths * 4, hipMemcpyDeviceToHost));
    return MRT_OK;
}

// work_queue::getPercentDone (work_queue.cpp:142-175): paths handed out over all paths of the
// render, callable from another host thread while the render runs.  Needs no GPU work: a finished
// launch counts whole (its stop event), a running one by the snapshot of its work counter that
// the path kernel stores into host memory, a launch not yet started as 0.
extern "C" mrt_status mrt_progress(mrt_scene* s, float* pct) {
    if (!s || !pct) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_progress: null");
    *pct = 0.0f;
    if (s->cpu) return mrt_cpu_progress(s->cpu, pct);
    std::lock_guard<std::mutex> lk(s->prog.mu);
    const size_t n = s->prog.n_chunks.load(std::memory_order_acquire);
    if (n == 0 || !s->prog.h_prog || s->prog.h_prog_cap < s->prog.base + n || s->prog.ev.size() < 2 * n || s->prog.h_seen.size() < n * MRT_NPART) return MRT_OK;  // not started
    double done = 0, total = 0;
    for (size_t k = 0; k < n; k++) {
        total += (double)s->prog.chunk_paths[k];
        if (hipEventQuery(s->prog.ev[2 * k + 1]) == hipSuccess) {
            done += (double)s->prog.chunk_paths[k];
        } else if (hipEventQuery(s->prog.ev[2 * k]) == hipSuccess) {
            // one snapshot per work partition (the paths it has handed out); snapshots from
            // different waves land out of order: report the largest seen so far
            const uint64_t np = s->prog.chunk_paths[k];
            for (uint32_t j = 0; j < MRT_NPART; j++) {
                uint64_t c = __atomic_load_n(&s->prog.h_prog[(s->prog.base + k) * MRT_NPART + j], __ATOMIC_RELAXED);
                c = std::max(c, s->prog.h_seen[k * MRT_NPART + j]);
                s->prog.h_seen[k * MRT_NPART + j] = c;
                done += (double)std::min<uint64_t>(c, np * (j + 1) / MRT_NPART - np * j / MRT_NPART);
            }
        }
    }
    *pct = total > 0 ? (float)std::min(100.0, done * 100.0 / total) : 0.0f;
    return MRT_OK;
}

// The UI thread's view of G_linearBackBuffer (main.cpp:387-444) without stopping the render: the
// newest snapshot whose sequence word was even, and unchanged, around the copy out of pinned memory.
extern "C" mrt_status mrt_preview(mrt_scene* s, float* rgb_out, uint32_t* samples_done) {
    if (!s || !rgb_out || !samples_done) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_preview: null");
    *samples_done = 0;
    if (s->cpu) return mrt_cpu_preview(s->cpu, rgb_out, samples_done);
    std::lock_guard<std::mutex> lk(s->prog.mu);
    if (!s->prev.h_seq || !s->prev.h_prev || s->prev.px.empty()) return MRT_OK;  // no preview render yet
    std::vector<float4> snap(s->prev.px.size());
    for (int tries = 0; tries < 1000; tries++) {
        const uint32_t a = __atomic_load_n(s->prev.h_seq, __ATOMIC_ACQUIRE);
        if (a == 0) return MRT_OK;  // nothing folded yet
        if (a & 1u) {               // a copy is landing: the previous one is being overwritten
            usleep(50);
            continue;
        }
        const uint32_t n = __atomic_load_n(s->prev.h_seq + 1, __ATOMIC_ACQUIRE);
        memcpy(snap.data(), s->prev.h_prev, snap.size() * 16);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (__atomic_load_n(s->prev.h_seq, __ATOMIC_ACQUIRE) != a) continue;  // torn: retry
        for (size_t i = 0; i < snap.size(); i++) memcpy(rgb_out + (size_t)s->prev.px[i] * 4, &snap[i], 16);
        *samples_done = n;
        return MRT_OK;
    }
    return MRT_OK;  // the render outran every attempt: report nothing rather than a torn image
}

extern "C" mrt_status mrt_set_worker_seeds(mrt_scene* s, uint32_t n_threads, const uint64_t* initstate, const uint64_t* initseq) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_set_worker_seeds: null");
    if (!s->cpu)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_set_worker_seeds: the reference's per-thread RNG order is a CPU-backend mode "
                                                  "(the GPU keys its PCG streams per path)");
    return mrt_cpu_set_worker_seeds(s->cpu, n_threads, initstate, initseq);
}

extern "C" mrt_status mrt_kernel_ms(mrt_scene* s, float* path_ms, uint32_t* launches) {
    if (!s || !path_ms) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_kernel_ms: null");
    if (s->cpu) {  // wall time of the last CPU render
        if (launches) *launches = 1;
        return mrt_cpu_last_ms(s->cpu, path_ms, nullptr);
    }
    HIPCHK(hipSetDevice(s->device));
    float total = 0;
    for (uint32_t k = 0; k < s->prog.n_launch; k++) {
        HIPCHK(hipEventSynchronize(s->prog.ev[2 * k + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, s->prog.ev[2 * k], s->prog.ev[2 * k + 1]));
        total += ms;
    }
    *path_ms = total;
    if (launches) *launches = s->prog.n_launch;
    return MRT_OK;
}
