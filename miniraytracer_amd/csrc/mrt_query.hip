// mrt_query.hip -- the entry points that read a scene without rendering it: the first-hit feature
// buffers (mrt_render_aux*), the ray queries (mrt_cast_rays*) and the radiance queries (mrt_trace_rays*).
// Their kernels live in mrt_aux.hip, mrt_cast.hip and mrt_probe.hip; this unit launches them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mrt_context.h"
#include "mrt_aux.h"
#include "mrt_cast.h"
#include "mrt_probe.h"

using namespace mrtd;

// ---- first-hit feature buffers (include/mrt.h "feature buffers and denoise") ----
// what both entry points read of the desc; flags: 0 or MRT_RF_FAST (ignored: the buffers come from
// the exact arithmetic's hit code on both backends)
static mrt_status aux_check(const char* who, const mrt_scene* s, const mrt_render_desc* d, const void* normal, const void* albedo) {
    if (!s || !d || !normal || !albedo) return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": null").c_str());
    if (d->width == 0 || d->height == 0 || d->sqrt_samples == 0 || (d->world && d->rank >= d->world))
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": bad desc").c_str());
    if (d->flags & ~MRT_RF_FAST)
        return mrt_internal_fail(MRT_ERR_INVALID, (std::string(who) + ": flags other than MRT_RF_FAST").c_str());
    return mrt_internal_check_pixels(d);
}

extern "C" mrt_status mrt_render_aux_device(mrt_scene* s, const mrt_render_desc* d, float* d_normal, float* d_albedo, void* stream) {
    MRT_GPU_ONLY(s, "mrt_render_aux_device");
    mrt_status st = aux_check("mrt_render_aux_device", s, d, d_normal, d_albedo);
    if (st) return st;
    // the pixel table and the sample grid are the render's (mrt_prepare); nothing else of the
    // workspace is used, and no flag of the render path applies
    mrt_render_desc dc = *d;
    dc.flags = 0;
    if ((st = mrt_prepare(s, &dc))) return st;
    if (s->ws.npix == 0) return MRT_OK;
    const aux_kernel_t fn = aux_kernel_table().kernel[s->variant];
    const PathLaunch& PL = s->pl[0];  // the exact build's stack sizes
    const PathParams P = launch_params(s, PL, d);
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipStream_t q = (hipStream_t)stream;
    hipLaunchKernelGGL(fn, dim3((s->ws.npix + 63u) / 64u), dim3(64), lds_bytes, q, P, (float4*)d_normal, (float4*)d_albedo);
    HIPCHK(hipGetLastError());
    // a later change of the pixel table or the sample grid waits for this kernel (quiesce); not
    // while `stream` is being captured: nothing runs now, and a captured event cannot be waited for
    // on the host (the caller keeps the layout while it replays the graph)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (q) HIPCHK(hipStreamIsCapturing(q, &cap));
    if (cap == hipStreamCaptureStatusNone) {
        HIPCHK(hipEventRecord(s->ev_aux, q));
        s->ev_aux_pending = true;
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_render_aux(mrt_scene* s, const mrt_render_desc* d, float* normal_out, float* albedo_out) {
    mrt_status st = aux_check("mrt_render_aux", s, d, normal_out, albedo_out);
    if (st) return st;
    if (s->cpu) return mrt_cpu_render_aux(s->cpu, d, normal_out, albedo_out);
    mrt_render_desc dc = *d;
    dc.flags = 0;
    if ((st = mrt_prepare(s, &dc))) return st;
    const std::vector<uint32_t> px = mrt_internal_local_pixels(d);
    if (px.empty()) return MRT_OK;
    float* dev = nullptr;  // normal, then albedo: n_local float4 each
    if (hipMalloc((void**)&dev, px.size() * 32) != hipSuccess) return mrt_internal_fail(MRT_ERR_OOM, "mrt_render_aux: device buffers");
    std::vector<float> local(px.size() * 8);
    st = mrt_render_aux_device(s, d, dev, dev + px.size() * 4, nullptr);
    hipError_t e = hipSuccess;
    if (!st) e = hipMemcpy(local.data(), dev, local.size() * 4, hipMemcpyDeviceToHost);  // (waits for the kernel)
    (void)hipFree(dev);
    if (st) return st;
    if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_HIP, hipGetErrorString(e));
    s->ev_aux_pending = false;
    for (size_t i = 0; i < px.size(); i++) {
        memcpy(normal_out + (size_t)px[i] * 4, &local[i * 4], 16);
        memcpy(albedo_out + (size_t)px[i] * 4, &local[(px.size() + i) * 4], 16);
    }
    return MRT_OK;
}

// ---- ray queries (include/mrt.h "ray queries") ----
// One mrt_cast_kernel launch over device records: the scene's variant from the cast table, one-wave
// groups with the exact build's walk stacks (the aux launch's).  It reads the scene tables and the
// rays and writes the hits; nothing of the render workspace, so it needs no mrt_prepare, takes no
// part in quiesce() and leaves no event behind.
static mrt_status cast_launch(mrt_scene* s, const mrt_ray* d_rays, uint32_t n, uint64_t seed, mrt_hit* d_hits, hipStream_t q) {
    CastParams P{};
    P.sc = s->S;
    P.rays = (const CastRay*)d_rays;
    P.hits = (CastHit*)d_hits;
    P.seed = seed;
    P.n = n;
    set_walk_lds(P, s, s->pl[0].lds_save);
    const cast_kernel_t fn = cast_kernel_table().kernel[s->variant];
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipLaunchKernelGGL(fn, dim3((uint32_t)(((uint64_t)n + 63u) / 64u)), dim3(64), lds_bytes, q, P);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

extern "C" mrt_status mrt_cast_rays_device(mrt_scene* s, const mrt_ray* d_rays, uint32_t n, uint64_t seed, mrt_hit* d_hits, void* stream) {
    MRT_GPU_ONLY(s, "mrt_cast_rays_device");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: null");
    if (n == 0) return MRT_OK;
    if (!d_rays || !d_hits) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: null");
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays_device: records not 16-byte aligned");
    HIPCHK(hipSetDevice(s->device));
    return cast_launch(s, d_rays, n, seed, d_hits, (hipStream_t)stream);
}

extern "C" mrt_status mrt_cast_rays(mrt_scene* s, const mrt_ray* rays, uint32_t n, uint64_t seed, mrt_hit* hits) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays: null");
    if (n == 0) return MRT_OK;
    if (!rays || !hits) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_cast_rays: null");
    if (s->cpu) return mrt_cpu_cast_rays(s->cpu, rays, n, seed, hits);
    HIPCHK(hipSetDevice(s->device));
    // staged in pieces of at most 2^20 rays (80 MiB of device records); piece k0 casts with seed + k0
    const uint32_t piece = std::min(n, 1u << 20);
    QueryStaging& Q = s->query;
    if (!Q.cast_stream) HIPCHK(hipStreamCreateWithFlags(&Q.cast_stream, hipStreamNonBlocking));
    if (mrt_status st = Q.d_cast.grow_own((size_t)piece * (sizeof(mrt_ray) + sizeof(mrt_hit)), "mrt_cast_rays: device records")) return st;
    mrt_ray* const d_rays = (mrt_ray*)Q.d_cast.p;
    mrt_hit* const d_hits = (mrt_hit*)(Q.d_cast.p + (size_t)piece * sizeof(mrt_ray));  // (48 * piece: 16-byte aligned)
    for (uint64_t k0 = 0; k0 < n; k0 += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - k0);
        HIPCHK(hipMemcpyAsync(d_rays, rays + k0, (size_t)m * sizeof(mrt_ray), hipMemcpyHostToDevice, Q.cast_stream));
        if (mrt_status st = cast_launch(s, d_rays, m, seed + k0, d_hits, Q.cast_stream)) return st;
        HIPCHK(hipMemcpyAsync(hits + k0, d_hits, (size_t)m * sizeof(mrt_hit), hipMemcpyDeviceToHost, Q.cast_stream));
        HIPCHK(hipStreamSynchronize(Q.cast_stream));
    }
    return MRT_OK;
}

// ---- radiance queries (include/mrt.h "radiance queries") ----
// The probe kernel's full grid in waves: kProbeWavesPerCU per CU of the scene's device, whatever the
// variant; a wave's level rows are 64 lanes x max(max_bounces, 1) float4.
static uint64_t probe_full_waves(const mrt_scene* s) { return (uint64_t)s->n_cu * kProbeWavesPerCU; }
static uint64_t probe_wave_bytes(uint32_t max_bounces) { return 64ull * std::max<uint32_t>(max_bounces, 1u) * 16ull; }

// One mrt_probe_kernel launch over device records: the scene's variant from the probe table, one-wave
// groups with the exact build's walk stacks (the cast launch's), `waves` of them, each lane striding
// over the records.  It reads the scene tables and the probes and writes the records and the level
// rows of its own lanes; nothing of the render workspace, so it needs no mrt_prepare, takes no part in
// quiesce() and leaves no event behind.
static mrt_status probe_launch(mrt_scene* s, const mrt_probe* d_probes, uint32_t n, uint32_t max_bounces, mrt_radiance* d_out, void* d_work,
                               uint32_t waves, hipStream_t q) {
    ProbeParams P{};
    P.sc = s->S;
    P.probes = (const ProbeRec*)d_probes;
    P.out = (ProbeOut*)d_out;
    P.lev = (float4*)d_work;
    P.n = n;
    P.max_bounces = max_bounces;
    P.lev_rows = std::max<uint32_t>(max_bounces, 1u);
    set_walk_lds(P, s, s->pl[0].lds_save);
    const probe_kernel_t fn = probe_kernel_table().kernel[s->variant];
    const size_t lds_bytes = walk_lds(s, P.lds_save).bytes();
    hipLaunchKernelGGL(fn, dim3(waves), dim3(64), lds_bytes, q, P);
    HIPCHK(hipGetLastError());
    return MRT_OK;
}

// the waves a launch over n records runs with `work_bytes` of level rows (0: fewer than one wave's)
static uint32_t probe_waves(const mrt_scene* s, uint32_t n, uint32_t max_bounces, uint64_t work_bytes) {
    const uint64_t have = work_bytes / probe_wave_bytes(max_bounces);
    return (uint32_t)std::min({have, probe_full_waves(s), ((uint64_t)n + 63u) / 64u});
}

extern "C" mrt_status mrt_trace_rays_workspace(const mrt_scene* s, uint32_t max_bounces, uint64_t* bytes_full, uint64_t* bytes_min) {
    MRT_GPU_ONLY(s, "mrt_trace_rays_workspace");
    if (!s || !bytes_full || !bytes_min) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_workspace: null");
    *bytes_min = probe_wave_bytes(max_bounces);
    *bytes_full = probe_full_waves(s) * probe_wave_bytes(max_bounces);
    return MRT_OK;
}

extern "C" mrt_status mrt_trace_rays_device(mrt_scene* s, const mrt_probe* d_probes, uint32_t n, uint32_t max_bounces, mrt_radiance* d_out,
                                            void* d_work, uint64_t work_bytes, void* stream) {
    MRT_GPU_ONLY(s, "mrt_trace_rays_device");
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: null");
    if (n == 0) return MRT_OK;
    if (!d_probes || !d_out || !d_work) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: null");
    if (((uintptr_t)d_probes | (uintptr_t)d_out | (uintptr_t)d_work) & 15u)
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: records or workspace not 16-byte aligned");
    if (work_bytes < probe_wave_bytes(max_bounces))
        return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays_device: workspace below one wave's level rows (mrt_trace_rays_workspace)");
    HIPCHK(hipSetDevice(s->device));
    return probe_launch(s, d_probes, n, max_bounces, d_out, d_work, probe_waves(s, n, max_bounces, work_bytes), (hipStream_t)stream);
}

extern "C" mrt_status mrt_trace_rays(mrt_scene* s, const mrt_probe* probes, uint32_t n, uint32_t max_bounces, mrt_radiance* out,
                                     uint64_t* rays_out) {
    if (!s) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays: null");
    if (n == 0) {
        if (rays_out) *rays_out = 0;
        return MRT_OK;
    }
    if (!probes || !out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_trace_rays: null");
    if (s->cpu) {
        if (mrt_status st = mrt_cpu_trace_rays(s->cpu, probes, n, max_bounces, out)) return st;
    } else {
        HIPCHK(hipSetDevice(s->device));
        // staged in pieces of at most MRT_TRACE_PIECE records (64 MiB of device records); the level rows
        // of the waves a piece can occupy, at most the full grid's
        uint32_t piece_max = MRT_TRACE_PIECE;
        if (const char* e = getenv("MRT_TRACE_PIECE_RECORDS"))  // test hook: a small piece (tests/test_probe_gpu.py)
            if (*e) piece_max = std::max(1u, std::min((uint32_t)strtoul(e, nullptr, 0), MRT_TRACE_PIECE));
        const uint32_t piece = std::min(n, piece_max);
        QueryStaging& Q = s->query;
        if (!Q.trace_stream) HIPCHK(hipStreamCreateWithFlags(&Q.trace_stream, hipStreamNonBlocking));
        if (mrt_status st = Q.d_trace.grow_own((size_t)piece * (sizeof(mrt_probe) + sizeof(mrt_radiance)), "mrt_trace_rays: device records")) return st;
        const uint64_t waves = std::min<uint64_t>(probe_full_waves(s), ((uint64_t)piece + 63u) / 64u);
        const uint64_t work_bytes = waves * probe_wave_bytes(max_bounces);
        if (mrt_status st = Q.d_trace_work.grow_own((size_t)work_bytes, "mrt_trace_rays: level workspace")) return st;
        mrt_probe* const d_probes = (mrt_probe*)Q.d_trace.p;
        mrt_radiance* const d_out = (mrt_radiance*)(Q.d_trace.p + (size_t)piece * sizeof(mrt_probe));  // (48 * piece: 16-byte aligned)
        for (uint64_t k0 = 0; k0 < n; k0 += piece) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - k0);
            HIPCHK(hipMemcpyAsync(d_probes, probes + k0, (size_t)m * sizeof(mrt_probe), hipMemcpyHostToDevice, Q.trace_stream));
            if (mrt_status st = probe_launch(s, d_probes, m, max_bounces, d_out, Q.d_trace_work.p, probe_waves(s, m, max_bounces, work_bytes), Q.trace_stream))
                return st;
            HIPCHK(hipMemcpyAsync(out + k0, d_out, (size_t)m * sizeof(mrt_radiance), hipMemcpyDeviceToHost, Q.trace_stream));
            HIPCHK(hipStreamSynchronize(Q.trace_stream));
        }
    }
    if (rays_out) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; i++) total += out[i].rays;
        *rays_out = total;
    }
    return MRT_OK;
}
