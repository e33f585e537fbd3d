// mrt_upload.hip -- a scene's way onto the device and off it: the choice of kernel variant, the table
// upload, the per-build launch sizing (PathLaunch), mrt_scene_free and mrt_scene_kernel_info.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mrt_context.h"
#include "mrt_tables.h"

using namespace mrtd;

// The tolerance contract's kernels: per variant the path-exact build (kPathExact), else the
// denormal-flushing build (kFtzVariant), else the plain fast build -- the variant's whole column
// (a build's workgroup shape, LDS fold levels and walk flags follow its own switches).
// MRT_PATH_EXACT=0 / MRT_FTZ=0 in the environment skip a build for every variant (A/B).
static void take_variant(KernelTable& m, const KernelTable& s, uint32_t i) {
    m.kernel[i] = s.kernel[i];
    m.lev_k[i] = s.lev_k[i];
    m.wg[i] = s.wg[i];
    m.tree[i] = s.tree[i];
    m.pq[i] = s.pq[i];
    m.box6_walk[i] = s.box6_walk[i];
    m.rewrite[i] = s.rewrite[i];
}
static const KernelTable& fast_table() {
    static const KernelTable t = [] {
        KernelTable m = kernel_table_fast();
        auto off = [](const char* name) {  // A/B hooks: MRT_FTZ=0, MRT_PATH_EXACT=0
            const char* e = getenv(name);
            return e && *e && atoi(e) == 0;
        };
        const KernelTable& z = kernel_table_fast_ftz();
        const KernelTable& x = kernel_table_fast_pex();
        for (uint32_t i = 0; i < kNumVariants; i++) {
            if (x.kernel[i] && !off("MRT_PATH_EXACT")) take_variant(m, x, i);
            else if (z.kernel[i] && !off("MRT_FTZ")) take_variant(m, z, i);
            // the exact arithmetic for the rounding-critical paths of the fast variants (mrt_retrace_kernel)
            m.retrace[i] = x.retrace[i];
        }
        return m;
    }();
    return t;
}

// first variant covering the scene's features: its own program shape first, then the interpreter
static uint32_t pick_variant(uint32_t features) {
    const uint32_t feat = features & 0xFFFFu, sig = MRT_SIG_OF(features);
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t i = 0; i < kNumVariants; i++) {
            const uint32_t vf = kVariants[i] & 0xFFFFu, vs = MRT_SIG_OF(kVariants[i]);
            if ((feat & ~vf) != 0 || (vf & FT_LIN) != (feat & FT_LIN)) continue;
            if (pass == 0 ? (vs == sig && sig != SIG_NONE) : vs == SIG_NONE) return i;
        }
    return kNumVariants - 1;
}

static mrt_status dev_alloc(mrt_scene* s, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return mrt_internal_fail(e == hipErrorOutOfMemory ? MRT_ERR_OOM : MRT_ERR_HIP, "hipMalloc failed");
    s->allocs.push_back(*p);
    return MRT_OK;
}
static mrt_status upload(mrt_scene* s, const void* src, size_t bytes, void** dst) {
    void* p = nullptr;
    mrt_status st = dev_alloc(s, &p, bytes);
    if (st) return st;
    if (bytes) {
        hipError_t e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return mrt_internal_fail(MRT_ERR_HIP, "hipMemcpy upload failed");
    }
    *dst = p;
    return MRT_OK;
}

extern "C" mrt_status mrt_init(int* device_count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        if (device_count) *device_count = 0;
        return mrt_internal_fail(MRT_ERR_NO_DEVICE, "no HIP device visible");
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, 0));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return mrt_internal_fail(MRT_ERR_NO_DEVICE, (std::string("device is ") + prop.gcnArchName + ", libmrt is built for gfx950").c_str());
    if (device_count) *device_count = n;
    return MRT_OK;
}

// the scene tables and the view's arrays to the device, the DScene that points at them, the scratch
static mrt_status upload_tables(mrt_scene* s, const mrt_scene_view* v, const SceneTables& T) {
    mrt_status st;
    DScene& S = s->S;
#define UP(src, n, dst) { void* t_ = nullptr; if ((st = upload(s, src, (size_t)(n) * sizeof(*(src)), &t_))) return st; *(dst) = (decltype(+*(dst)))t_; }
    UP(T.nodes.data(), T.nodes.size(), &S.nodes);
    UP(v->children, v->n_children, &S.children);
    UP(v->mesh_nodes, v->n_mesh_nodes, &S.mnodes);
    UP(T.wide.data(), T.wide.size(), &S.mwide);
    S.mwide_n = (uint32_t)T.wide.size();
    UP(T.bwide.data(), T.bwide.size(), &S.bwide);
    UP(T.bprims.data(), T.bprims.size(), &S.bprims);
    UP((const float4*)v->tri_geo, (size_t)v->n_tris * 3, &S.tri_geo);
    UP((const float4*)v->tri_nrm, (size_t)v->n_tris * 3, &S.tri_nrm);
    UP(T.dmats.data(), T.dmats.size(), &S.mats);
    UP(T.bleaf.data(), T.bleaf.size(), &S.bleaf);
    S.nbleaf = T.nbleaf;
    S.nbleaf_f = (float)T.nbleaf;
    S.inv_nbleaf = 1.0f / S.nbleaf_f;
    S.blist = T.blist;
    S.blazy = T.blazy;
    S.light_once = T.light_once;
    UP(v->textures, v->n_textures, &S.texs);
    UP((const float4*)v->perlin_ranvec, 256, &S.ranvec);
    UP(v->perlin_perm, 768, &S.perm);
    UP(v->texels, (size_t)v->n_texels, &S.texels);
    if (T.cornell_hits.empty()) {
        UP(T.prog.data(), T.prog.size(), &S.prog);
    } else {  // Cornell shape: the hit table behind the END op, one op's size per entry (mrt_sig.h)
        std::vector<LinOp> pw(T.prog);
        pw.resize(T.prog.size() + kHitCount);
        memcpy(pw.data() + T.prog.size(), T.cornell_hits.data(), (size_t)kHitCount * kHitWords * 4);
        UP(pw.data(), pw.size(), &S.prog);
    }
    {
        const char* e = getenv("MRT_NO_REWRITE");  // A/B hook: the interpreter on the program as compiled
        if (!T.prog_fast.empty() && !(e && *e && *e != '0')) UP(T.prog_fast.data(), T.prog_fast.size(), &s->prog_fast);
    }
    UP(&v->camera, 1, &S.camp);
#undef UP
    S.root = v->root;
    S.biased = v->biased;
    S.sky = v->sky;
    S.cam = v->camera;
    s->n_nodes = v->n_nodes;
    s->prog_ops = T.prog_ops;
    void* p;
    if ((st = upload(s, &s->S, sizeof(DScene), &p))) return st;
    s->d_S = (DScene*)p;
    if ((st = dev_alloc(s, &p, sizeof(RenderScratch)))) return st;
    s->d_scratch = (RenderScratch*)p;
    HIPCHK(hipMemset(p, 0, sizeof(RenderScratch)));  // the cancel flag starts clear
    return MRT_OK;
}

// The launch of each numerics build of the scene's kernel variant (s->pl): LDS stacks, grid, side slots.
static mrt_status size_launches(mrt_scene* s, const SceneTables& T, const hipDeviceProp_t& prop) {
    // kernel variant + LDS stacks sized from the scene graph (top frame lives in registers)
    s->features = T.features;
    s->variant = pick_variant(s->features);
    const bool lin_kernel = (kVariants[s->variant] & FT_LIN) != 0;
    s->lds_frames = lin_kernel ? 0 : (uint32_t)std::max(T.max_frames - 1, 0);
    s->lds_rays = lin_kernel ? 0 : (uint32_t)T.max_rays;
    s->lds_mesh = (uint32_t)T.max_mesh;
    // the query ray parked in LDS: instances (scene_hit_lin)
    s->lds_save = (lin_kernel && (kVariants[s->variant] & FT_INST)) ? 9u : 0u;  // (round 6: 15 -> 9, mrt_lin.h inst_ray)
    // resumable mesh walk: deeper pod_bvh trees keep the wave walking longer
    s->walk_min = T.wide.size() >= 2048 ? 40u : 32u;  // inner nodes: bunny 2937, teapot ~1045
    bool walk_min_env = false;
    if (const char* e = getenv("MRT_WALK_MIN"))  // sweep hook (tools/ab_walk.sh)
        if (*e) {
            s->walk_min = (uint32_t)atoi(e);
            walk_min_env = true;
        }
    s->n_cu = (uint32_t)prop.multiProcessorCount;
    // resident workgroups per CU: one 256-thread group = one wave per SIMD (a 64-thread group =
    // a quarter of that); VGPRs (512 per SIMD lane, granule 8) and LDS (160 KiB per CU) bound it.
    // (The runtime occupancy query under-counts gfx950 register budgets, so it is computed from
    // the kernel's attributes.)  Per numerics build: their register counts differ.
    const KernelTable* tabs[2] = {&kernel_table_exact(), &fast_table()};
    for (int k = 0; k < 2; k++) {
        PathLaunch& L = s->pl[k];
        L.fn = tabs[k]->kernel[s->variant];
        L.wg = tabs[k]->wg[s->variant];
        const uint32_t waves_per_wg = L.wg / 64u;
        // the Cornell walk of the tolerance contract (mrt_sig.h cornell_fast_hit) parks no ray
        L.lds_save = tabs[k]->box6_walk[s->variant] ? 0u : s->lds_save;
        L.rewrite = tabs[k]->rewrite[s->variant] != 0;
        L.retrace = tabs[k]->retrace[s->variant];
        // a fast-arithmetic kernel hands its rounding-critical paths to the exact arithmetic
        // (mrt_shade.h light_critical); MRT_RETRACE=0 at upload keeps them (A/B)
        {
            const char* e = getenv("MRT_RETRACE");
            L.handover = k == 1 && L.retrace && L.fn != kernel_table_fast_pex().kernel[s->variant] && !(e && *e && atoi(e) == 0);
        }
        // the path-exact build (the metal bunny under the tolerance contract) yields at 32 walking
        // lanes: 40 -1.2%, 28 -1.7%, 48 -10% (bunny 1024x1024x64, profiles/r04_ab.txt section 13)
        L.walk_min = (!walk_min_env && L.fn == kernel_table_fast_pex().kernel[s->variant]) ? 32u : s->walk_min;
        hipFuncAttributes fa{};
        HIPCHK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(L.fn)));
        const int vg = std::max(8, (fa.numRegs + 7) & ~7);
        const int nb_vgpr = std::max(1, std::min(8, 512 / vg) * 4 / (int)waves_per_wg);  // waves per CU / waves per group
        auto groups = [&](size_t lds) { return std::max(1, lds ? std::min<int>(nb_vgpr, (int)((160u * 1024u) / lds)) : nb_vgpr); };
        // the group's LDS as the kernel indexes it (mrt_launch.h WaveLds): the stacks, the variant's fold
        // levels and queue of path starts, each wave's copy of the Cornell hit table (mrt_sig.h;
        // T.cornell_hits, uploaded behind the program)
        WaveLds lds = walk_lds(s, L.lds_save);
        lds.lev_k = tabs[k]->lev_k[s->variant];
        lds.pq = tabs[k]->pq[s->variant];
        lds.box6 = tabs[k]->box6_walk[s->variant] != 0;
        lds.waves = waves_per_wg;
        if (lds.box6 && T.cornell_hits.empty()) return mrt_internal_fail(MRT_ERR_INVALID, "Cornell walk without a hit table");
        if (lds.bytes() > (size_t)prop.sharedMemPerBlock) return mrt_internal_fail(MRT_ERR_INVALID, "scene graph too deep for the LDS stacks");
        int nb = groups(lds.bytes());
        if (tabs[k]->tree[s->variant]) {
            // the LDS the resident groups leave free, split among them: the treelet of each group
            const size_t per = std::min<size_t>((160u * 1024u) / nb, (size_t)prop.sharedMemPerBlock);
            const uint32_t node_bytes = WaveLds::kNodeWords * 4u;  // BvhWide
            const uint32_t n_nodes = (uint32_t)T.bwide.size();
            uint32_t cap = per > lds.bytes() ? (uint32_t)((per - lds.bytes()) / node_bytes) : 0u;
#ifdef MRT_EXPERIMENTS
            if (const char* e = getenv("MRT_TREELET_NODES"))  // sweep hook
                if (*e) cap = std::min<uint32_t>(cap, (uint32_t)atoi(e));
#endif
            lds.tree_n = L.tree_n = std::min(cap, n_nodes);
        }
        L.lds_bytes = lds.bytes();
        L.vgprs = (uint32_t)fa.numRegs;
#ifdef MRT_EXPERIMENTS
        if (const char* e = getenv("MRT_BLOCKS_PER_CU"))  // experiment hook
            if (*e) nb = std::max(1, atoi(e));
#endif
        L.grid = prop.multiProcessorCount * nb;
        // every work partition needs waves of its own: a wave leaves its partition only once it is
        // handed out, and visits at most MRT_STEAL_TRIES partitions (mrt_kernels.hip)
        if (L.grid < (int)MRT_NPART) return mrt_internal_fail(MRT_ERR_HIP, "path kernel grid smaller than the work partitions");
        s->max_threads = std::max(s->max_threads, (size_t)L.grid * L.wg);
        // the slots of an async launch's side kernels (kSideSlots): the Cornell walk kernel at eight
        // one-wave groups per SIMD, the register-bound grid
        const int wps = std::min(8, 512 / vg);
        if (tabs[k]->box6_walk[s->variant] && L.wg == 64u && nb == wps * 4 && wps == 8)
            L.side = std::min(kSideSlots, L.grid / 2) / (int)MRT_NPART * (int)MRT_NPART;
        if (L.side && L.retrace) {  // a retrace that does not fit a freed slot stays on the render's stream
            hipFuncAttributes ra{};
            HIPCHK(hipFuncGetAttributes(&ra, reinterpret_cast<const void*>(L.retrace)));
            L.retrace_side = ra.numRegs <= kSideVgprs;
        }
    }
    return MRT_OK;
}

extern "C" mrt_status mrt_scene_upload(int device, const mrt_scene_view* v, mrt_scene** out) {
    if (!out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_upload: null");
    if (device == MRT_DEVICE_CPU) {  // the CPU backend (explicit choice only)
        mrt_cpu_scene* c = nullptr;
        mrt_status st = mrt_cpu_scene_create(v, &c);
        if (st) return st;
        mrt_scene* s = new mrt_scene();
        s->device = MRT_DEVICE_CPU;
        s->cpu = c;
        s->n_nodes = v->n_nodes;
        s->features = mrt_cpu_scene_features(c);
        *out = s;
        return MRT_OK;
    }
    if (device < 0) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_upload: bad device");
    SceneTables T;
    mrt_status st = mrt_internal_scene_tables(v, &T);
    if (st) return st;
    HIPCHK(hipSetDevice(device));
    // owned until *out takes it: every early return below frees the scene and what it has uploaded
    std::unique_ptr<mrt_scene, decltype(&mrt_scene_free)> owner(new mrt_scene(), mrt_scene_free);
    mrt_scene* const s = owner.get();
    s->device = device;
    if ((st = upload_tables(s, v, T))) return st;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if ((st = size_launches(s, T, prop))) return st;
    *out = owner.release();
    return MRT_OK;
}

extern "C" void mrt_scene_free(mrt_scene* s) {
    if (!s) return;
    if (s->cpu) {
        mrt_cpu_scene_free(s->cpu);
        delete s;
        return;
    }
    (void)hipSetDevice(s->device);
    if (s->ev_done_pending) (void)hipEventSynchronize(s->ev_done);
    for (void* p : s->allocs) (void)hipFree(p);
    for (hipEvent_t e : s->prog.ev) (void)hipEventDestroy(e);
    if (s->prog.pstream) (void)hipStreamDestroy(s->prog.pstream);
    if (s->prog.h_prog) (void)hipHostFree(s->prog.h_prog);
    if (s->prog.h_one) (void)hipHostFree(s->prog.h_one);
    if (s->prev.h_prev) (void)hipHostFree(s->prev.h_prev);
    if (s->prev.h_seq) (void)hipHostFree(s->prev.h_seq);
    if (s->ev_done) (void)hipEventDestroy(s->ev_done);
    if (s->ev_aux_pending) (void)hipEventSynchronize(s->ev_aux);
    if (s->ev_aux) (void)hipEventDestroy(s->ev_aux);
    if (s->fold.fstream) (void)hipStreamDestroy(s->fold.fstream);
    if (s->query.cast_stream) (void)hipStreamDestroy(s->query.cast_stream);
    if (s->query.trace_stream) (void)hipStreamDestroy(s->query.trace_stream);
    for (hipEvent_t e : {s->fold.ev_kern, s->fold.ev_fold[0], s->fold.ev_fold[1]})
        if (e) (void)hipEventDestroy(e);
    delete s;  // (the workspace and staging buffers release themselves: DevBuf)
}

extern "C" mrt_status mrt_scene_kernel_info(const mrt_scene* s, mrt_kernel_info* out) {
    if (!s || !out) return mrt_internal_fail(MRT_ERR_INVALID, "mrt_scene_kernel_info: null");
    out->features = s->features;
    if (s->cpu) {  // the host instantiation that runs it (mrt_cpu.hip), threads of the last render
        float ms;
        uint32_t threads = 0;
        mrt_cpu_last_ms(s->cpu, &ms, &threads);
        *out = mrt_kernel_info{};
        out->features = s->features;
        out->kernel_features = (s->features & FT_LIN) ? (FT_LIN | FT_ALL) : FT_ALL;
        out->grid = threads;
        return MRT_OK;
    }
    out->kernel_features = kVariants[s->variant];
    const PathLaunch& L = s->pl[s->last_numerics];
    out->lds_bytes = (uint32_t)L.lds_bytes;
    out->grid = s->last_grid ? s->last_grid : (uint32_t)L.grid;  // (an async launch with side slots: fewer groups)
    out->prog_ops = s->prog_ops;
    out->vgprs = L.vgprs;
    out->wg = L.wg;
    out->tree_nodes = L.tree_n;  // BvhWide nodes per workgroup
    out->build = s->last_numerics == 0 ? MRT_BUILD_EXACT
               : L.fn == kernel_table_fast_pex().kernel[s->variant] ? MRT_BUILD_PATH_EXACT
               : L.fn == kernel_table_fast_ftz().kernel[s->variant] ? MRT_BUILD_FAST_FTZ
                                                                     : MRT_BUILD_FAST;
    out->n_cu = s->n_cu;
    out->handed_over = 0;
    out->handover_lost = 0;
    if (s->d_scratch) {
        // after the scene's last render, its fold included: ev_done is recorded on the render's
        // stream (or the context's fold stream), which the legacy null stream of a plain hipMemcpy
        // is not ordered after
        HIPCHK(hipSetDevice(s->device));
        if (s->ev_done_pending) HIPCHK(hipEventSynchronize(s->ev_done));
        RenderScratch n{};
        if (hipMemcpy(&n, s->d_scratch, sizeof n, hipMemcpyDeviceToHost) != hipSuccess)
            return mrt_internal_fail(MRT_ERR_HIP, "mrt_scene_kernel_info: counter read");
        out->handed_over = n.handed_over;
        out->handover_lost = n.lost;
    }
    return MRT_OK;
}
