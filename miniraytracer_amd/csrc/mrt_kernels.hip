// mrt_kernels.hip -- the path kernel (DESIGN.md "Kernels"), built three times from this one source:
//   build/obj/mrt_kernels_exact.o  MRT_FAST=0, -ffp-contract=off: the exact numerics contract,
//                                  bit-for-bit the reference built exact (tests/golden/stream_*.npz)
//   build/obj/mrt_kernels_fast.o   MRT_FAST=1, FMA contraction + reciprocal division + hardware
//                                  rcp/sqrt/rsq + f32 transcendentals: the tolerance contract
//                                  (per-pixel RMSE < 1e-3 vs the reference as shipped)
//   build/obj/mrt_kernels_fastz.o  the tolerance contract with f32 denormals flushed, for the
//                                  variants mrt_launch.h's kFtzVariant selects
// Each build exports its KernelTable (mrt_launch.h); the host picks one per render
// (mrt_render_desc.flags & MRT_RF_FAST), the fast one merged with the FTZ build's variants.
//
// mrt_path_kernel: persistent waves pull 256-path batches (64 near the end of a launch) from
// per-XCD partition counters (one atomic per wave per batch, like work_queue::getWork pulls a tile,
// work_queue.cpp:158-166) and run trace() for each lane's path to completion; per-path radiance
// is written sample-major [s][local pixel] (coalesced).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include <utility>

#include "mrt_launch.h"

using namespace mrtd;

// which table this build provides (experiments may build the "fast" slot with other switches)
#ifndef MRT_TABLE_FAST
#define MRT_TABLE_FAST MRT_FAST
#endif
// the third build: the tolerance contract with f32 denormals flushed (-fgpu-flush-denormals-to-zero),
// for the variants kFtzVariant selects (mrt_launch.h)
#ifndef MRT_TABLE_FTZ
#define MRT_TABLE_FTZ 0
#endif
// the fourth: exact arithmetic + forward fold, the tolerance contract's kPathExact variants
#ifndef MRT_TABLE_PEX
#define MRT_TABLE_PEX 0
#endif
#if MRT_TABLE_PEX
#define MRT_PATH_KERNEL mrt_path_kernel_pex
#elif MRT_TABLE_FTZ
#define MRT_PATH_KERNEL mrt_path_kernel_fastz
#elif MRT_TABLE_FAST
#define MRT_PATH_KERNEL mrt_path_kernel_fast
#else
#define MRT_PATH_KERNEL mrt_path_kernel
#endif


// Persistent waves with per-lane path regeneration: every loop iteration advances each busy lane
// by one segment (one trace() call); a lane whose path ended takes the next path index from its
// wave's pool at once (ballot + mbcnt compaction), and a wave refills its pool 64 paths at a time
// with one atomic (work_queue::getWork, work_queue.cpp:158-166).  Lanes stay busy until the pool
// runs dry instead of idling until the longest path of a 64-path batch finishes.
// Waves per SIMD the register allocator must reach (caps VGPRs at 512/W): the path loop is
// latency-bound, so a few spilled registers cost less than the lost occupancy.  Tuned per
// variant on MI355X (DESIGN.md "Occupancy").
// (compact variants -- Cornell, Cornell room + mesh, plain interpreter -- reach 80 VGPRs without
// spills at 6; built without SLP vectorisation (Makefile), the wide-feature variants run best at
// 6 waves (80 VGPRs; round 4, with MRT_TREE_WG 768: 4 waves before) and the room + mesh variant
// at 7 (72 VGPRs, no LDS fold levels))
#ifndef MRT_WPE_WIDE
#define MRT_WPE_WIDE (MRT_FAST ? 6 : 4)
#endif
#ifndef MRT_WPE_LIN
// forward fold: no LDS levels; 8 since the Cornell walk stores a path's radiance where it ends: 64 VGPRs,
// and the 80 scalar registers a wave may hold for eight to fit a SIMD (7 before, 68 VGPRs; without the
// attribute the kernel allocates 94 scalar registers, which run as seven waves on a grid sized for eight)
#define MRT_WPE_LIN (MRT_FWD_FOLD ? 8 : 6)
#endif
#ifndef MRT_WPE_MESH
#define MRT_WPE_MESH 7
#endif
// the room + mesh walk of the tolerance contract, fast arithmetic (C3) and path-exact (C4): 8 waves
// (fast: 62 VGPRs, no VGPR spill; path-exact: 64, 9 spilled).  Round 5 against 7: teapot 17.01 vs
// 17.51 ms per step, bunny 40.60 vs 41.07 (profiles/r05_ab.txt sections 22-23)
#ifndef MRT_WPE_ROOM_MESH
#define MRT_WPE_ROOM_MESH ((MRT_FAST || MRT_TABLE_PEX) ? 8 : MRT_WPE_MESH)
#endif
#ifndef MRT_WPE_LIN_GEN
// the interpreter's compact variants (no program shape): 6 waves (80 VGPRs, spill-free).  Round 4
// held them at 5 (96 VGPRs): the room op's per-lane axis select had become a lookup table in
// scratch, which kept the query ray in scratch memory; with sel3 it is gone, 81 VGPRs at 5 waves
// (C2 through the interpreter 43.3 -> 46.4 Grays/s), 80 at 6 (47.7), 72 + 5 spilled at 7 (44.1;
// profiles/r05_ab.txt section 6)
// The exact contract's interpreter kernels keep 5 (96 VGPRs): at 6 the exact arithmetic spilled 39
// VGPRs (C2 through the interpreter, exact: 45.2 ms per step at 6, 40.3 at 5, 43.5 at 4 waves,
// round 6, profiles/r06_ab.txt section 4)
#define MRT_WPE_LIN_GEN (MRT_FAST || MRT_TABLE_PEX ? 6 : 5)
#endif
template <uint32_t F> struct PathOcc {
    static constexpr bool kWide = (F & (FT_BVHW | FT_TEX | FT_VOLUME)) != 0 || !(F & FT_LIN);
    static constexpr int W = kWide ? (!(F & FT_LIN) ? 4 : MRT_WPE_WIDE)
                             : ((F & FT_MESH) != 0 ? (MRT_SIG_OF(F) == SIG_ROOM_MESH ? MRT_WPE_ROOM_MESH : MRT_WPE_MESH)
                                                   : (MRT_SIG_OF(F) != SIG_NONE ? MRT_WPE_LIN : MRT_WPE_LIN_GEN));
};
#if defined(MRT_EXPERIMENTS) && defined(MRT_PHASES)  // build ONE of the two TUs with it
__device__ unsigned long long g_phases[12];
extern "C" int mrt_debug_phases(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phases), sizeof(g_phases)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phases), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif
// Launch end.  A wave whose partition is handed out takes work from ONE other partition (chosen
// per wave group in four directions, MRT_STEAL_SPREAD), in small claims, then ends.  Visiting all
// eight (the round-2 rule) cost every wave 8 failing atomics at the launch's end, on 8 addresses
// hit by all 7168 waves at once: 3.5-4 us each against 0.6 us for a claim mid-launch (wave
// timelines, tools/wtimes.py), while the wave's in-flight lanes waited -- a fixed ~40 us per launch,
// 4% of an 8-rank share.  Every partition is still finished by its own waves.
#ifndef MRT_STEAL_SMALL
#define MRT_STEAL_SMALL 1
#endif
#ifndef MRT_STEAL_TRIES
#define MRT_STEAL_TRIES 2u  // partitions a wave takes work from (its own first) before it ends
#endif
#ifndef MRT_STEAL_SPREAD
#define MRT_STEAL_SPREAD 1
#endif
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)  // build ONE of the two TUs with it
// per wave of the last launch: start, pool exhausted, end (s_memrealtime, 100 MHz), workgroup
// + time inside successful / failed claim atomics (10-ns ticks) and their counts (ok | fail << 32)
__device__ unsigned long long g_wtimes[7 * 16384];
#if (MRT_TABLE_FTZ || !MRT_TABLE_FAST) && !MRT_TABLE_PEX  // the reader in one TU only (the FTZ build runs the Cornell kernels)
extern "C" int mrt_debug_wtimes(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wtimes), sizeof(unsigned long long) * 7 * (size_t)n) != hipSuccess;
}
#endif
#define WT_MARK(v) (v) = __builtin_amdgcn_s_memrealtime()
#else
#define WT_MARK(v) (void)0
#endif
#if defined(MRT_EXPERIMENTS) && defined(MRT_BSTATS)  // build ONE of the two TUs with it
namespace mrtd { __device__ unsigned long long g_bstats[64]; }
extern "C" int mrt_debug_bstats(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mrtd::g_bstats), sizeof(g_bstats)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[64] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(mrtd::g_bstats), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif
// resumable mesh walk (room + mesh kernels): the walk loop returns the wave to shading / new rays
// once at most P.walk_min lanes still walk (set on upload from the mesh BVH's size: 32, or 40 for
// BVHs of >= 2048 inner nodes -- measured: bunny, 2937 inner nodes, best at 40 (+4% over 32);
// teapot, ~1045, at 28-32 (40: -3%)) and at least MRT_WALK_OTHER lanes have other work
#ifndef MRT_WALK_OTHER
#define MRT_WALK_OTHER 16u
#endif
// walk steps between two yield checks of the resumable mesh walk (round 6: 2 against 1, teapot +1.5%,
// bunny +0.8%; 3: +1.0% / +0.6%, profiles/r06_ab.txt section 8)
// Path starts batched in the resumable mesh loop (round 6): the lanes whose path ended start new
// ones only once at least MRT_START_MIN of the wave's lanes are idle (or none is busy), so the path
// start (claim, PCG seeding, the camera ray with its disk-rejection draws) runs at a wider lane
// mask; the idle lanes wait for it through a walk.  Measured (profiles/r06_ab.txt section 13):
// teapot (fast) +0.6% at 8, +2.9% at 16; bunny (path-exact) +0.9% at 8, -1.2% at 16.  The plain loop
// (bvh_node scenes: book2 -0.1% / -1.0%, random spheres +0.5% / -0.3%) keeps 1 (MRT_START_MIN_PLAIN).
#ifndef MRT_START_MIN
#define MRT_START_MIN (MRT_FAST ? 16u : 8u)
#endif
#ifndef MRT_START_MIN_PLAIN
#define MRT_START_MIN_PLAIN 1u
#endif
#ifndef MRT_WALK_UNROLL
#define MRT_WALK_UNROLL 2
#endif
// Leaf postponing in the resumable mesh walk (mrt_trace.h mesh_step_spec): the path-exact build
// (the metal bunny, C4) chooses per step between a leaf step and an inner step by majority
// (MRT_SPEC_LEAF 0): bunny +0.8%; the fast build (teapot, C3) keeps mesh_step (-5.5% with it); a leaf
// step once 8 / 16 / 32 / 48 runs are parked: bunny -10% / -2.2% / -19% / -58% (profiles/r06_ab.txt
// sections 8 and 14)
#ifndef MRT_MESH_SPEC
#define MRT_MESH_SPEC MRT_TABLE_PEX
#endif
#ifndef MRT_SPEC_LEAF
#define MRT_SPEC_LEAF 0u
#endif
#if defined(MRT_EXPERIMENTS) && defined(MRT_WPE)  // experiment hook: override for every variant
#define MRT_OCC(F) MRT_WPE
#else
#define MRT_OCC(F) PathOcc<F>::W
#endif
// fold levels kept in LDS per lane (the rest in HBM): where the LDS budget at the target
// occupancy allows it
// (Cornell: 2 at 6 WGs/CU; wide variants at 3 WGs/CU: MRT_LEVK_WIDE; room + mesh: MRT_LEVK_MESH)
#ifndef MRT_LEVK_CORNELL
#define MRT_LEVK_CORNELL 2u
#endif
#ifndef MRT_LEVK_WIDE
#define MRT_LEVK_WIDE 2u
#endif
#ifndef MRT_LEVK_MESH
#define MRT_LEVK_MESH 0u
#endif
template <uint32_t F> struct PathLevLds {
    static constexpr uint32_t K = MRT_FWD_FOLD ? 0u  // no stored levels
                                  : ((F & 0xFFFFu & ~FT_BIASED) == (FT_LIN | FT_INST)) ? MRT_LEVK_CORNELL
                                  : PathOcc<F>::kWide                  ? MRT_LEVK_WIDE
                                  : ((F & FT_MESH) != 0)               ? MRT_LEVK_MESH
                                                                       : 0u;
};
// Path starts made a wave at a time (see the path loop): on in the tolerance-contract build for the
// shared-constructor loop of one-wave workgroups
#ifndef MRT_PATHQ
#define MRT_PATHQ MRT_FAST
#endif
// the plain path loop reads the scene's kernel arguments through an opaque pointer each iteration
// (round 5: book2 -1.5%, random spheres -1% per step; SGPR spills of book2's kernel 110 -> 35; in
// the Cornell kernels' shared-constructor loop it removed their 4 SGPR spills but not a step's time:
// 8.648 vs 8.655 ms, three rounds, not kept)
#ifndef MRT_OPAQUE_SCENE
#define MRT_OPAQUE_SCENE 1
#endif
// rounding-critical light samples handed to the exact arithmetic (mrt_shade.h light_critical): the
// fast-arithmetic builds' light-sampled variants (MRT_CRIT=0 builds it out: A/B)
#ifndef MRT_CRIT
#define MRT_CRIT 1
#endif
template <uint32_t F>
static constexpr bool kCrit = MRT_CRIT && MRT_FAST && (F & FT_BIASED) != 0;
// where crit_check finds the launch's list: PathParams (the kernel's only argument) starts the
// argument segment
template <uint32_t F>
static constexpr uint32_t kCritOff = kCrit<F> ? (uint32_t)offsetof(PathParams, rt) : 0u;
// the path kernel's scene arguments (P.sc) through an opaque pointer into the argument segment (P is
// the kernel's only argument: it starts the segment): read where used, not held in registers
MRT_DFN const DScene& kernarg_scene() {
    const MRT_CONST_AS DScene* sp =
        (const MRT_CONST_AS DScene*)((const MRT_CONST_AS char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(PathParams, sc));
    asm volatile("" : "+s"(sp));
    return *(const DScene*)sp;
}
// the same for the whole argument struct: what only a refill of the Cornell kernels' queue of path
// starts reads (the path key's and the claim's parameters, the camera's address) is scalar-loaded
// there, once per 64 starts, instead of held in SGPRs across the path loop
MRT_DFN const PathParams& kernarg_params() {
    const MRT_CONST_AS PathParams* pp = (const MRT_CONST_AS PathParams*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(pp));
    return *(const PathParams*)pp;
}
#ifndef MRT_OPAQUE_RESUME
#define MRT_OPAQUE_RESUME 0  // the same in the room + mesh kernels' resumable loop: measured C3 -0.6%, C4 0 (A/B hook)
#endif
template <uint32_t F> struct PathQ {
    static constexpr bool on = MRT_PATHQ && (F & FT_MESH) == 0 && !TreeOf<F>::on;
    // LDS words per lane slot: o, dir, time, PCG state + inc, index (12); + the wave's claim state
    static constexpr uint32_t words = on ? 13u : 0u;
};
// set bits of a wave mask below this lane (v_mbcnt: no per-lane 64-bit mask kept live)
MRT_DFN uint32_t rank_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
MRT_DFN uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
// wave-uniform values kept in SGPRs (the compiler otherwise held the pool bounds in VGPRs and
// spilled them to scratch, reloaded every claim)
MRT_DFN uint64_t uni64(uint64_t x) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}
// a path's radiance: three words (sample-major, coalesced)
MRT_DFN void store_radiance(float* dst, f3 L) {
    dst[0] = L.x;
    dst[1] = L.y;
    dst[2] = L.z;
}
template <uint32_t F>
__global__ void __launch_bounds__(TreeOf<F>::wg) __attribute__((amdgpu_waves_per_eu(MRT_OCC(F)))) MRT_PATH_KERNEL(PathParams P) {
    constexpr uint32_t LK = PathLevLds<F>::K;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    // the group's LDS (mrt_launch.h WaveLds): this wave's slice, the group's treelet behind the slices
    const WaveLds L{P.lds_frames, P.lds_rays, P.lds_mesh, P.lds_save, LK, PathQ<F>::words, kBox6Walk<F> != 0u, TreeOf<F>::wg / 64u};
    uint32_t* const slice = lds + wave * L.stride();
    LStack Lw = lds_stacks(L, slice, lane);
    if constexpr (TreeOf<F>::on) {
        // the workgroup's copy of the top wide nodes, filled once before any wave starts a path; no
        // other barrier follows in this persistent kernel
        float4* const tree = reinterpret_cast<float4*>(lds + L.tree_at());
        for (uint32_t i = threadIdx.x; i < P.tree_n * 4u; i += blockDim.x) tree[i] = P.tree_src[i];
        __syncthreads();
        Lw.tree = tree;
        Lw.tree_b = P.tree_n;
    }
    // A Cornell walk kernel's hit table, queue of path starts and basis axes: in a one-wave group the
    // wave's slice is the group's, so each address is a constant of the kernel, not a scalar register
    // held across the path loop (two of the 80 that eight waves per SIMD leave)
    static_assert(!kBox6Walk<F> || PathQ<F>::on, "the Cornell walk's basis axes live in the queue's claim row");
    uint32_t* const front = kBox6Walk<F> && TreeOf<F>::wg == 64u ? lds : slice;
    if constexpr (kBox6Walk<F>) {
        auto addr = [](uint32_t* p) -> uint32_t {
            const uint32_t a = (uint32_t)(uintptr_t)(MRT_LDS_AS uint32_t*)p;
            return TreeOf<F>::wg == 64u ? a : (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        };
        Lw.hits = addr(front + L.hit_table());
        Lw.axes = addr(front + L.axes_at());
    }
    const LStack Ls = Lw;
    // the wave's queue of path starts ([word][entry], PathQ)
    float* const Lq = kBox6Walk<F> ? (float*)(front + L.queue_at()) : (float*)(Ls.mesh + L.queue_past_mesh());
    const DScene& S = P.sc;
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const LevStore<LK> lev{(MRT_GLOBAL_AS v4f*)P.lev, P.lev_rows, (uint32_t)slot,
                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(MRT_LDS_AS uint32_t*)(Ls.mesh + L.levels_past_mesh()))};

    // main.cpp:180/235 stop on !G_isRunning: a launch of a cancelled render does no work (mrt_render
    // splits a cancellable render into several launches)
    if (__hip_atomic_load(P.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return;
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
    uint64_t wt0 = 0, wt_ex = 0, wt1 = 0, wt_f = 0, wt_aok = 0, wt_afail = 0, wt_n = 0;
    WT_MARK(wt0);
#endif
    // whether the lane holds a path.  Cornell walk: a 0 / 1 word, not a bool -- the flag crosses the
    // loop's blocks in a vector register either way, and a lane mask made from a word is one compare
    // where one made from a bool in a register was v_and + v_cmp
    std::conditional_t<kBox6Walk<F> != 0u, uint32_t, bool> active = false;
    uint32_t idx = 0;
    PathState ps;
    // The launch's paths are split into MRT_NPART equal contiguous partitions, one work counter
    // each (128 B apart): the waves of workgroup b start on partition b % MRT_NPART -- the XCD the
    // workgroup is dispatched to, round robin -- and move on to the next partition once theirs is
    // handed out.  One counter for all 7168 waves serialised ~1 M claims per C2 launch on one
    // address (measured: claims 4x larger, 1024 paths, made the kernel 14% faster).
    // Every wave's first claim is static (the waves of a partition take its first batches in order);
    // its counter hands out what follows, so a launch does not open with one atomic per wave (short
    // launches only -- P.static_first, set by the host when a wave gets fewer than 64 claims: there
    // the opening atomics are a visible share; in long launches the static batch of a wave that
    // starts late in a pipelined step delays that launch's end).
    const uint32_t wpb = blockDim.x >> 6;  // waves per workgroup
    uint32_t part = blockIdx.x % MRT_NPART;  // wave-uniform: the partition claims come from
    uint32_t part_tries = 0;                 // partitions found handed out
    // the partitions a wave visits after its own: every one (step odd, coprime with 8); with
    // MRT_STEAL_SPREAD the waves of one partition leave it in four directions instead of one
    // (a Cornell walk kernel keeps it in the claim row between claims, with the state below)
    uint32_t steal_step = MRT_STEAL_SPREAD ? 1u + 2u * ((blockIdx.x / MRT_NPART) & 3u) : 1u;
    bool in_tail = false;                    // the partition's last paths: small claims
    uint64_t pool_next = 0, pool_end = 0;    // wave-uniform: the wave's claimed, not yet taken paths
    if (P.static_first) {
        pool_next = uni64(umin64(P.part_base[part] + ((uint64_t)(blockIdx.x / MRT_NPART) * wpb + wave) * MRT_BATCH, P.part_base[part + 1]));
        pool_end = uni64(umin64(pool_next + MRT_BATCH, P.part_base[part + 1]));
    }
    bool exhausted = false;  // no paths left in the pool nor in any partition
    // Queue kernels keep the claim state (pool bounds, partition) in LDS between claims -- it is
    // touched once per 64 path starts -- so it holds no registers across the path loop (held in
    // registers it cost VGPR spills to scratch: 1.2 GB/launch of extra HBM writes on C2).
    uint32_t* const Lc = reinterpret_cast<uint32_t*>(Lq) + WaveLds::kQueueRows * WaveLds::kLanes;
    // (Cornell walk, eight waves per SIMD: 80 scalar registers.  "lane == 0" is made where it is used --
    // as a mask held across the path loop it was two of them -- and the steal step lives in the row)
    auto first_lane = [&]() -> bool {
        uint32_t l = lane;
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (kBox6Walk<F>) asm volatile("" : "+v"(l));
#endif
        return l == 0;
    };
    auto cold_store = [&]() {
        if (first_lane()) {
            Lc[0] = (uint32_t)pool_next;
            Lc[1] = (uint32_t)(pool_next >> 32);
            Lc[2] = (uint32_t)pool_end;
            Lc[3] = (uint32_t)(pool_end >> 32);
            Lc[4] = part | (part_tries << 8) | ((uint32_t)in_tail << 16) | (kBox6Walk<F> ? steal_step << 24 : 0u);
        }
    };
    auto cold_load = [&]() {
        auto rd = [&](uint32_t k) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)Lc[k]); };
        pool_next = (uint64_t)rd(0) | ((uint64_t)rd(1) << 32);
        pool_end = (uint64_t)rd(2) | ((uint64_t)rd(3) << 32);
        const uint32_t w = rd(4);
        part = w & 0xFFu;
        part_tries = (w >> 8) & 0xFFu;
        in_tail = ((w >> 16) & 1u) != 0;
        if constexpr (kBox6Walk<F>) steal_step = w >> 24;
    };
    if constexpr (PathQ<F>::on) cold_store();
    uint32_t done_rays = 0;
    PhaseClock ph{};
#ifdef MRT_PHASES
    ph.t = __builtin_amdgcn_s_memtime();
#endif
    // the next c path indices of the wave's pool, the lane of rank r taking index *i (>= n_paths:
    // none); the pool refilled by one atomic per claim (work_queue::getWork, work_queue.cpp:158-166)
    auto claim = [&](uint32_t c, uint32_t r, bool want, uint64_t* i) {
        const PathParams& Q = P;
        const uint32_t have = (uint32_t)(pool_end - pool_next);
        uint64_t nb = 0, ne = 0;
        if (have < c) {
            while (part_tries < MRT_STEAL_TRIES) {  // wave-uniform
                const uint64_t pe = Q.part_base[part + 1], p0 = Q.part_dyn[part];
                const uint32_t batch = in_tail ? MRT_TAIL_BATCH : MRT_BATCH;
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                uint64_t wt_a = 0;
                WT_MARK(wt_a);
#endif
                if (first_lane()) {
                    nb = p0 + atomicAdd(Q.counter + part * MRT_COUNTER_STRIDE, (unsigned long long)batch);
                    // every 32nd claim: a system-scope store to host memory, read by mrt_progress
                    // without any GPU queue (a device-to-host copy could wait behind this launch)
                    if (Q.hprog && (((nb - p0) / batch) & 31u) == 0)
                        __hip_atomic_store(Q.hprog + part, nb + batch - Q.part_base[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                // lane 0's claim to every lane, as a scalar (the whole wave runs claim())
                nb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(nb >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)nb);
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                {
                    uint64_t wt_b = 0;
                    WT_MARK(wt_b);
                    if (nb < pe) { wt_aok += wt_b - wt_a; wt_n += 1; }
                    else { wt_afail += wt_b - wt_a; wt_n += 1ull << 32; }
                }
#endif
                if (nb < pe) {
                    ne = umin64(nb + batch, pe);
                    // near the partition's end, claims shrink so the last ones finish together
#if MRT_STEAL_SMALL
                    in_tail = pe - ne <= Q.tail_zone / MRT_NPART;
#else
                    in_tail = in_tail || pe - ne <= Q.tail_zone / MRT_NPART;
#endif
                    break;
                }
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                if (wt_f == 0) WT_MARK(wt_f);
#endif
                part_tries++;
                part = (part + steal_step) % MRT_NPART;
                // (MRT_STEAL_SMALL: the first claim on the next partition is a small one -- it is
                // usually in its own tail zone -- and the claim's position decides the next size)
                in_tail = MRT_STEAL_SMALL;
            }
        }
        if (want) {
            const uint64_t j = nb + (r - have);
            *i = r < have ? pool_next + r : (j < ne ? j : ~0ull);
        }
        if (have < c) {
            pool_next = umin64(nb + (c - have), ne);
            pool_end = ne;
        } else {
            pool_next += c;
        }
        exhausted = part_tries >= MRT_STEAL_TRIES && pool_next >= pool_end;
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
        if (exhausted && wt_ex == 0) WT_MARK(wt_ex);
#endif
    };
    // The same for a Cornell walk kernel's refill, the pool in 32 bits (mrt_launch.h pool_claim32: a
    // launch's path indices are below 2^32): the pool bounds, the partition's end and the tail-zone test
    // are scalar compares and selects instead of 64-bit vector ones on broadcast values, a lane's index
    // one 32-bit add.  The counters, the progress word and the claim row's words are what claim() makes;
    // the row's words 1 and 3 (the bounds' high halves) stay the zeros the kernel's first store wrote.
    uint32_t pool32_next = 0, pool32_end = 0;
    auto cold_store32 = [&]() {
        if (first_lane()) {
            Lc[0] = pool32_next;
            Lc[2] = pool32_end;
            Lc[4] = part | (part_tries << 8) | ((uint32_t)in_tail << 16) | (steal_step << 24);
        }
    };
    auto cold_load32 = [&]() {
        auto rd = [&](uint32_t k) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)Lc[k]); };
        pool32_next = rd(0);
        pool32_end = rd(2);
        const uint32_t w = rd(4);
        part = w & 0xFFu;
        part_tries = (w >> 8) & 0xFFu;
        in_tail = ((w >> 16) & 1u) != 0;
        steal_step = w >> 24;
    };
    auto claim32 = [&](uint32_t c, uint32_t r, uint32_t* i, const PathParams& Q) {
        const uint32_t have = pool32_end - pool32_next;
        uint32_t nb = 0, ne = 0;
        if (have < c) {
            while (part_tries < MRT_STEAL_TRIES) {  // wave-uniform
                const uint32_t pe = (uint32_t)Q.part_base[part + 1];
                const uint64_t p0 = Q.part_dyn[part];
                const uint32_t batch = in_tail ? MRT_TAIL_BATCH : MRT_BATCH;
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                uint64_t wt_a = 0;
                WT_MARK(wt_a);
#endif
                uint64_t got = 0;
                if (first_lane()) {
                    got = p0 + atomicAdd(Q.counter + part * MRT_COUNTER_STRIDE, (unsigned long long)batch);
                    if (Q.hprog && (((got - p0) / batch) & 31u) == 0)
                        __hip_atomic_store(Q.hprog + part, got + batch - Q.part_base[part], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                got = uni64(got);  // lane 0's claim to every lane, as a scalar
                const bool ok = pool_claim32(got, batch, pe, &nb, &ne);
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                {
                    uint64_t wt_b = 0;
                    WT_MARK(wt_b);
                    if (ok) { wt_aok += wt_b - wt_a; wt_n += 1; }
                    else { wt_afail += wt_b - wt_a; wt_n += 1ull << 32; }
                }
#endif
                if (ok) {
#if MRT_STEAL_SMALL
                    in_tail = pool_tail32(pe, ne, Q.tail_zone);
#else
                    in_tail = in_tail || pool_tail32(pe, ne, Q.tail_zone);
#endif
                    break;
                }
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
                if (wt_f == 0) WT_MARK(wt_f);
#endif
                part_tries++;
                part = (part + steal_step) % MRT_NPART;
                in_tail = MRT_STEAL_SMALL;
            }
            *i = pool_index32(r, have, pool32_next, nb, ne);
        } else {
            *i = pool32_next + r;  // (r < c <= have)
        }
        pool_take32(c, have, nb, ne, &pool32_next, &pool32_end);
        exhausted = part_tries >= MRT_STEAL_TRIES && pool32_next >= pool32_end;
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
        if (exhausted && wt_ex == 0) WT_MARK(wt_ex);
#endif
    };
    auto begin_path = [&]() {
        ps.depth = 0;
        ps.nlev = 0;
#if MRT_FWD_FOLD
        ps.T = f3{1.0f, 1.0f, 1.0f};
#endif
        active = true;
    };
    // Lanes without a path take the next path indices from the wave's pool (ballot + mbcnt
    // compaction).  start(u, v) begins a lane's path at camera coordinates (u, v) with its PCG stream
    // seeded from the path key (path_key_of).
    auto take_paths = [&](auto&& start) {
        const uint64_t need = __ballot(!active);
        if (!need || exhausted) return;
        const uint32_t c = (uint32_t)__popcll(need);
        uint64_t i = 0;
        claim(c, active ? 0u : rank_below(need), !active, &i);
        PH_MARK(ph, 0);
        if (!active && i < P.n_paths) {
            idx = (uint32_t)i;
            BSTAT(10);
            float u, v;
            path_key_of(P, idx, ps.rng, &u, &v);
            start(u, v);
            begin_path();
        }
        PH_MARK(ph, 4);
    };
    // a finished path: the recursion's fold, radiance out (sample-major, coalesced), rays counted
    auto finish_path = [&](f3 L) {
        L = end_path(ps, lev, L);
        PH_MARK(ph, 5);
#if defined(MRT_EXPERIMENTS) && defined(MRT_EXP_NOSTORE)  // experiment: what the radiance store costs
        if (__float_as_uint(L.x) == 0x7fc00123u)
#endif
        store_radiance(P.rad + (size_t)idx * 3, L);
        if (P.path_rays) P.path_rays[idx] = ps.rays();
        done_rays += ps.rays();
        active = false;
    };
    // mesh variants keep one constructor per branch: the shared-constructor loop spills there
    // (bunny -4%, teapot -5%; Cornell +1.8%, book2 0)
#ifndef MRT_SHARED_WIDE
#define MRT_SHARED_WIDE 0  // not the wide (bvh_node) variants: the plain loop has 6 spills instead of 29 there
                           // (random spheres +4.4%, scene 1 +5%; profiles/r03_ab.txt)
#endif
    constexpr bool kShared = (F & FT_MESH) == 0 && (MRT_SHARED_WIDE || !PathOcc<F>::kWide);
    constexpr bool kResume = MRT_SIG_OF(F) == SIG_ROOM_MESH;
    static_assert(kShared || !kBox6Walk<F>, "the Cornell fast walk's hit table is set up by the shared-constructor loop");
    if constexpr (kShared) {
        // One iteration: (1) every lane with a ray traces one segment; a path that ends is folded
        // and stored; (2) lanes without a path take new ones (camera ray arguments); (3) ONE
        // make_ray for every lane with a next ray -- camera and scattered rays alike, instead of one
        // constructor per branch at partial lane occupancy; (4) diffuse scatters finish their pdfs
        // on the new ray.
        uint32_t q_head = 0, q_n = 0;  // wave-uniform: the queue's next entry, its valid entries
        // The radiance store of a path that ended is held in registers and issued in the NEXT
        // iteration, after the hit, beside the material load: the code waits for the vector memory
        // counter (stores count in vmcnt on gfx950) right after a store wherever it reuses nearby
        // registers, which stalled the wave for the store's whole round trip every iteration
        // (measured: SQ_WAIT_ANY 23 -> 36 quad-cycles per ray once the path loop had fewer
        // instructions); beside the material load the two round trips overlap.
        // The Cornell walk (kBox6Walk) reads its material from the wave's LDS hit table: the common
        // path of its iteration has no vector-memory load for a store to share vmcnt with, so it stores
        // where the path ends (kHeldStore off) and the four held registers and the lane mask are gone
        // from its loop: 64 VGPRs, eight waves per SIMD.
        constexpr bool kHeldStore = !kBox6Walk<F>;
        f3 st_v{0.0f, 0.0f, 0.0f};
        uint32_t st_off = 0;  // byte offset of the path's radiance (a launch chunk is < 4 GiB)
        bool st_pend = false;
        // Cornell fast walk: the sphere's 1 / radius, once per launch (mrt_sig.h cornell_sphere_inv_rad)
        float sph_inv_rad = 0.0f;
        // ... and the walk's scene words and the depth limit, held in scalar registers for the launch
        // (mrt_sig.h CornellWords)
        std::conditional_t<kBox6Walk<F> != 0u, CornellWords, NoCornellWords> cw{};
        if constexpr (kBox6Walk<F>) {
            sph_inv_rad = cornell_sphere_inv_rad(const_ptr(S.prog));
            cw = cornell_words(const_ptr(S.prog), P.max_bounces,
                               (S.biased != MRT_NONE ? 1u << kCwBiased : 0u) | (S.light_once ? 1u << kCwLightOnce : 0u) |
                                   (S.blist ? 1u << kCwBlist : 0u) | (P.path_rays ? 1u << kCwPathRays : 0u));
            // the scene's hit table (kHitCount entries behind the program's END op, mrt_tables.hip
            // cornell_hit_fill) into the wave's LDS: the first three 16-byte quads of each entry, one
            // per lane, packed (entry e's quad q lands at quad 3 e + q = the lane).  Only this wave
            // reads them, after this store in its own LDS queue: no barrier.
            const uint32_t e = lane / 3u, qd = lane - e * 3u;
            if (lane < kHitCount * (kHitLdsWords / 4u)) {
                const v4f* src = reinterpret_cast<const v4f*>(S.prog + kSigs[SIG_CORNELL].n) + e * (kHitWords / 4u) + qd;
                const v4f q = *src;
                ((MRT_LDS_AS v4f*)(uintptr_t)Ls.hits)[lane] = q;
                // the lane that holds an entry's normal (quad 0) also makes its basis axis v, with the
                // per-lane basis' own function on the same bits, into the wave's axes (trace_split's
                // diffuse branch reads it by identity; the sphere's entry has no normal, its quad is not used).
                // The claim state beside it is words 0-4 of the row, written by lane 0 above.
                if (qd == 0u) {
                    const f3 v = onb_axis_v(f3{q.x, q.y, q.z});
                    ((MRT_LDS_AS v4f*)(uintptr_t)Ls.axes)[e] = v4f{v.x, v.y, v.z, 0.0f};
                }
            }
            // the light's quad in the sphere's slot of the axes (after the stores above, the sphere's
            // unused axis among them: one wave's LDS stores land in order): the rect's extents and area
            // from the launch's words, once per wave (mrt_sig.h cornell_light_quad), and whether a scatter's
            // pdf can be negative (kCwPdfSigned): not under the walk's light with its area's sign clear --
            // +0, positive, or a NaN of that sign
            const LightQuad lq = cornell_light_quad(__uint_as_float(cw.light.b0), __uint_as_float(cw.light.b1),
                                                    __uint_as_float(cw.light.b2), __uint_as_float(cw.light.b3));
            if (lane == kLightQuadSlot * 3u) ((MRT_LDS_AS v4f*)(uintptr_t)Ls.axes)[kLightQuadSlot] = v4f{lq.ex, lq.ez, lq.area, 0.0f};
            const bool area_ok = (__float_as_uint(lq.area) >> 31) == 0u;
            cw.flags |= uniform_u32(S.biased != MRT_NONE && !(S.light_once && area_ok) ? 1u << kCwPdfSigned : 0u);
        }
        for (;;) {
            if constexpr (kBox6Walk<F>) cornell_words_hold(cw);
            bool want_ray = false;
            // the next ray's arguments: written and read within one iteration (declared here, a
            // field a branch leaves unset is dead, not carried round the loop in copied registers)
            PendRay pr;
            // Cornell walk: the next ray's origin and inside count start as the lane's own and are
            // assigned back below for EVERY lane, not under want_ray (a lane without a next ray holds
            // no path: its ray is never read again).  Assigned under the mask, the old values had to
            // survive in the lanes outside it, so the new ones were made elsewhere and copied in:
            // four register copies per iteration and four VGPRs (64 -> 60).
            if constexpr (kBox6Walk<F>) { pr.o = ps.r.o; pr.inside = ps.r.inside; }
            if (active) {
                f3 L{0.0f, 0.0f, 0.0f};  // (left undefined, it was carried round the loop in copied registers)
                // (the held store is issued inside, after the hit, beside the material load)
                uint32_t max_bounces = P.max_bounces;
                if constexpr (kBox6Walk<F>) max_bounces = cw.max_bounces;
                const bool ended = trace_split<F, LK>(S, ps, max_bounces, lev, Ls, &L, &pr, ph, [&]() {
                    if constexpr (kHeldStore) {
                        if (st_pend) store_radiance(reinterpret_cast<float*>(reinterpret_cast<char*>(P.rad) + st_off), st_v);
                        st_pend = false;
                    }
                }, CritSink{idx, kCritOff<F>}, sph_inv_rad, cornell_ptr(cw));
                PH_MARK(ph, 2);
                if (ended) {
                    if constexpr (kHeldStore) {
                        st_v = end_path(ps, lev, L);
                        st_off = idx * 12u;
                        st_pend = true;
                    } else {
                        // the same three words at the same address, idx * 12 as two shift-adds (in the
                        // multiply's place; profiles/r13_valu_cost.txt prices the two forms alike)
                        const f3 R = end_path(ps, lev, L);
                        uint32_t i4 = idx << 2;
#if defined(__HIP_DEVICE_COMPILE__)
                        asm volatile("" : "+v"(i4));  // (kept apart from the sum: rejoined, it is the multiply again)
#endif
                        store_radiance(reinterpret_cast<float*>(reinterpret_cast<char*>(P.rad) + ((i4 << 1) + i4)), R);
                    }
                    if constexpr (kBox6Walk<F>) {
                        if (cornell_flag(&cw, kCwPathRays)) kernarg_params().path_rays[idx] = ps.rays();
                    } else if (P.path_rays) P.path_rays[idx] = ps.rays();
                    done_rays += ps.rays();
                    active = false;
                } else {
                    want_ray = true;
                }
            }
            PH_MARK(ph, 3);
            if constexpr (PathQ<F>::on) {
                // new paths from the wave's queue of path starts; when it runs short, the next 64
                // starts are made at once, one per lane at full width (path key, PCG seeding, the
                // camera's disk-rejection and time draws), instead of by the ~1/3 of lanes whose
                // path just ended: the same paths with the same streams, in the same order
                // (the time word: only kernels with moving spheres read a ray's time; the others neither
                // compute nor store it, the refill steps their streams over its draw)
                constexpr bool kTimeWord = (F & FT_MOVING) != 0;
                auto pop = [&](uint32_t e) {
                    const float* q = Lq + e;
                    pr.o = f3{q[0], q[64], q[128]};
                    pr.dir = f3{q[192], q[256], q[320]};
                    pr.time = kTimeWord ? q[384] : 0.0f;
                    ps.rng.state = (uint64_t)__float_as_uint(q[448]) | ((uint64_t)__float_as_uint(q[512]) << 32);
                    ps.rng.inc = (uint64_t)__float_as_uint(q[576]) | ((uint64_t)__float_as_uint(q[640]) << 32);
                    idx = __float_as_uint(q[704]);
                    pr.inside = 0;
                    pr.kind = 0;
                    want_ray = true;
                    begin_path();
                };
                const uint64_t need = __ballot(!active);
                const uint32_t c = (uint32_t)__popcll(need);
                const uint32_t avail = q_n - q_head;
                if (c != 0u && (avail != 0u || !exhausted)) {
                    const uint32_t rank = active ? 64u : rank_below(need);
                    if (rank < avail) pop(q_head + rank);
                    if (c <= avail) {
                        q_head += c;
                    } else {
                        q_head = q_n = 0;
                        if (!exhausted) {
                            uint64_t i = 0;
                            // (a Cornell walk kernel reads the refill's parameters here, not across the loop,
                            // and claims in 32 bits)
                            const PathParams& Q = kBox6Walk<F> ? kernarg_params() : P;
                            uint32_t j = 0;
                            if constexpr (kBox6Walk<F>) {
                                cold_load32();
                                claim32(64u, lane, &j, Q);
                                cold_store32();
                            } else {
                                cold_load();
                                claim(64u, lane, true, &i);
                                cold_store();
                            }
                            const bool valid = kBox6Walk<F> ? j < Q.n_paths : i < Q.n_paths;
                            BSTATC(17, valid);
                            if (valid) {
                                BSTAT(10);
                                Pcg rng;
                                float u, v, time;
                                f3 o, dir;
                                // the index as the 32-bit value it is (i < n_paths is known here, and
                                // path_coords' conversion to double was made from all 64 bits)
                                uint32_t i32 = kBox6Walk<F> ? j : (uint32_t)i;
#if defined(__HIP_DEVICE_COMPILE__)
                                if constexpr (!kBox6Walk<F>) asm volatile("" : "+v"(i32));
#endif
                                path_key_of(Q, i32, rng, &u, &v);
                                camera_ray_args<kTimeWord>(Q.sc, rng, u, v, &o, &dir, &time);
                                float* q = Lq + lane;
                                q[0] = o.x; q[64] = o.y; q[128] = o.z;
                                q[192] = dir.x; q[256] = dir.y; q[320] = dir.z;
                                if constexpr (kTimeWord) q[384] = time;
                                q[448] = __uint_as_float((uint32_t)rng.state);
                                q[512] = __uint_as_float((uint32_t)(rng.state >> 32));
                                q[576] = __uint_as_float((uint32_t)rng.inc);
                                q[640] = __uint_as_float((uint32_t)(rng.inc >> 32));
                                q[704] = __uint_as_float(i32);
                            }
                            q_n = (uint32_t)__popcll(__ballot(valid));  // a prefix of the lanes
                            const uint32_t r2 = rank - avail;
                            if (!active && r2 < q_n) pop(r2);
                            q_head = min(c - avail, q_n);
                        }
                    }
                }
                PH_MARK(ph, 4);
            } else {
                take_paths([&](float u, float v) {
                    camera_ray_args(S, ps.rng, u, v, &pr.o, &pr.dir, &pr.time);
                    pr.inside = 0;
                    pr.kind = 0;
                    want_ray = true;
                });
            }
            if (!__any(active)) {  // the last store
                if constexpr (kHeldStore) {
                    if (st_pend) store_radiance(reinterpret_cast<float*>(reinterpret_cast<char*>(P.rad) + st_off), st_v);
                }
                break;
            }
            PH_MARK(ph, 0);
            BSTATC(15, active);
            if constexpr (kBox6Walk<F>) { ps.r.o = pr.o; ps.r.inside = pr.inside; }
            if (want_ray) {
                BSTATC(12, pr.kind != 0);
                // Cornell walk: the light's area for the scatter's pdf below, the third word of the wave's
                // light quad (mrt_sig.h cornell_light_quad) at a wave-uniform address, issued ahead of the
                // ray's constructor, which covers its latency (one VGPR until finish_scatter).  A volatile
                // read: a plain one is sunk into the pdf's block, where the code waits for it at once.
                float light_area = 0.0f;
                if constexpr (kBox6Walk<F> != 0u && (F & FT_BIASED) != 0u)
                    light_area = *(const volatile MRT_LDS_AS float*)(uintptr_t)(Ls.axes + kLightQuadSlot * (kHitAxisWords * 4u) + 8u);
                ps.r = make_ray(kBox6Walk<F> ? ps.r.o : pr.o, pr.dir, pr.time, kBox6Walk<F> ? ps.r.inside : pr.inside);
                // the Cornell fast walk's light test, once per ray: the scatter's light pdf below and
                // the next iteration's walk both read it (one VGPR across the back edge)
                if constexpr (kBox6Walk<F>) ps.lt = cornell_light_t<F>(cw.light, ps.r);
                PH_MARK(ph, 8);
                if (pr.kind) finish_scatter<F, LK>(S, ps, lev, pr, cornell_ptr(cw), light_area);
            }
            PH_MARK(ph, 7);
        }
    } else if constexpr (kResume) {
        // Cornell room + one pod_bvh mesh (scenes 8 / 9): the mesh walk is RESUMABLE.  Lanes walk
        // the BVH for different numbers of steps, so a walk run to completion inside one segment
        // leaves most lanes of the wave idle while the longest walks finish (lane utilisation
        // 0.13-0.17 measured).  Here a lane's walk state (node ref, stack depth, its LDS stack, the
        // walls' closest hit) persists across iterations; the walk loop hands the wave back once
        // few lanes still walk and enough others can shade or start new rays, and the stragglers
        // resume next iteration beside fresh rays (Aila & Laine 2009 "dynamic ray fetch", per
        // lane).  Every lane runs the same operations in the same order as mesh_hit: bit-exact.
        constexpr uint32_t PH_BEGIN = 1, PH_WALK = 2, PH_DONE = 3;
        using W = SigWalk<F, SIG_ROOM_MESH>;
        constexpr uint32_t kMeshPC = 7;  // LIST, 6 rects, MESH, LIST_END (mrt_sig.h kSigs)
        static_assert(kSigs[SIG_ROOM_MESH].op[kMeshPC] == LOP_MESH, "room + mesh program shape");
        const MRT_CONST_AS LinOp* prog = const_ptr(S.prog);
        uint32_t phase = 0, ref = 0, msp = 0;
#if MRT_MESH_SPEC
        uint32_t pref = 0;  // the parked leaf run (mesh_step_spec)
#endif
        SigState w;
        w.closest = FLT_MAX_;
        w.hnode = MRT_NONE;
        w.hinst = MRT_NONE;
        w.hdone = false;
        HitRec rec;
        for (;;) {
#if MRT_OPAQUE_RESUME
            const DScene& S = kernarg_scene();  // (shadows P.sc for this iteration)
            const MRT_CONST_AS LinOp* prog = const_ptr(S.prog);
#endif
            if (MRT_START_MIN <= 1 || (uint32_t)__popcll(__ballot(!active)) >= MRT_START_MIN || !__any(active))
                take_paths([&](float u, float v) {
                    ps.r = camera_ray(S, ps.rng, u, v);
                    phase = PH_BEGIN;
                });
            if (!__any(active)) break;
            PH_MARK(ph, 0);
            if (phase == PH_BEGIN) {  // the room's walls (scene_hit_sig's ops 0..6), then the mesh root box
                w.cur = ps.r;
                w.closest = FLT_MAX_;
                w.hnode = MRT_NONE;
                w.hinst = MRT_NONE;
                w.hdone = false;
                const MRT_CONST_AS LinOp& lo = prog[0];
                const bool in = !(LOP_FLAGS(lo) & MRT_F_HASBOX) || lin_box(lo, w.cur, 0.001f, w.closest);
#if MRT_FAST_ROOM
                // tolerance contract: the room's five walls as one slab test (cornell_room_fill; the
                // box test of the root list only skips work), then the light (op 3)
                (void)in;
                static_assert(kSigs[SIG_ROOM_MESH].op[kSigs[SIG_ROOM_MESH].n - 1] == LOP_END, "room in the END op");
                room_walls_op(prog[kSigs[SIG_ROOM_MESH].n - 1], w.cur, 0.001f, w);
                W::template run<3, 4>(S, prog, 0.001f, w, true, rec, Ls);
#else
                W::template run<1, kMeshPC>(S, prog, 0.001f, w, in, rec, Ls);
#endif
                const mrt_node mn = ld_node(const_ptr(S.nodes) + prog[kMeshPC].node);
                const MRT_CONST_AS mrt_mesh_node& rt = const_ptr(S.mnodes)[mn.a];
                const bool enter = in && aabb_hit(f3{rt.bmin[0], rt.bmin[1], rt.bmin[2]}, f3{rt.bmax[0], rt.bmax[1], rt.bmax[2]}, ps.r,
                                                  0.001f, w.closest);
                ref = mn.b;
#if MRT_MESH_SENT
                Ls.mesh[lane] = kMeshEmpty;  // the stack's bottom (mrt_trace.h kMeshEmpty)
                msp = 1;
#else
                msp = 0;
#endif
#if MRT_MESH_SPEC
                pref = 0;
#endif
                phase = enter ? PH_WALK : PH_DONE;
            }
            PH_MARK(ph, 1);
            // at least one step per iteration for every walking lane (no lane starves), then more
            // while enough lanes walk or too few have anything else to do
            while (__any(phase == PH_WALK)) {
                // some walking lane's ray is not nice (the box tests' slow path; wave-uniform)
                const bool bad = any_lane(phase == PH_WALK && !ps.r.nice);
#pragma unroll
                for (int u = 0; u < MRT_WALK_UNROLL; u++) {  // (A/B hook: steps between two yield checks)
#if MRT_MESH_SPEC
                    // the wave's choice: a leaf step once enough runs are parked or no inner step is left
                    const bool can_inner = phase == PH_WALK && ref != kMeshEnd && !((ref & MESH_LEAF) && pref != 0u);
                    // (MRT_SPEC_LEAF 0: a leaf step when at least as many lanes can take one as an inner step)
                    const uint32_t n_leaf = (uint32_t)__popcll(__ballot(phase == PH_WALK && pref != 0u));
                    const uint32_t n_inner = (uint32_t)__popcll(__ballot(can_inner));
                    const bool leaf_iter = MRT_SPEC_LEAF ? (n_leaf >= MRT_SPEC_LEAF || n_inner == 0u) : n_leaf >= n_inner;
                    if (phase == PH_WALK) {
                        const uint32_t st = mesh_step_spec<false>(S, ps.r, 0.001f, w.closest, rec, Ls, ref, pref, msp, w.hdone, leaf_iter, bad);
                        if (st == 1u) w.hnode = kMeshPC;  // w.closest = the hit's t, w.hdone set
                        phase = st != 0u ? PH_DONE : PH_WALK;
                    }
#else
                    if (phase == PH_WALK) {
                        const mrt_node mn = ld_node(const_ptr(S.nodes) + prog[kMeshPC].node);
                        const uint32_t st = mesh_step<false, true>(S, mn, ps.r, 0.001f, w.closest, rec, Ls, ref, msp, w.hdone, bad);
                        if (st == 1u) w.hnode = kMeshPC;  // w.closest = the hit's t, w.hdone set
                        phase = st != 0u ? PH_DONE : PH_WALK;
                    }
#endif
                }
                if ((uint32_t)__popcll(__ballot(phase == PH_WALK)) <= P.walk_min &&
                    (uint32_t)__popcll(__ballot(phase == PH_DONE || (!active && !exhausted))) >= MRT_WALK_OTHER)
                    break;  // others can shade / start rays: done lanes, or idle lanes with paths left
            }
            PH_MARK(ph, 6);
            if (phase == PH_DONE) {
                if (w.hnode == kMeshPC) {  // the mesh's record, deferred by the walk (mesh_step<.., true>)
                    const mrt_node mn = ld_node(const_ptr(S.nodes) + prog[kMeshPC].node);
                    mesh_hit_rec(S, mn, ps.r, w.closest, rec);
                } else if (!w.hdone && w.hnode != MRT_NONE) {
                    W::template derive<0>(prog, w, ps.r, ps.r, rec);
                }
                f3 L{0.0f, 0.0f, 0.0f};
                const bool ended = shade_hit<F, LK>(S, ps, P.max_bounces, lev, w.hnode != MRT_NONE, rec, &L, ph, CritSink{idx, kCritOff<F>});
                PH_MARK(ph, 2);
                phase = PH_BEGIN;
                if (ended) {
                    finish_path(L);
                    phase = 0;
                }
            }
            PH_MARK(ph, 3);
        }
    } else {
        for (;;) {
            if (MRT_START_MIN_PLAIN <= 1 || (uint32_t)__popcll(__ballot(!active)) >= MRT_START_MIN_PLAIN || !__any(active))
                take_paths([&](float u, float v) { ps.r = camera_ray(S, ps.rng, u, v); });
            if (!__any(active)) break;
            PH_MARK(ph, 0);
#if MRT_OPAQUE_SCENE
            // the scene's kernel arguments re-derived each iteration through an opaque constant
            // pointer: its fields are scalar-loaded at their uses in the segment instead of held in
            // SGPRs across the path loop (which spilled them into VGPR lanes)
            const DScene& Sseg = kernarg_scene();
#else
            const DScene& Sseg = S;
#endif
            if (active) {
                f3 L{0.0f, 0.0f, 0.0f};
                const bool ended = trace_segment<F, LK>(Sseg, ps, P.max_bounces, lev, Ls, &L, ph, CritSink{idx, kCritOff<F>});
                PH_MARK(ph, 2);
                if (ended) finish_path(L);
            }
            PH_MARK(ph, 3);
        }
    }
#ifdef MRT_PHASES
    if (lane == 0)
        for (int i = 0; i < 12; i++) atomicAdd(&g_phases[i], (unsigned long long)ph.a[i]);
#endif
#if defined(MRT_EXPERIMENTS) && defined(MRT_WTIMES)
    WT_MARK(wt1);
    if (lane == 0) {
        const size_t g = ((size_t)blockIdx.x * (blockDim.x >> 6) + wave) * 7;
        if (g + 6 < 7 * 16384) {
            g_wtimes[g + 4] = wt_aok;
            g_wtimes[g + 5] = wt_afail;
            g_wtimes[g + 6] = wt_n;
            g_wtimes[g] = wt0;
            g_wtimes[g + 1] = wt_ex;
            g_wtimes[g + 2] = wt1;
            g_wtimes[g + 3] = (uint64_t)blockIdx.x | ((wt_f ? wt_f - wt0 : 0ull) << 20);
        }
    }
#endif
    // one 64-bit add per wave
    uint64_t my = done_rays;
    for (int off = 32; off > 0; off >>= 1) my += __shfl_xor(my, off);
    if (lane == 0 && my) atomicAdd(P.rays, (unsigned long long)my);
}

// The exact arithmetic (the path-exact build: the reference's, forward fold) for the paths a
// fast-arithmetic launch listed as rounding-critical (mrt_shade.h light_critical; PathParams::rt):
// each traced from its camera ray to its end as the reference traces it -- including its
// non-finite end, which the fold then turns into main.cpp:162-164's doubling -- and its radiance
// written over the fast one in the launch's radiance buffer, before the fold.  A few hundred to a
// few thousand paths per launch: one-wave groups over the list, one path per lane; the last group
// to finish clears the list for the next launch.  (The launch's ray count stays the fast paths'.)
// The Cornell variant at eight waves per SIMD, that is at most 64 VGPRs (one spilled): under
// MRT_RF_FOLD_ASYNC its waves run beside the next launch's path kernel, each in the slot a 64-VGPR
// path wave left free (mrt_context.h kSideSlots).  The other variants' launches keep their grids
// and their retrace its registers.
template <uint32_t F>
static constexpr bool kRetrace = MRT_TABLE_PEX && MRT_FWD_FOLD && (F & FT_BIASED) != 0 && !kPathExact<F>;
template <uint32_t F>
static constexpr uint32_t kRetraceWpe = MRT_SIG_OF(F) == SIG_CORNELL ? 8u : 1u;
#if MRT_TABLE_PEX
template <uint32_t F>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kRetraceWpe<F>))) mrt_retrace_kernel(PathParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const LStack Ls = lds_stacks(WaveLds{P.lds_frames, P.lds_rays, P.lds_mesh, P.lds_save}, lds, lane);
    const LevStore<0> lev{nullptr, 0u, 0u, 0u};
    const DScene& S = P.sc;
    PhaseClock ph{};
    const uint32_t listed = __hip_atomic_load(P.rt.n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t n = min(listed, P.rt.cap);
    if (blockIdx.x == 0 && lane == 0 && n) atomicAdd(P.rt.total, (unsigned long long)n);
    if (blockIdx.x == 0 && lane == 0 && listed > n) atomicAdd(P.rt.lost, (unsigned long long)(listed - n));  // (kept fast)
    for (uint32_t i = blockIdx.x * 64u + lane; i < n; i += gridDim.x * 64u) {
        const uint32_t idx = P.rt.idx[i];
        uint32_t lp, sl;
        path_coords(P, idx, &lp, &sl);
        PathState ps;
        float u, v;
        path_key_at(P, lp, P.s0 + sl, ps.rng, &u, &v);
        ps.r = camera_ray(S, ps.rng, u, v);
        ps.depth = 0;
        ps.nlev = 0;
        ps.T = f3{1.0f, 1.0f, 1.0f};
        f3 L{0.0f, 0.0f, 0.0f};
        while (!trace_segment<F, 0>(S, ps, P.max_bounces, lev, Ls, &L, ph)) {
        }
        L = end_path(ps, lev, L);
        store_radiance(P.rad + (size_t)idx * 3u, L);
    }
    if (lane == 0 && atomicAdd(P.rt.done, 1u) == gridDim.x - 1u) {
        atomicExch(P.rt.n, 0u);  // every group has read the count: the list is empty for the next launch
        atomicExch(P.rt.done, 0u);
    }
}
#endif
template <uint32_t F>
static constexpr path_kernel_t kfn_retrace() {
#if MRT_TABLE_PEX
    if constexpr (kRetrace<F>) return mrt_retrace_kernel<F>;
#endif
    return nullptr;
}

template <uint32_t F>
static constexpr path_kernel_t kfn() {
#if MRT_TABLE_PEX
    if constexpr (!kPathExact<F>) return nullptr;  // (not instantiated: another build runs it)
    else
#elif MRT_TABLE_FTZ
    if constexpr (!kFtzVariant<F>) return nullptr;  // (not instantiated: the plain fast build runs it)
    else
#endif
    return MRT_PATH_KERNEL<F>;
}

// one entry per variant of mrt_launch.h's kVariants
template <size_t... I>
static KernelTable make_table(const char* numerics, std::index_sequence<I...>) {
    return KernelTable{numerics,
                       {kfn<kVariants[I]>()...},
                       {PathLevLds<kVariants[I]>::K...},
                       {TreeOf<kVariants[I]>::wg...},
                       {TreeOf<kVariants[I]>::on...},
                       {PathQ<kVariants[I]>::words...},
                       {kBox6Walk<kVariants[I]>...},
                       {(uint32_t)(kLinSlabOps<kVariants[I]> && MRT_SIG_OF(kVariants[I]) == SIG_NONE)...},
                       {kfn_retrace<kVariants[I]>()...}};
}
#if MRT_TABLE_PEX
const KernelTable& mrtd::kernel_table_fast_pex() {
    static const KernelTable t = make_table("fast", std::make_index_sequence<kNumVariants>{});
#elif MRT_TABLE_FTZ
const KernelTable& mrtd::kernel_table_fast_ftz() {
    static const KernelTable t = make_table("fast", std::make_index_sequence<kNumVariants>{});
#elif MRT_TABLE_FAST
const KernelTable& mrtd::kernel_table_fast() {
    static const KernelTable t = make_table("fast", std::make_index_sequence<kNumVariants>{});
#else
const KernelTable& mrtd::kernel_table_exact() {
    static const KernelTable t = make_table("exact", std::make_index_sequence<kNumVariants>{});
#endif
    return t;
}
