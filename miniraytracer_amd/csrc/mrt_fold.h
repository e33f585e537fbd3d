// mrt_fold.h -- the fold unit (mrt_fold.hip) as the render sees it: host functions that enqueue the
// fold of a launch chunk and the final kernel.  The kernels, their grids and their tuning macros stay
// inside mrt_fold.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mrt.h"

// The render's last chunk (out != null) also finishes the pixels -- final_pixel into the caller's
// output -- and resets the counters (FoldEnd), so no separate final kernel follows it.
struct FoldEnd {
    float4* out;                     // the render's output (last chunk), or null: keep folding into acc
    uint32_t ns;                     // samples per pixel (mode 0 divides by it)
    unsigned long long* counters;    // work counters of the render's launches (MRT_COUNTER_STRIDE apart)
    unsigned long long* hprog;       // their progress snapshots in host memory (or null)
    uint32_t nreset;                 // counter slots to reset (MRT_CNT_SLOTS per launch)
    uint32_t nprog;                  // progress snapshots to reset (MRT_NPART per launch)
};

enum class FoldShape {
    Full,       // mrt_fold_kernel: a thread per pixel
    Lean,       // mrt_fold_lean_kernel (mode 0 only; takes no FoldEnd: a final kernel follows the render)
    Async,      // mrt_fold_async_kernel<false>: the full grid, a 256-thread group per CU (`groups`: the CUs)
    AsyncSide,  // mrt_fold_async_kernel<true>: `groups` one-wave groups, the side slots of the launch
};

// the fold of samples [s0, s1) of a chunk's radiance into acc (or, fe.out set, finished into it) on `q`
__attribute__((visibility("hidden"))) mrt_status mrt_fold_enqueue(FoldShape shape, uint32_t groups, const float* rad, float4* acc, uint32_t npix, uint32_t s0, uint32_t s1,
                            uint32_t mode, float max_lum, const FoldEnd& fe, hipStream_t q);
// mrt_final_kernel: acc finished into out after ns samples; resets nreset counter slots and nprog snapshots
__attribute__((visibility("hidden"))) mrt_status mrt_final_enqueue(const float4* acc, float4* out, uint32_t npix, uint32_t ns, uint32_t mode, float max_lum,
                             unsigned long long* counters, unsigned long long* hprog, uint32_t nreset, uint32_t nprog, hipStream_t q);
