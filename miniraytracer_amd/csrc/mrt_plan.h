// mrt_plan.h -- the arithmetic of a render's launches as pure host functions: the launch chunk, the
// work partitions and tail zone of one launch, the counter-slot sets.  No HIP runtime call: mrt_prepare
// and mrt_render_device (mrt_render.hip) call these, and so does tools/claim_check.cpp without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/mrt.h"
#include "mrt_launch.h"

namespace mrtd {

inline uint32_t auto_chunk(uint32_t npix, uint32_t ns) {
    // keep the per-chunk radiance buffer within ~4 GiB of HBM (288 GB per MI355X)
    const size_t budget = (size_t)4 << 30;
    size_t per_sample = (size_t)npix * 12;
    size_t c = per_sample ? budget / per_sample : ns;
    if (c < 1) c = 1;
    return (uint32_t)std::min<size_t>(c, ns);
}

// samples per launch of a render of ns samples over npix local pixels (the zero return, which mrt_prepare
// reports as an image too large for one launch, is kept from the clamps' first form: they now end at >= 1)
inline uint32_t plan_chunk(uint32_t npix, uint32_t ns, uint32_t chunk_samples, uint32_t flags) {
    uint32_t chunk = chunk_samples ? std::min(chunk_samples, ns) : auto_chunk(npix, ns);
    chunk = (uint32_t)std::min<uint64_t>(chunk, 0xFFFFFFFFull / std::max<uint32_t>(npix, 1));  // 32-bit path index
    // 32-bit byte offsets of the chunk's radiance (the path kernel's held store, mrt_kernels.hip)
    chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, 0xFFFFFFFFull / (12ull * std::max<uint32_t>(npix, 1))));
    if (chunk == 0) return 0;
    if (flags & MRT_RF_PATH_DEBUG) chunk = ns;  // debug keeps every path
    return chunk;
}

// what of PathParams follows from a launch's path count: a launch of n_paths paths by `grid` groups of
// `waves` waves each
inline void plan_partitions(PathParams& P, uint32_t n_paths, int grid, uint32_t waves) {
    P.n_paths = n_paths;
    P.tail_zone = (uint32_t)std::min<uint64_t>((uint64_t)grid * waves * 2 * MRT_BATCH, P.n_paths);  // ~2 big claims per wave
    P.static_first = (uint64_t)P.n_paths < (uint64_t)grid * waves * MRT_BATCH * 64u;
    // MRT_NPART contiguous work partitions, one counter each; the waves of partition k (workgroups
    // b with b % MRT_NPART == k) take its first batches statically when P.static_first
    for (uint32_t k = 0; k <= MRT_NPART; k++) P.part_base[k] = (uint64_t)P.n_paths * k / MRT_NPART;
    for (uint32_t k = 0; k < MRT_NPART; k++) {
        const uint64_t waves_k = (uint64_t)((grid - k + MRT_NPART - 1) / MRT_NPART) * waves;
        P.part_dyn[k] = P.part_base[k] + (P.static_first ? waves_k * MRT_BATCH : 0);
    }
}

// Two sets of counter slots / progress snapshots, `half` launches each, at FIXED offsets 0 and half:
// consecutive MRT_RF_FOLD_ASYNC renders alternate between them, because a render's last fold still
// resets its set while the next render's kernels count in the other.  The stride must not follow each
// render's own launch count: a render of 1 launch after one of 4 would otherwise start its set inside
// the previous render's (whose reset then lands mid-claim).  The set is grown only after quiesce() (no
// render pending), and render R+2 -- the next user of R's set -- waits for R's last fold (its first
// launch waits for the fold of the same radiance parity, and folds run in order on the context's stream).
struct SlotPlan {
    uint32_t need, half, launches;  // the render's launches; launch slots per set; of both sets
};
inline SlotPlan plan_slots(uint32_t ns, uint32_t chunk, uint32_t slot_half) {
    const uint32_t need = (ns + chunk - 1) / chunk;
    const uint32_t half = std::max(slot_half, need);
    return SlotPlan{need, half, 2 * half};
}

}  // namespace mrtd
