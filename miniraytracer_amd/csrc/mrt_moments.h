// mrt_moments.h -- what the adaptive render's two drivers (mrt_render.hip for the GPU, mrt_cpu.hip
// for the CPU backend) share, behind include/mrt.h "sample moments and the adaptive render".
#pragma once
#include <vector>
#include "mrt_internal.h"

// mrt_render_adaptive's arguments: what both backends accept
mrt_status mrt_internal_adaptive_check(const void* scene, const mrt_render_desc* d, const mrt_adaptive_params* p, const void* rgb_out);
// the desc of refinement pass k >= 1 over `pixels`: d on a grid 2^k times as fine, its own seed
// (mrt_cpu.hip: the path streams' splitmix64)
mrt_render_desc mrt_internal_adaptive_pass(const mrt_render_desc* d, uint32_t k, const uint32_t* pixels, uint32_t n_pixels);
// the slots i < n whose moments (n float4) refine, ascending: mrt_moments_refine of
// include/mrt_adaptive.h, compiled once (mrt_adaptive.hip) for both backends
std::vector<uint32_t> mrt_internal_refine_slots(const float* moments, uint32_t n, float atol, float rtol);

// GPU: enqueue on `stream` (a hipStream_t) without synchronising or allocating
// mrt_moments_kernel: a radiance chunk [s][local pixel] float3 into moments[slots ? slots[lp] : lp]
mrt_status mrt_internal_moments_enqueue(const float* d_rad, uint32_t n_pixels, uint32_t n_samples, const uint32_t* d_slots, float* d_moments,
                                        void* stream);
// mrt_merge_kernel: pass pixels c[j], j < n, into the running colour C[slots[j]] over N samples
mrt_status mrt_internal_merge_enqueue(const float* d_c, uint32_t n, const uint32_t* d_slots, float* d_C, float N, float nsf, void* stream);
