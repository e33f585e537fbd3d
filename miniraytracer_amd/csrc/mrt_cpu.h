// mrt_cpu.h -- the CPU backend (mrt_cpu.hip) as seen from the C-ABI entry points (mrt_render.hip, mrt_upload.hip, mrt_query.hip):
// a scene uploaded to MRT_DEVICE_CPU carries one of these instead of device tables.
#pragma once
#include "../../include/mrt.h"

struct mrt_cpu_scene;
mrt_status mrt_cpu_scene_create(const mrt_scene_view* v, mrt_cpu_scene** out);
void mrt_cpu_scene_free(mrt_cpu_scene* c);
uint32_t mrt_cpu_scene_features(const mrt_cpu_scene* c);
// mrt_scene_set_camera: later renders and feature buffers start their paths from *cam
void mrt_cpu_set_camera(mrt_cpu_scene* c, const mrt_camera* cam);
mrt_status mrt_cpu_render(mrt_cpu_scene* c, const mrt_render_desc* d, float* rgb_out, uint64_t* rays_out, const volatile int* cancel);
// first-hit feature buffers (mrt_render_aux): host W*H*4 each, owned pixels only
mrt_status mrt_cpu_render_aux(mrt_cpu_scene* c, const mrt_render_desc* d, float* normal_out, float* albedo_out);
// ray queries (mrt_cast_rays; arguments checked by the caller): host records
mrt_status mrt_cpu_cast_rays(mrt_cpu_scene* c, const mrt_ray* rays, uint32_t n, uint64_t seed, mrt_hit* hits);
// radiance queries (mrt_trace_rays; arguments checked by the caller): host records.  The host-only
// helpers of that section (mrt_probe_seed, mrt_camera_path_probe, mrt_pano_probe) are defined beside
// it, where the camera's arithmetic is compiled for the host.
mrt_status mrt_cpu_trace_rays(mrt_cpu_scene* c, const mrt_probe* probes, uint32_t n, uint32_t max_bounces, mrt_radiance* out);
// the adaptive render (mrt_render_adaptive; arguments checked by the caller)
mrt_status mrt_cpu_render_adaptive(mrt_cpu_scene* c, const mrt_render_desc* d, const mrt_adaptive_params* p, float* rgb_out, float* moments_out,
                                   uint64_t* rays_out, const volatile int* cancel);
mrt_status mrt_cpu_progress(mrt_cpu_scene* c, float* pct);
mrt_status mrt_cpu_last_ms(mrt_cpu_scene* c, float* ms, uint32_t* threads);
mrt_status mrt_cpu_preview(mrt_cpu_scene* c, float* rgb_out, uint32_t* samples_done);
mrt_status mrt_cpu_set_worker_seeds(mrt_cpu_scene* c, uint32_t n, const uint64_t* initstate, const uint64_t* initseq);
