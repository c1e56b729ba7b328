// rl_light_film.hip.h -- the kernels behind rl_plot_unit_light_paths* and rl_plot_unit_render_samples_direct*: the light kernel
// with a film.  What rl_light_kernel writes into a sample record this one splats where the value is produced, and it splats the
// value of a path that has just ended on a light unless the sample at the vertex before has already estimated it (the header's
// "counting light once").  The body and the launch's block are rl_light.hip.h's (rl_light_body<STAGE, CYL, true>,
// RlLightFilmQueue).  Included by rl_api.hip after rl_light.hip.h and rl_step.hip.h (rl_store_begun_state).
#pragma once

template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_light_film_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    rl_light_body<STAGE, CYL, true>(scene, lay, queue);
}

// ---- the two ends of rl_plot_unit_render_samples_direct*'s loop (grid-stride, one record per lane) ----

// rl_begin_paths_kernel for the rays of camera samples (48-byte records), which also clears the states' `sampled` bytes.
__global__ __launch_bounds__(RL_BLOCK) void rl_direct_begin_kernel(const RlCameraSample* __restrict__ camera, uint64_t first_path,
                                                                   RlPathState* __restrict__ states, uint8_t* __restrict__ sampled, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlF4* in = (const RlF4*)(camera + i);
        const RlF4 r0 = in[0], r1 = in[1];
        rl_store_begun_state(states + i, r0, r1, first_path + i);
        sampled[i] = 0;
    }
}

// What rl_ray_paths_kernel writes for a path, from the state the loop left: a state that is still live used up max_segments.
__global__ __launch_bounds__(RL_BLOCK) void rl_direct_results_kernel(const RlPathState* __restrict__ states, RlPathResult* __restrict__ results,
                                                                     uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlF4* rec = (const RlF4*)(states + i);
        const RlF4 q2 = rec[2];
        const uint32_t end = rl_f2u(q2.z);
        const bool live = end == RL_PATH_LIVE;
        results[i] = rl_path_result(live ? 0.0f : q2.w, rl_f2u(q2.y), live ? RL_OBJECT_NONE : rl_f2u(rec[3].z), live ? (uint32_t)RL_PATH_END_LIMIT : end);
    }
}
