// rl_film.hip.h -- the film behind rl_plot_unit_plot_photons* and rl_plot_unit_render_samples*: PlotUnit::plot
// (plot_unit.rs:87-95) for photons a caller holds, and what the path kernel with a film (rl_paths.hip.h: rl_film_paths_kernel)
// splats with at the point where a path ends.  Included by rl_api.hip after rl_kernels.hip.h and before rl_paths.hip.h.
#pragma once

// Where the film path kernel splats: a plot unit's buffer and the launch constants of rl_splat_weights.  The host writes it
// behind the launch's queue counter (RlFilmQueue) instead of passing it as kernel arguments: seven more scalar registers held
// across the persistent loop spilled (40 spilled SGPRs against the path kernel's 29), while the lanes that end with a value can
// load the block where they use it.
struct RlFilm {
    float* plot;
    uint32_t width, height;
    float wm1, hm1; // (float)width - 1, (float)height - 1 (plot_unit.rs:60-61)
    float aspect_ratio;
    uint32_t off_cie; // RlSceneLayout::off_cie: the splat finds the CIE table from it rather than hold sv.cie across the loop
};
struct RlFilmQueue {
    unsigned long long next; // the path kernel's queue counter: zero at launch
    RlFilm film;
};

// plot_pixel (plot_unit.rs:56-84) of one photon: the arithmetic and the f32 atomics of rl_plot_kernel.
__device__ __forceinline__ void rl_film_splat(float* __restrict__ plot, const RlF3 c, const RlSplat& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float* px = plot + 3ull * s.idx[k];
        unsafeAtomicAdd(px + 0, c.x * s.w[k]);
        unsafeAtomicAdd(px + 1, c.y * s.w[k]);
        unsafeAtomicAdd(px + 2, c.z * s.w[k]);
    }
}

// PlotUnit::plot for `n` photons of the caller's: one photon per lane, grid-stride, the CIE table in LDS.  rl_plot_kernel with two
// differences: a photon whose x or y is NaN or infinite is skipped (include/robigo_luculenta.h), and the index is 64 bits wide.
// Every other photon lands on four pixels inside the buffer whatever its fields hold: rl_splat_weights clamps the pixel
// coordinates after the conversion to int, which saturates on the device (a NaN product converts to 0).
__global__ __launch_bounds__(RL_BLOCK) void rl_film_photons_kernel(const RlMappedPhoton* __restrict__ photons, uint64_t n,
                                                                   const RlF4* __restrict__ cie, uint32_t width, uint32_t height,
                                                                   float aspect_ratio, float* __restrict__ plot) {
    __shared__ RlF4 s_cie[RL_CIE_SAMPLES];
    for (uint32_t i = threadIdx.x; i < RL_CIE_SAMPLES; i += RL_BLOCK) s_cie[i] = cie[i];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlMappedPhoton ph = photons[i];
        if (ph.probability == 0.0f) continue;
        if (!(fabsf(ph.x) < INFINITY && fabsf(ph.y) < INFINITY)) continue;
        const RlF3 c = rl_mul(rl_tristimulus(s_cie, ph.wavelength), ph.probability);
        rl_film_splat(plot, c, rl_splat_weights(width, height, aspect_ratio, ph.x, ph.y));
    }
}
