// rl_adaptive.hip.h -- the device code behind rl_adaptive_unit_samples* and rl_plot_unit_render_adaptive: camera samples drawn tile by
// tile from a plan (rl_adaptive_plan.h), and the splat of what the unchanged path kernel (rl_paths.hip.h: rl_ray_paths_kernel) made of
// them, each with its tile's weight.  Two pointwise kernels around that launch; no ray kernel here.  The arithmetic is the contract
// stated in include/robigo_luculenta.h: f32 in the stated order, no contraction, the correctly rounded divide.  The per-sample
// functions are RL_HD so that tests/adaptive_host can compile them with g++; the product never runs them on the CPU.
// Included by rl_api.hip after rl_film.hip.h (rl_film_splat); needs rl_core.h (rl_camera_path, rl_splat_weights) and the public
// header (RlCameraSample, RlPathResult).
#pragma once
#include "rl_adaptive_plan.h"

// The tile of sample j of a plan: the t with off[t] <= j < off[t + 1].  off[0] = 0, off[n_tiles] = the plan's n_paths > j, and the
// offsets grow strictly (every tile has a sample), so the search ends on the one such t: ceil(log2(n_tiles)) steps, 13 at 1920 x 1080.
// A plain per-lane binary search.  A wave's 64 consecutive samples span few tiles, so a wave-uniform search for the first and the
// last of them would shorten it; that form was not built and neither was measured: the kernel is bound by its 80 bytes of stores
// and the camera's arithmetic, and the offsets of a film stay in cache.
RL_HD uint32_t rl_adaptive_tile_of(const uint32_t* off, uint32_t n_tiles, uint32_t j) {
    uint32_t lo = 0u, hi = n_tiles;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A screen coordinate in [-1, 1] from the unit draw u over the cell [lo, hi] of an axis whose last pixel is m1 = size - 1: the
// inverse of plot_pixel's px = (x * 0.5 + 0.5) * m1 (plot_unit.rs:60-61), up to rounding.
RL_HD float rl_adaptive_screen(float lo, float hi, float u, float m1) {
    const float p = lo + (hi - lo) * u;
    return (p / m1 - 0.5f) * 2.0f;
}

// The draws of sample `path` of a plan in the cell `cell`: rl_begin_path's from block 0, word for word -- the wavelength from w[0],
// the camera time from w[3] -- and the screen position from w[1], w[2] inside the cell.
struct RlAdaptiveDraw {
    float x, y, t, wavelength;
};
RL_HD RlAdaptiveDraw rl_adaptive_draw(float wm1, float hm1, float aspect_ratio, const RlAdaptiveCell cell, uint64_t seed, uint32_t stream,
                                      uint64_t path) {
    const RlRngBlock b0 = rl_rng_block(seed, stream, path, 0);
    RlAdaptiveDraw d;
    d.wavelength = rl_get_wavelength(b0.w[0]);
    d.x = rl_adaptive_screen(cell.x_lo, cell.x_hi, rl_get_unit(b0.w[1]), wm1);
    d.y = rl_adaptive_screen(cell.y_lo, cell.y_hi, rl_get_unit(b0.w[2]), hm1) / aspect_ratio;
    d.t = rl_get_unit(b0.w[3]);
    return d;
}
// The ray of a draw: rl_begin_path's camera, which draws the lens from block 1 of the path.
RL_HD RlSpectralRay rl_adaptive_ray(const RlSceneView& sv, const RlAdaptiveDraw d, uint64_t seed, uint32_t stream, uint64_t path) {
    RlPath p;
    rl_camera_path(sv, d.x, d.y, d.t, d.wavelength, seed, stream, path, &p);
    RlSpectralRay r;
    r.origin = RlVector3{p.origin.x, p.origin.y, p.origin.z};
    r.wavelength = p.wavelength;
    r.direction = RlVector3{p.direction.x, p.direction.y, p.direction.z};
    r.reserved = 0u;
    return r;
}

#if defined(__HIPCC__)
// The device's view of a plan and of the film it is for: what rl_adaptive_unit_plan uploaded.
struct RlAdaptivePlan {
    const uint32_t* off;         // n_tiles + 1 exclusive prefix sums of the counts
    const RlAdaptiveCell* cells; // n_tiles
    const uint32_t* weight_bits; // n_tiles: the bits of w_t
    uint32_t n_tiles;
    float wm1, hm1, aspect_ratio; // (float)width - 1, (float)height - 1, width / height as rl_splat_weights takes them
};

// Kernel one: samples first_sample .. first_sample + n - 1 of the plan as paths first_path + first_sample + i, one per lane,
// grid-stride as rl_camera_rays_kernel.  samples[i] is the record; rays, if given, is the same ray
// again as a contiguous array, which is what the path kernel reads.  No LDS.  The register cap: the kernel runs beside a resident
// open trace kernel, four of whose waves per SIMD leave 32 VGPRs (rl_error.hip.h).  Only the scene's camera record is read.
__global__ __launch_bounds__(RL_BLOCK) __attribute__((amdgpu_num_vgpr(32))) void rl_adaptive_samples_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, RlAdaptivePlan plan, uint64_t seed, uint32_t stream, uint64_t first_path,
    uint32_t first_sample, RlCameraSample* __restrict__ samples, RlSpectralRay* __restrict__ rays, uint32_t n) {
    RlSceneView sv = {};
    sv.camera_rec = scene + lay.off_camera;
    // (a 32-bit index, left by the guard where the grid's stride would wrap it past 2^32: a wrapped lane would start over.  The
    // 64-bit form of rl_camera_rays_kernel costs the register that puts this kernel over its cap.)
    const uint32_t stride = gridDim.x * RL_BLOCK;
    for (uint32_t i = blockIdx.x * RL_BLOCK + threadIdx.x; i < n;) {
        const uint32_t j = first_sample + i; // (< the plan's n_paths <= 2^32 - 1: the host checks the range)
        const uint32_t tile = rl_adaptive_tile_of(plan.off, plan.n_tiles, j);
        const uint64_t path = first_path + j;
        const RlAdaptiveDraw d = rl_adaptive_draw(plan.wm1, plan.hm1, plan.aspect_ratio, plan.cells[tile], seed, stream, path);
        // (the record's second half first: the tile and its weight are not held across the camera's arithmetic)
        *(uint4*)&samples[i].x = make_uint4(rl_f2u(d.x), rl_f2u(d.y), tile, plan.weight_bits[tile]);
        uint32_t k = i;
        asm volatile("" : "+v"(k)); // (opaque: the record's address is made again behind the camera, not held across it)
        const RlSpectralRay r = rl_adaptive_ray(sv, d, seed, stream, first_path + (first_sample + k));
        samples[k].ray = r;
        if (rays) rays[k] = r;
        if (k + stride < k) break;
        i = k + stride;
    }
}

// Kernel two: rl_film_photons_kernel reading two arrays.  Where a path ended with a value and its sample's position is finite,
// get_tristimulus(wavelength) * (value * w_t) goes onto the four pixels of plot_pixel(x, y): one f32 multiply of value and weight,
// then the film's arithmetic (rl_splat_weights, rl_film_splat).  Per sample 16 of the record's 48 bytes and the result's value are
// read; the CIE table is read from global memory where the photon kernel keeps it in LDS: the open trace kernel leaves none.
__global__ __launch_bounds__(RL_BLOCK) __attribute__((amdgpu_num_vgpr(32))) void rl_adaptive_splat_kernel(
    const RlCameraSample* __restrict__ samples, const RlPathResult* __restrict__ results, uint64_t n, const RlF4* __restrict__ cie,
    uint32_t width, uint32_t height, float aspect_ratio, float* __restrict__ plot) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const float value = results[i].value;
        if (value == 0.0f) continue;
        const float x = samples[i].x, y = samples[i].y;
        if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY)) continue;
        const float weighted = value * rl_u2f(samples[i].reserved1);
        const RlF3 c = rl_mul(rl_tristimulus(cie, samples[i].ray.wavelength), weighted);
        rl_film_splat(plot, c, rl_splat_weights(width, height, aspect_ratio, x, y));
    }
}
#endif
