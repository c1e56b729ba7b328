// rl_relight.hip.h -- the kernels behind rl_relight_unit_*: a film that keeps photons by wavelength AND by the light a path ended on
// (n_groups * n_nodes planes of width x height floats, group-major then node-major), filled by one routed splat of traced camera
// samples.  The arithmetic of a photon is rl_spectral_photons_kernel's (rl_spectral.hip.h), operation for operation; what is new is
// where it lands: the cube of the group that a one-byte-per-object table gives the emitter in RlPathResult::object.  The mix of the
// cubes into a gather unit is rl_spectral_project_kernel itself on the composed (n_groups * n_nodes) x 3 matrix (rl_api.hip).
// Included by rl_api.hip after rl_spectral.hip.h; needs rl_core.h (rl_splat_weights) only: no scene, no CIE table, no ray kernel.
#pragma once

// The camera rays of samples [0, n) as the contiguous array the path kernel reads: one sample per lane, grid-stride.  A sample is
// three 16-byte words and its ray the first two (include/robigo_luculenta.h: RlCameraSample), so a lane moves two of them.
__global__ __launch_bounds__(RL_BLOCK) void rl_relight_rays_kernel(const RlCameraSample* __restrict__ samples, RlSpectralRay* __restrict__ rays,
                                                                    uint64_t n) {
    static_assert(sizeof(RlCameraSample) == 48 && sizeof(RlSpectralRay) == 32 && offsetof(RlCameraSample, ray) == 0, "a sample starts with its ray");
    const float4* in = reinterpret_cast<const float4*>(samples);
    float4* out = reinterpret_cast<float4*>(rays);
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const float4 a = in[3u * i], b = in[3u * i + 1u];
        out[2u * i] = a;
        out[2u * i + 1u] = b;
    }
}

// The routed splat of `n` traced samples: one sample per lane, grid-stride, the index 64 bits wide, no LDS.  Skipped: a zero value, a
// NaN or infinite x, y or wavelength (rl_spectral_photons_kernel's rules for the photon {x, y, value, wavelength}), an object that is
// not one of the table's n_objects (RL_OBJECT_NONE is such a value), and an object whose group is not one of the film's n_groups
// (RL_RELIGHT_DROP = 0xff is such a value: n_groups <= RL_RELIGHT_MAX_GROUPS = 16; the host only uploads tables whose other entries
// are below n_groups, and the comparison here keeps a lane inside the film whatever the table holds).  The table is read per lane,
// one byte, and only for an object below n_objects.  results[i].end and .segments are not read.
__global__ __launch_bounds__(RL_BLOCK) void rl_relight_splat_kernel(const RlCameraSample* __restrict__ samples, const RlPathResult* __restrict__ results,
                                                                     uint64_t n, const uint8_t* __restrict__ groups, uint32_t n_objects, uint32_t width,
                                                                     uint32_t height, uint32_t n_nodes, uint32_t n_groups, float spacing,
                                                                     float aspect_ratio, float* __restrict__ film) {
    const uint64_t n_pixels = (uint64_t)width * height;
    const float last = (float)(int)(n_nodes - 1u);
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const float value = results[i].value;
        const uint32_t object = results[i].object;
        if (value == 0.0f) continue;
        const float x = samples[i].x, y = samples[i].y, wavelength = samples[i].ray.wavelength;
        if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY)) continue;
        if (!(fabsf(wavelength) < INFINITY)) continue;
        if (object >= n_objects) continue;
        const uint32_t group = groups[object];
        if (group >= n_groups) continue;
        const float f = (wavelength - 380.0f) / spacing;
        const float fl = floorf(f);
        const float r = f - fl;
        const bool lo_in = fl >= 0.0f && fl <= last;          // node (int)fl
        const bool hi_in = fl >= -1.0f && fl <= last - 1.0f;  // node (int)fl + 1
        if (!(lo_in || hi_in)) continue;
        const int node = (int)fl; // -1 .. n_nodes - 1
        const float lo = value * (1.0f - r);
        const float hi = value * r;
        const RlSplat s = rl_splat_weights(width, height, aspect_ratio, x, y);
        float* cube = film + (uint64_t)(group * n_nodes) * n_pixels; // (group * n_nodes < 16 * 401)
        if (lo_in) {
            float* plane = cube + (uint64_t)node * n_pixels;
#pragma unroll
            for (int k = 0; k < 4; ++k) unsafeAtomicAdd(plane + s.idx[k], lo * s.w[k]);
        }
        if (hi_in) {
            float* plane = cube + (uint64_t)(node + 1) * n_pixels;
#pragma unroll
            for (int k = 0; k < 4; ++k) unsafeAtomicAdd(plane + s.idx[k], hi * s.w[k]);
        }
    }
}
