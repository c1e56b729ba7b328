// rl_spectral.hip.h -- the kernels behind rl_spectral_unit_*: a film that keeps photons by wavelength (n_nodes planes of
// width x height floats, node-major) and its projection into a gather unit under a caller's n_nodes x 3 matrix.  The arithmetic is
// the contract stated in include/robigo_luculenta.h: f32, in the stated order, no contraction; add, multiply, floorf and the
// correctly rounded divide only, so the CPU restatement (tests/_spectral_oracle.py) holds the projection bit for bit and the film
// up to the order of its atomics.  Included by rl_api.hip after rl_film.hip.h; needs rl_core.h (rl_splat_weights) only: no scene, no
// CIE table, no ray kernel.
#pragma once

// The splat of `n` photons: one photon per lane, grid-stride, the index 64 bits wide.  rl_film_photons_kernel's rules (a zero
// probability, a NaN or infinite x or y: skipped) and one more: a NaN or infinite wavelength is skipped.  Whether a node is in the
// film is decided on fl as a float, so (int)fl is only evaluated for -1 <= fl <= n_nodes - 1.  Every other photon lands on four
// pixels inside each of at most two planes whatever its fields hold (rl_splat_weights clamps the pixel coordinates).
//   The film is planar: the two pixels of a row share a cache line in each plane, so a photon touches at most four lines per node
//   as the XYZ film does per photon, with eight atomics against its twelve; a wave's atomics fall wherever its photons do (the
//   float atomics execute at the memory side: nothing of the 81 planes has to stay in L2).
__global__ __launch_bounds__(RL_BLOCK) void rl_spectral_photons_kernel(const RlMappedPhoton* __restrict__ photons, uint64_t n, uint32_t width,
                                                                       uint32_t height, uint32_t n_nodes, float spacing, float aspect_ratio,
                                                                       float* __restrict__ film) {
    const uint64_t n_pixels = (uint64_t)width * height;
    const float last = (float)(int)(n_nodes - 1u);
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlMappedPhoton ph = photons[i];
        if (ph.probability == 0.0f) continue;
        if (!(fabsf(ph.x) < INFINITY && fabsf(ph.y) < INFINITY)) continue;
        if (!(fabsf(ph.wavelength) < INFINITY)) continue;
        const float f = (ph.wavelength - 380.0f) / spacing;
        const float fl = floorf(f);
        const float r = f - fl;
        const bool lo_in = fl >= 0.0f && fl <= last;          // node (int)fl
        const bool hi_in = fl >= -1.0f && fl <= last - 1.0f;  // node (int)fl + 1
        if (!(lo_in || hi_in)) continue;
        const int node = (int)fl; // -1 .. n_nodes - 1
        const float lo = ph.probability * (1.0f - r);
        const float hi = ph.probability * r;
        const RlSplat s = rl_splat_weights(width, height, aspect_ratio, ph.x, ph.y);
        if (lo_in) {
            float* plane = film + (uint64_t)node * n_pixels;
#pragma unroll
            for (int k = 0; k < 4; ++k) unsafeAtomicAdd(plane + s.idx[k], lo * s.w[k]);
        }
        if (hi_in) {
            float* plane = film + (uint64_t)(node + 1) * n_pixels;
#pragma unroll
            for (int k = 0; k < 4; ++k) unsafeAtomicAdd(plane + s.idx[k], hi * s.w[k]);
        }
    }
}

// The projection: one pixel per lane, the node loop in order with a separate multiply and add per component.  The matrix is read
// through wave-uniform loads (every lane of a launch reads the same n_nodes x 3 floats: they come through the scalar cache), so the
// kernel has no LDS and a lane's only vector traffic is its n_nodes film values, one coalesced dword per plane, and its three
// results.  dst is a gather unit's tristimulus buffer: width x height x 3 floats.
__global__ __launch_bounds__(RL_BLOCK) void rl_spectral_project_kernel(const float* __restrict__ film, const float* __restrict__ matrix,
                                                                       uint64_t n_pixels, uint32_t n_nodes, float* __restrict__ dst) {
    for (uint64_t p = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; p < n_pixels; p += (uint64_t)gridDim.x * RL_BLOCK) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        const float* column = film + p;
#pragma unroll 8
        for (uint32_t b = 0; b < n_nodes; ++b) {
            const float v = column[(uint64_t)b * n_pixels];
            x = x + matrix[3u * b] * v;
            y = y + matrix[3u * b + 1u] * v;
            z = z + matrix[3u * b + 2u] * v;
        }
        dst[p * 3u] = x;
        dst[p * 3u + 1u] = y;
        dst[p * 3u + 2u] = z;
    }
}
