// rl_denoise.hip.h -- the kernels behind rl_denoise_unit_denoise: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010)
// over a gather unit's tristimulus buffer, guided by the films of rl_scene_render_features.  The arithmetic is the contract stated
// in include/robigo_luculenta.h: f32, in the stated order, no contraction; add, multiply, the correctly rounded divide, rl_sqrtf and
// rl_expf only, so the CPU restatement (tests/_denoise_oracle.py) is held bit for bit.  Included by rl_api.hip; needs rl_math.h and
// rl_core.h (RlF4) only: no scene, no ray kernel.
#pragma once

static_assert(sizeof(RlF4) == 16 && alignof(RlF4) == 16, "the guide record and the LDS tile are read in 16-byte words");

// The guide record of a pixel, two 16-byte words: {n.xyz, z} and {a.xyz, live}.  live is 1.0f or 0.0f.
#define RL_DENOISE_GUIDE_WORDS 2

// One launch per call: the record of every pixel from the three guide films (any of them null: aux acts as (1, 0, 0), the others as
// zeros).  Films are width x height x 3 floats, as a gather unit holds them.
__global__ __launch_bounds__(RL_BLOCK) void rl_denoise_guides_kernel(const float* __restrict__ albedo, const float* __restrict__ normal,
                                                                     const float* __restrict__ aux, uint32_t n_pixels, RlF4* __restrict__ guides) {
    for (uint32_t p = blockIdx.x * RL_BLOCK + threadIdx.x; p < n_pixels; p += gridDim.x * RL_BLOCK) {
        const size_t o = (size_t)p * 3;
        const float wgt = aux ? aux[o] : 1.0f;
        const float depth = aux ? aux[o + 1] : 0.0f;
        const bool live = wgt > 0.0f;
        const float z = live ? depth / wgt : 0.0f;
        RlF3 a = rl_f3(0.0f, 0.0f, 0.0f), n = rl_f3(0.0f, 0.0f, 0.0f);
        if (albedo && live) a = rl_f3(albedo[o] / wgt, albedo[o + 1] / wgt, albedo[o + 2] / wgt);
        if (normal) {
            const float nx = normal[o], ny = normal[o + 1], nz = normal[o + 2];
            const float l2 = (nx * nx + ny * ny) + nz * nz;
            const float len = rl_sqrtf(l2);
            if (len > 0.0f) n = rl_f3(nx / len, ny / len, nz / len);
        }
        guides[(size_t)p * RL_DENOISE_GUIDE_WORDS] = RlF4{n.x, n.y, n.z, z};
        guides[(size_t)p * RL_DENOISE_GUIDE_WORDS + 1] = RlF4{a.x, a.y, a.z, live ? 1.0f : 0.0f};
    }
}

// What a pass reads beside the buffers.  kc is kc_i, the colour constant of this pass.
struct RlDenoisePass {
    uint32_t width, height;
    uint32_t step;         // s = 1 << i
    uint32_t classes_x;    // min(s, width): the residue classes mod s that have a pixel, per axis
    uint32_t classes_y;
    uint32_t tiles_x;      // lattice tiles per residue class and axis: ceil(ceil(width / s) / 16)
    uint32_t tiles_y;
    float kc, kn, kz, ka;
};

// The weight of tap q for centre p and its three products, added to the sums: the per-tap table of the contract, in its order.
// cp, cq: C_i of p and q; np, nq: {n.xyz, z}; ap, aq: {a.xyz, live}; hh: h[dy + 2] * h[dx + 2].
__device__ __forceinline__ void rl_denoise_tap(const RlDenoisePass& job, RlF3 cp, RlF4 np, RlF4 ap, RlF3 cq, RlF4 nq, RlF4 aq, float hh,
                                               float* sum_w, RlF3* sum_c) {
    const float m = fabsf(cp.y) + fabsf(cq.y);
    const float r = m > 0.0f ? (cp.y - cq.y) / m : 0.0f;
    const float e_c = r * r;
    const float dx = np.x - nq.x, dy = np.y - nq.y, dz = np.z - nq.z;
    const float e_n = (dx * dx + dy * dy) + dz * dz;
    const float mz = np.w > nq.w ? np.w : nq.w;
    const float rz = mz > 0.0f ? (np.w - nq.w) / mz : 0.0f;
    const float e_z = rz * rz;
    const float ax = ap.x - aq.x, ay = ap.y - aq.y, az = ap.z - aq.z;
    const float e_a = (ax * ax + ay * ay) + az * az;
    const float x = ((e_c * job.kc + e_n * job.kn) + e_z * job.kz) + e_a * job.ka;
    const float wt = hh * rl_expf(-x);
    *sum_w += wt;
    sum_c->x += wt * cq.x;
    sum_c->y += wt * cq.y;
    sum_c->z += wt * cq.z;
}

// The taps of a pixel lie on the lattice of stride s through it, so a workgroup takes a 16 x 16 LATTICE tile -- the pixels
// (rx + s (16 tx + i), ry + s (16 ty + j)) of one residue class (rx, ry) mod s -- and stages the 20 x 20 lattice neighbourhood in
// LDS: C_i with the live flag in its fourth component (clear for an element outside the image, so the tap loop has one test), and
// the two guide words.  The tile does not depend on s: one kernel serves every pass.
//   LDS layout.  Three arrays of 16-byte words, one per word of the element, rows of RL_DENOISE_PITCH words.  A ds_read_b128
//   serves a wave in four groups of 16 lanes that each span two tile rows (lanes 0-3, 12-15 of one and 4-11 of the next), and
//   its banks are (address / 4) mod 64: 16 words.  With the 20-word rows of the neighbourhood the second row's lanes land 4 words
//   into the first row's (20 mod 16), a two-way conflict on a quarter of the lanes; a pitch that is a multiple of 16 words puts
//   lane lx of either row on word (lx + const) mod 16: conflict-free.  32 is the smallest such pitch that holds 20.
//   Measured against the same loop reading every tap from global memory (profiles/denoise_bench.txt): the
//   tile wins at s = 1, 2, 4 and draws at s = 8, 16, where its staging loads are strided; it is kept for every step.
#define RL_DENOISE_TILE 16
#define RL_DENOISE_HALO 2
#define RL_DENOISE_SPAN (RL_DENOISE_TILE + 2 * RL_DENOISE_HALO)
#define RL_DENOISE_PITCH 32
#define RL_DENOISE_LDS_WORDS (RL_DENOISE_SPAN * RL_DENOISE_PITCH)

__global__ __launch_bounds__(RL_DENOISE_TILE * RL_DENOISE_TILE) void rl_denoise_pass_kernel(const float* __restrict__ in, const RlF4* __restrict__ guides,
                                                                                          RlDenoisePass job, float* __restrict__ out) {
    __shared__ RlF4 s_c[RL_DENOISE_LDS_WORDS], s_n[RL_DENOISE_LDS_WORDS], s_a[RL_DENOISE_LDS_WORDS];
    // the workgroup's residue class and tile: blockIdx.x = ((ry * tiles_y + ty) * classes_x + rx) * tiles_x + tx
    uint32_t b = blockIdx.x;
    const uint32_t tx = b % job.tiles_x;
    b /= job.tiles_x;
    const uint32_t rx = b % job.classes_x;
    b /= job.classes_x;
    const uint32_t ty = b % job.tiles_y;
    const uint32_t ry = b / job.tiles_y;
    const int s = (int)job.step;
    // lattice coordinates of the neighbourhood's corner; pixel = residue + s * lattice
    const long long lx0 = (long long)tx * RL_DENOISE_TILE - RL_DENOISE_HALO, ly0 = (long long)ty * RL_DENOISE_TILE - RL_DENOISE_HALO;
    for (uint32_t e = threadIdx.x; e < RL_DENOISE_SPAN * RL_DENOISE_SPAN; e += RL_DENOISE_TILE * RL_DENOISE_TILE) {
        const uint32_t u = e % RL_DENOISE_SPAN, v = e / RL_DENOISE_SPAN;
        // (64-bit: s * lattice stays far below 2^63 for any image the units accept, and a pixel past the edge must not wrap)
        const long long px = (long long)rx + s * (lx0 + u), py = (long long)ry + s * (ly0 + v);
        RlF4 c = RlF4{0.0f, 0.0f, 0.0f, 0.0f}, gn = c, ga = c;
        if (px >= 0 && px < (long long)job.width && py >= 0 && py < (long long)job.height) {
            const size_t p = (size_t)py * job.width + (size_t)px;
            gn = guides[p * RL_DENOISE_GUIDE_WORDS];
            ga = guides[p * RL_DENOISE_GUIDE_WORDS + 1];
            c = RlF4{in[p * 3], in[p * 3 + 1], in[p * 3 + 2], ga.w};
        }
        s_c[v * RL_DENOISE_PITCH + u] = c;
        s_n[v * RL_DENOISE_PITCH + u] = gn;
        s_a[v * RL_DENOISE_PITCH + u] = ga;
    }
    __syncthreads();
    const uint32_t i = threadIdx.x % RL_DENOISE_TILE, j = threadIdx.x / RL_DENOISE_TILE;
    const long long px = (long long)rx + s * (lx0 + RL_DENOISE_HALO + i), py = (long long)ry + s * (ly0 + RL_DENOISE_HALO + j);
    if (px >= (long long)job.width || py >= (long long)job.height) return;
    const uint32_t centre = (j + RL_DENOISE_HALO) * RL_DENOISE_PITCH + (i + RL_DENOISE_HALO);
    const RlF4 c4 = s_c[centre];
    const RlF3 cp = rl_f3(c4.x, c4.y, c4.z);
    RlF3 result = cp;
    if (c4.w != 0.0f) {
        const RlF4 np = s_n[centre], ap = s_a[centre];
        const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sum_w = 0.0f;
        RlF3 sum_c = rl_f3(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const uint32_t q = (uint32_t)((int)centre + dy * RL_DENOISE_PITCH + dx);
                const RlF4 q4 = s_c[q];
                if (q4.w != 0.0f) rl_denoise_tap(job, cp, np, ap, rl_f3(q4.x, q4.y, q4.z), s_n[q], s_a[q], h[dy + 2] * h[dx + 2], &sum_w, &sum_c);
            }
        }
        result = rl_f3(sum_c.x / sum_w, sum_c.y / sum_w, sum_c.z / sum_w);
    }
    const size_t p = (size_t)py * job.width + (size_t)px;
    out[p * 3] = result.x;
    out[p * 3 + 1] = result.y;
    out[p * 3 + 2] = result.z;
}
