// rl_denoise.hip.h -- the kernels behind rl_denoise_unit_denoise: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010)
// over a gather unit's tristimulus buffer, guided by the films of rl_scene_render_features.  The arithmetic is the contract stated
// in include/robigo_luculenta.h: f32, in the stated order, no contraction; add, multiply, the correctly rounded divide, rl_sqrtf and
// rl_expf only, so the CPU restatement (tests/_denoise_oracle.py) is held bit for bit.  Included by rl_api.hip; needs rl_math.h and
// rl_core.h (RlF4) only: no scene, no ray kernel.  At the end, the two kernels of rl_denoise_unit_denoise_variance: the same pass with
// the error unit's variance as the colour term, held to tests/_denoise_variance_oracle.py in the same way.
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

// The weight of tap q for centre p and its products, added to the sums: the per-tap table of the contract, in its order.
// cp, cq: C_i of p and q; np, nq: {n.xyz, z}; ap, aq: {a.xyz, live}; hh: h[dy + 2] * h[dx + 2].  The colour term is all that
// differs between the two forms: the relative difference of luminance (rl_denoise_unit_denoise), or, with VARIANCE, the squared
// difference over the sum vp + vq of the two pixels' variances V_i (rl_denoise_unit_denoise_variance), whose filtered sum the tap
// then adds to *sum_v.
template <bool VARIANCE>
__device__ __forceinline__ void rl_denoise_tap(const RlDenoisePass& job, RlF3 cp, float vp, RlF4 np, RlF4 ap, RlF3 cq, float vq, RlF4 nq, RlF4 aq,
                                               float hh, float* sum_w, RlF3* sum_c, float* sum_v) {
    float e_c;
    if (VARIANCE) {
        const float dl = cp.y - cq.y;
        const float m = vp + vq;
        e_c = m > 0.0f ? (dl * dl) / m : 0.0f;
    } else {
        const float m = fabsf(cp.y) + fabsf(cq.y);
        const float r = m > 0.0f ? (cp.y - cq.y) / m : 0.0f;
        e_c = r * r;
    }
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
    if (VARIANCE) *sum_v += (wt * wt) * vq;
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
//   The body of the kernel is rl_denoise_pass.inc.h, shared as text with the variance form below.
#define RL_DENOISE_TILE 16
#define RL_DENOISE_HALO 2
#define RL_DENOISE_SPAN (RL_DENOISE_TILE + 2 * RL_DENOISE_HALO)
#define RL_DENOISE_PITCH 32
#define RL_DENOISE_LDS_WORDS (RL_DENOISE_SPAN * RL_DENOISE_PITCH)

__global__ __launch_bounds__(RL_DENOISE_TILE * RL_DENOISE_TILE) void rl_denoise_pass_kernel(const float* __restrict__ in, const RlF4* __restrict__ guides,
                                                                                          RlDenoisePass job, float* __restrict__ out) {
#define RL_DENOISE_VARIANCE 0
#include "rl_denoise_pass.inc.h"
#undef RL_DENOISE_VARIANCE
}

// ---- the variance form (rl_denoise_unit_denoise_variance) ----
// (The two kernels are named apart from the rl_denoise_ pair: tests/test_denoise.py holds that prefix to exactly the two above.)

// The same pass with the variance colour term: reads C_i and V_i, writes C_{i+1} and V_{i+1}.  job.kc is kv, the same every pass.
__global__ __launch_bounds__(RL_DENOISE_TILE * RL_DENOISE_TILE) void rl_variance_denoise_pass_kernel(const float* __restrict__ in,
                                                                                                   const float* __restrict__ v_in,
                                                                                                   const RlF4* __restrict__ guides, RlDenoisePass job,
                                                                                                   float* __restrict__ out, float* __restrict__ v_out) {
#define RL_DENOISE_VARIANCE 1
#include "rl_denoise_pass.inc.h"
#undef RL_DENOISE_VARIANCE
}

// V_0 from the error unit's planes: d = Q - (S * S) / N, d < 0 ? 0 : d, v = d * ratio, (float)v -- rl_error_estimate_kernel's v, so
// rl_sqrtf(V_0) is that kernel's se.  `ratio` is (double)N / (double)(k - 1), divided on the host.  Pointwise, 16 B read and 4 B
// written per pixel; two pixels a lane as rl_error_observe_kernel takes them, for the same reason held to 32 VGPRs: it may run
// beside a resident open trace kernel.
__device__ __forceinline__ float rl_denoise_variance_one(double s, double q, double n_total, double ratio) {
    double d = q - (s * s) / n_total;
    d = d < 0.0 ? 0.0 : d;
    const double v = d * ratio;
    return (float)v;
}

__global__ __launch_bounds__(RL_BLOCK) __attribute__((amdgpu_num_vgpr(32))) void rl_variance_denoise_kernel(const double* __restrict__ sum_y,
                                                                                                           const double* __restrict__ sum_q,
                                                                                                           uint64_t n_pixels, double n_total, double ratio,
                                                                                                           float* __restrict__ variance) {
    const uint64_t n2 = n_pixels / 2;
    const double2* s2 = (const double2*)sum_y;
    const double2* q2 = (const double2*)sum_q;
    float2* v2 = (float2*)variance;
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const double2 s = s2[i], q = q2[i];
        v2[i] = float2{rl_denoise_variance_one(s.x, q.x, n_total, ratio), rl_denoise_variance_one(s.y, q.y, n_total, ratio)};
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n_pixels & 1)) {
        const uint64_t p = n_pixels - 1;
        variance[p] = rl_denoise_variance_one(sum_y[p], sum_q[p], n_total, ratio);
    }
}
