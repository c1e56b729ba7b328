// rl_denoise_pass.inc.h -- the body of a pass kernel of rl_denoise.hip.h, which includes it once inside each of its two __global__
// functions with RL_DENOISE_VARIANCE defined as 0 (rl_denoise_pass_kernel) or 1 (rl_variance_denoise_pass_kernel): one copy of the
// staging, the tap loop and the write-back.  Text, not a __device__ function: the same body inlined from a function compiles the
// plain kernel to other instructions than it had on its own (39 VGPRs for 43, a fifth of the lines moved), and that kernel is held
// instruction-identical across changes (profiles/denoise_variance_isa_diff.txt).
//   In scope: in, guides, job, out, and with RL_DENOISE_VARIANCE v_in and v_out, the width x height planes V_i and V_{i+1}.  With
// RL_DENOISE_VARIANCE the staged C word's fourth component carries V_i[q] instead of the live flag, and liveness is read from the
// albedo word's fourth component, which holds it in both forms (clear for an element outside the image, as the C word is): the LDS
// is the same three arrays.
#ifndef RL_DENOISE_VARIANCE
#error "included by rl_denoise.hip.h only"
#endif
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
#if RL_DENOISE_VARIANCE
            c = RlF4{in[p * 3], in[p * 3 + 1], in[p * 3 + 2], v_in[p]};
#else
            c = RlF4{in[p * 3], in[p * 3 + 1], in[p * 3 + 2], ga.w};
#endif
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
#if RL_DENOISE_VARIANCE
    float result_v = c4.w, sum_v = 0.0f;
    if (s_a[centre].w != 0.0f) {
#else
    float sum_v = 0.0f; // (not used in this form)
    if (c4.w != 0.0f) {
#endif
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
                if ((RL_DENOISE_VARIANCE ? s_a[q].w : q4.w) != 0.0f)
                    rl_denoise_tap<RL_DENOISE_VARIANCE != 0>(job, cp, c4.w, np, ap, rl_f3(q4.x, q4.y, q4.z), q4.w, s_n[q], s_a[q], h[dy + 2] * h[dx + 2],
                                                             &sum_w, &sum_c, &sum_v);
            }
        }
        result = rl_f3(sum_c.x / sum_w, sum_c.y / sum_w, sum_c.z / sum_w);
#if RL_DENOISE_VARIANCE
        result_v = sum_v / (sum_w * sum_w);
#endif
    }
    const size_t p = (size_t)py * job.width + (size_t)px;
    out[p * 3] = result.x;
    out[p * 3 + 1] = result.y;
    out[p * 3 + 2] = result.z;
#if RL_DENOISE_VARIANCE
    v_out[p] = result_v;
#endif
