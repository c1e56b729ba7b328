// rl_error.hip.h -- the kernels behind rl_error_unit_*: two f64 planes S and Q of per-pixel sums over the plot buffers shown to the
// unit, and the estimate of the standard error of S from them, per pixel and per 16 x 16 tile.  The arithmetic is the contract
// stated in include/robigo_luculenta.h: f64 and f32 in the stated order, no contraction; add, multiply, the correctly rounded divide,
// the f64 -> f32 conversion and rl_sqrtf only, so the CPU restatement (tests/_error_oracle.py) is held bit for bit.  Included by
// rl_api.hip; needs rl_math.h (rl_sqrtf) only: no scene, no ray kernel.
#pragma once

#define RL_ERROR_TILE_PIXELS (RL_ERROR_TILE * RL_ERROR_TILE)
static_assert(RL_ERROR_TILE_PIXELS == 256, "one 256-thread workgroup per tile; the tree starts at stride 128");

// One observation: S += y, Q += y * y / n over all pixels, y the Y component of the interleaved XYZ plot buffer, which is only
// read.  Pointwise: 12 B of plot buffer and 16 B of state read, 16 B written per pixel.  A lane takes two pixels -- one double2 each
// of S and Q, 16-byte accesses, and the two Y dwords of the pair's 24 bytes of plot buffer (the wave's reads bring in every line of
// the buffer anyway) -- grid-stride, the index 64 bits wide; an odd last pixel goes to lane 0 of workgroup 0, in the manner of
// rl_gather_kernel's tail.  Two pixels, not four, and the register cap below: an f64 divide holds some ten registers while it runs,
// and the kernel must keep to the 32 VGPRs that four resident waves per SIMD of an open trace kernel leave free (rl_kernels.hip.h),
// or every observation of a running App queues up behind the trace kernel's workgroups instead of running beside them.
__device__ __forceinline__ void rl_error_observe_one(double& s, double& q, float y, double n) {
    const double yd = (double)y;
    s = s + yd;
    q = q + (yd * yd) / n;
}

__global__ __launch_bounds__(RL_BLOCK) __attribute__((amdgpu_num_vgpr(16))) void rl_error_observe_kernel(double* __restrict__ sum_y,
                                                                                                         double* __restrict__ sum_q,
                                                                                                         const float* __restrict__ xyz,
                                                                                                         uint64_t n_pixels, double n_paths) {
    const uint64_t n2 = n_pixels / 2;
    double2* s2 = (double2*)sum_y;
    double2* q2 = (double2*)sum_q;
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const float y0 = xyz[6 * i + 1], y1 = xyz[6 * i + 4]; // x0 y0 z0 x1 y1 z1
        double2 s = s2[i], q = q2[i];
        rl_error_observe_one(s.x, q.x, y0, n_paths);
        rl_error_observe_one(s.y, q.y, y1, n_paths);
        s2[i] = s;
        q2[i] = q;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n_pixels & 1)) {
        const uint64_t p = n_pixels - 1;
        double s = sum_y[p], q = sum_q[p];
        rl_error_observe_one(s, q, xyz[3 * p + 1], n_paths);
        sum_y[p] = s;
        sum_q[p] = q;
    }
}

// The two trees of a tile, for a workgroup of 256 threads of which thread t holds the pair (vse, vy) of tile raster index t: every
// thread's pair goes to LDS (tree_se, tree_y: 256 doubles each); the strides 128 and 64 cross waves and are added from LDS between
// barriers; wave 0 then holds v[0 .. 63] in registers, one per lane, and the strides 32 .. 1 are cross-lane moves (lane i reads lane
// i + stride and adds it onto its own: the lanes below `stride` hold exactly v[i] + v[i + stride]; what the lanes above it hold is
// never read again).  Same additions, same order, same bits as the stated tree.  Thread 0 writes the tile's pair; the waves 1 .. 3
// leave at the second barrier, so the call is the last thing its kernel does.  Shared with rl_robust_estimate_kernel
// (rl_robust.hip.h).
__device__ __forceinline__ void rl_error_tile_trees(double* tree_se, double* tree_y, uint32_t t, uint32_t tile, double vse, double vy,
                                                    double* __restrict__ tiles) {
    tree_se[t] = vse;
    tree_y[t] = vy;
    __syncthreads();
    if (t < 128u) {
        vse = tree_se[t] + tree_se[t + 128u];
        vy = tree_y[t] + tree_y[t + 128u];
        tree_se[t] = vse;
        tree_y[t] = vy;
    }
    __syncthreads();
    if (t >= 64u) return; // wave 0 goes on alone
    vse = tree_se[t] + tree_se[t + 64u];
    vy = tree_y[t] + tree_y[t + 64u];
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) {
        vse = vse + __shfl_down(vse, stride, 64);
        vy = vy + __shfl_down(vy, stride, 64);
    }
    if (t == 0u) {
        tiles[2 * (uint64_t)tile] = vse;
        tiles[2 * (uint64_t)tile + 1] = vy;
    }
}

// The estimate: one workgroup per tile, thread t on the tile's pixel (t % 16, t / 16), so t is the tile raster index of the tree.
// A thread outside the image contributes +0.0 to both trees and writes nothing.  The trees are rl_error_tile_trees'.  LDS: the two
// 256-double arrays, 4,096 bytes.  `ratio` is (double)N / (double)(k - 1), divided on the host.
__global__ __launch_bounds__(RL_ERROR_TILE_PIXELS) void rl_error_estimate_kernel(const double* __restrict__ sum_y, const double* __restrict__ sum_q,
                                                                                  uint32_t width, uint32_t height, uint32_t tiles_x, double n_total, double ratio,
                                                                                  float* __restrict__ se_out, double* __restrict__ tiles) {
    __shared__ double tree_se[RL_ERROR_TILE_PIXELS];
    __shared__ double tree_y[RL_ERROR_TILE_PIXELS];
    const uint32_t t = threadIdx.x;
    const uint32_t tile = blockIdx.x; // tiles in raster order, one workgroup each
    const uint32_t x = (tile % tiles_x) * RL_ERROR_TILE + (t % RL_ERROR_TILE), y = (tile / tiles_x) * RL_ERROR_TILE + (t / RL_ERROR_TILE);
    double vse = 0.0, vy = 0.0;
    if (x < width && y < height) {
        const uint64_t p = (uint64_t)y * width + x;
        const double s = sum_y[p], q = sum_q[p];
        double d = q - (s * s) / n_total;
        d = d < 0.0 ? 0.0 : d;
        const double v = d * ratio;
        const float se = rl_sqrtf((float)v);
        se_out[p] = se;
        vse = (double)se;
        vy = fabs(s);
    }
    rl_error_tile_trees(tree_se, tree_y, t, tile, vse, vy, tiles);
}
