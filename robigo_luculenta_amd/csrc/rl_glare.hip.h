// rl_glare.hip.h -- the kernel behind rl_glare_unit_apply: one K x K gather table per spectral node applied to a spectral unit's
// film, the result projected under an n_nodes x 3 matrix in the same launch.  The convolved cube never exists in memory.  The
// arithmetic is the contract stated in include/robigo_luculenta.h: f32, a separate multiply and add, per pixel and node the row
// sums r_j in tap order, then g = sum of the r_j in row order, then acc_c = acc_c + matrix[b][c] * g; the CPU restatement
// (tests/_glare_oracle.py) holds it bit for bit.  Included by rl_api.hip; needs rl_core.h only: no scene, no CIE table, no ray kernel.
#pragma once

#define RL_GLARE_TILE_X 64 // output pixels of a workgroup: 64 x 16, four in a row per lane (16 x 16 lanes)
#define RL_GLARE_TILE_Y 16
#define RL_GLARE_BLOCK 256
#define RL_GLARE_MAX_GRID (1u << 20)

typedef float RlGlare2 __attribute__((ext_vector_type(2)));
typedef float RlGlare4 __attribute__((ext_vector_type(4)));

// LDS of a launch, in floats: the staged tile with its halo, rows of `stride` floats (a multiple of 4: every lane's window loads are
// 16-byte aligned), then the node's table, rows of `table stride` floats (the same).  At 65 taps: 128 x 80 + 65 x 68 floats = 58,640
// bytes, below the 64 KiB a launch gets without asking and two workgroups to a CU; at 33 taps 23,184 bytes, seven.
__host__ __device__ inline uint32_t rl_glare_stride(uint32_t taps) { return (RL_GLARE_TILE_X + taps - 1u + 3u) & ~3u; }
__host__ __device__ inline uint32_t rl_glare_table_stride(uint32_t taps) { return (taps + 3u) & ~3u; }
__host__ __device__ inline uint32_t rl_glare_lds_floats(uint32_t taps) {
    return rl_glare_stride(taps) * (RL_GLARE_TILE_Y + taps - 1u) + taps * rl_glare_table_stride(taps);
}

// One tap of the table on a lane's four pixels: r_p = r_p + t * v_p, multiply and add separate, as two packed operations each.
// The fast form: every staged value outside the film is +0 and the table is finite, so the tap the contract skips adds t * 0 =
// +-0 to a row sum that is never -0 (it starts at +0, and x + y is -0 only if both are): the bits of the skip.
__device__ __forceinline__ void rl_glare_tap(RlGlare2& r01, RlGlare2& r23, float t, float v0, float v1, float v2, float v3) {
    const RlGlare2 tt = {t, t};
    const RlGlare2 a = {v0, v1}, b = {v2, v3};
    r01 = r01 + tt * a;
    r23 = r23 + tt * b;
}
// The exact form, for a table with a NaN or an infinity in it (t * 0 is then not 0): a tap outside the film leaves r as it was.
// `first` is the window column of v0; columns lo .. hi of the lane's row are inside the film (none if the row is not: lo > hi).
__device__ __forceinline__ void rl_glare_tap_skip(float (&r)[4], float t, float v0, float v1, float v2, float v3, int first, int lo, int hi) {
    const float v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float sum = r[p] + t * v[p];
        r[p] = (first + p >= lo && first + p <= hi) ? sum : r[p];
    }
}

// Grid: one block per 64 x 16 tile in raster order, tiles_x to a row (a launch of fewer blocks strides over them: the grid is capped
// at RL_GLARE_MAX_GRID); block: RL_GLARE_BLOCK lanes, lane (lx, ly) = (thread & 15, thread >> 4) owns pixels
// (x0 + 4 lx .. + 3, y0 + ly).  Per node: the plane's tile plus halo and the node's table are staged in LDS once (zeros outside the
// film), then every lane walks the K rows of the table; in a row it slides a window of staged values through registers, one
// ds_read_b128 of the tile and one (wave-uniform, broadcast) of the table per four taps and sixteen multiply-adds, so the LDS runs
// at an eighth of what the vector unit asks for.  Rows of taps are independent chains; the four pixels of a lane are too.
// EXACT_SKIP: see rl_glare_tap_skip.  The host picks it when a table entry is not finite and never otherwise.
template <bool EXACT_SKIP>
__global__ __launch_bounds__(RL_GLARE_BLOCK) void rl_glare_kernel(const float* __restrict__ film, const float* __restrict__ tables,
                                                                  const float* __restrict__ matrix, uint32_t width, uint32_t height,
                                                                  uint32_t n_nodes, uint32_t taps, uint32_t tiles_x, uint32_t n_tiles,
                                                                  float* __restrict__ dst) {
    extern __shared__ RlGlare4 rl_glare_lds[];
    float* const tile = (float*)rl_glare_lds;
    const uint32_t radius = taps >> 1;
    const uint32_t stride = rl_glare_stride(taps), table_stride = rl_glare_table_stride(taps);
    const uint32_t rows = RL_GLARE_TILE_Y + taps - 1u, cols = RL_GLARE_TILE_X + taps - 1u;
    float* const table = tile + stride * rows;
    const uint32_t lx = threadIdx.x & 15u, ly = threadIdx.x >> 4;
    const uint64_t n_pixels = (uint64_t)width * height;
    const uint32_t quads = taps >> 2; // whole groups of four taps; taps is odd, so one or three taps remain
  for (uint32_t tile_index = blockIdx.x; tile_index < n_tiles; tile_index += gridDim.x) {
    const uint32_t tile_y = tile_index / tiles_x, tile_x = tile_index - tile_y * tiles_x;
    const int x_first = (int)(tile_x * RL_GLARE_TILE_X) - (int)radius; // the film column of tile column 0
    const int y_first = (int)(tile_y * RL_GLARE_TILE_Y) - (int)radius;
    // (EXACT_SKIP) the window columns of this lane's rows that are inside the film, relative to the lane's first column
    const int col_lo = -x_first - (int)(4u * lx), col_hi = (int)width - 1 - x_first - (int)(4u * lx);
    const int row_lo = -y_first - (int)ly, row_hi = (int)height - 1 - y_first - (int)ly;

    RlGlare2 acc_x[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, acc_y[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, acc_z[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    for (uint32_t b = 0; b < n_nodes; ++b) {
        __syncthreads(); // the previous node's tile and table have been read
        const float* plane = film + (uint64_t)b * n_pixels;
        for (uint32_t r = threadIdx.x >> 6; r < rows; r += RL_GLARE_BLOCK / 64u) {
            const int qy = y_first + (int)r;
            const bool row_in = qy >= 0 && qy < (int)height;
            for (uint32_t c = threadIdx.x & 63u; c < stride; c += 64u) {
                const int qx = x_first + (int)c;
                float v = 0.0f;
                if (row_in && c < cols && qx >= 0 && qx < (int)width) v = plane[(uint64_t)qy * width + (uint32_t)qx];
                tile[r * stride + c] = v;
            }
        }
        const float* node_table = tables + (uint64_t)b * taps * taps;
        for (uint32_t r = threadIdx.x >> 6; r < taps; r += RL_GLARE_BLOCK / 64u)
            for (uint32_t c = threadIdx.x & 63u; c < table_stride; c += 64u) table[r * table_stride + c] = c < taps ? node_table[r * taps + c] : 0.0f;
        __syncthreads();

        RlGlare2 g01 = {0.0f, 0.0f}, g23 = {0.0f, 0.0f};
        for (uint32_t j = 0; j < taps; ++j) {
            const RlGlare4* src = (const RlGlare4*)(tile + (ly + j) * stride + 4u * lx);
            const RlGlare4* trow = (const RlGlare4*)(table + j * table_stride);
            RlGlare4 cur = src[0];
            if constexpr (EXACT_SKIP) {
                const bool row_in = (int)j >= row_lo && (int)j <= row_hi;
                const int lo = row_in ? col_lo : 1, hi = row_in ? col_hi : 0;
                float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (uint32_t q = 0; q <= quads; ++q) {
                    const bool more = q < quads || (taps & 3u) == 3u; // taps beyond the first of this group
                    const RlGlare4 nxt = more ? src[q + 1u] : cur;    // (as below: inside the row's stride)
                    const RlGlare4 t = trow[q];
                    const int i = (int)(4u * q);
                    rl_glare_tap_skip(r, t.x, cur.x, cur.y, cur.z, cur.w, i, lo, hi);
                    if (more) {
                        rl_glare_tap_skip(r, t.y, cur.y, cur.z, cur.w, nxt.x, i + 1, lo, hi);
                        rl_glare_tap_skip(r, t.z, cur.z, cur.w, nxt.x, nxt.y, i + 2, lo, hi);
                    }
                    if (q < quads) rl_glare_tap_skip(r, t.w, cur.w, nxt.x, nxt.y, nxt.z, i + 3, lo, hi);
                    cur = nxt;
                }
                g01 = g01 + RlGlare2{r[0], r[1]};
                g23 = g23 + RlGlare2{r[2], r[3]};
            } else {
                RlGlare2 r01 = {0.0f, 0.0f}, r23 = {0.0f, 0.0f};
                for (uint32_t q = 0; q < quads; ++q) {
                    const RlGlare4 nxt = src[q + 1u];
                    const RlGlare4 t = trow[q];
                    rl_glare_tap(r01, r23, t.x, cur.x, cur.y, cur.z, cur.w);
                    rl_glare_tap(r01, r23, t.y, cur.y, cur.z, cur.w, nxt.x);
                    rl_glare_tap(r01, r23, t.z, cur.z, cur.w, nxt.x, nxt.y);
                    rl_glare_tap(r01, r23, t.w, cur.w, nxt.x, nxt.y, nxt.z);
                    cur = nxt;
                }
                const RlGlare4 t = trow[quads];
                rl_glare_tap(r01, r23, t.x, cur.x, cur.y, cur.z, cur.w);
                if ((taps & 3u) == 3u) {
                    const RlGlare4 nxt = src[quads + 1u]; // (reaches 8 bytes past the row's staged columns, inside its stride: not used)
                    rl_glare_tap(r01, r23, t.y, cur.y, cur.z, cur.w, nxt.x);
                    rl_glare_tap(r01, r23, t.z, cur.z, cur.w, nxt.x, nxt.y);
                }
                g01 = g01 + r01;
                g23 = g23 + r23;
            }
        }
        const float mx = matrix[3u * b], my = matrix[3u * b + 1u], mz = matrix[3u * b + 2u];
        acc_x[0] = acc_x[0] + RlGlare2{mx, mx} * g01;
        acc_x[1] = acc_x[1] + RlGlare2{mx, mx} * g23;
        acc_y[0] = acc_y[0] + RlGlare2{my, my} * g01;
        acc_y[1] = acc_y[1] + RlGlare2{my, my} * g23;
        acc_z[0] = acc_z[0] + RlGlare2{mz, mz} * g01;
        acc_z[1] = acc_z[1] + RlGlare2{mz, mz} * g23;
    }

    const uint32_t y = tile_y * RL_GLARE_TILE_Y + ly;
    const uint32_t x = tile_x * RL_GLARE_TILE_X + 4u * lx;
    if (y >= height) continue;
    float* out = dst + ((uint64_t)y * width + x) * 3u;
    const float px[4] = {acc_x[0].x, acc_x[0].y, acc_x[1].x, acc_x[1].y};
    const float py[4] = {acc_y[0].x, acc_y[0].y, acc_y[1].x, acc_y[1].y};
    const float pz[4] = {acc_z[0].x, acc_z[0].y, acc_z[1].x, acc_z[1].y};
#pragma unroll
    for (uint32_t p = 0; p < 4u; ++p) {
        if (x + p < width) {
            out[3u * p] = px[p];
            out[3u * p + 1u] = py[p];
            out[3u * p + 2u] = pz[p];
        }
    }
  }
}
