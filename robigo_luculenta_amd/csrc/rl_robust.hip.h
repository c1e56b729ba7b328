// rl_robust.hip.h -- the kernels behind rl_robust_unit_*: M sub-films ("buckets") of f64 X, Y, Z sums over the plot buffers shown to
// the unit, and their combination per pixel by a median of means whose trim follows the Gini coefficient of the M bucket means
// (Buisine et al. 2021).  The arithmetic is the contract stated in include/robigo_luculenta.h: f64 in the stated order, no
// contraction; add, multiply, the correctly rounded divide, comparisons and the f64 -> f32 conversion only, so the CPU restatement
// (tests/_robust_oracle.py) is held bit for bit.  Included by rl_api.hip; needs nothing of the scene or the ray kernels.  The
// estimate kernel at the end adds rl_sqrtf (rl_math.h) and the error unit's tile trees (rl_error.hip.h, included before this file);
// its restatement is tests/_robust_error_oracle.py.
#pragma once

// The device layout: plane (j * 3 + c) -- component c of bucket j -- starts at double `(j * 3 + c) * stride`, stride = the pixel
// count rounded up to even, so that every plane starts on 16 bytes and takes double2 accesses (the host layout of download and
// upload is dense; the calls copy plane by plane).
#define RL_ROBUST_LANES 64

// (double)n[j] of every bucket, by value in the kernel arguments: read with wave-uniform indices, so through scalar loads.
struct RlRobustCounts {
    double n[RL_ROBUST_MAX_BUCKETS];
};

// One observation into one bucket: S[c] = S[c] + (double)p[c] over all pixels and the three components; the interleaved XYZ plot
// buffer is only read.  Pointwise: 12 B of plot buffer and 24 B of state read, 24 B written per pixel.  As rl_error_observe_kernel: a
// lane takes two pixels -- one double2 of each of the three planes, 16-byte accesses, and the pair's 24 bytes of plot buffer as
// three 8-byte loads (24 i is a multiple of 8) -- grid-stride, the index 64 bits wide; an odd last pixel goes to lane 0 of workgroup
// 0.  No divide.  The register cap: the kernel must keep to the 32 VGPRs that four resident waves per SIMD of an open trace kernel
// leave free (rl_kernels.hip.h), or every observation of a running render queues up behind the trace kernel's workgroups.  As for
// rl_error_observe_kernel it is the attribute value 16 that holds the allocation to 32 (38 to 40 with 24, 28 or 32); no scratch.
__global__ __launch_bounds__(RL_BLOCK) __attribute__((amdgpu_num_vgpr(16))) void rl_robust_observe_kernel(double* __restrict__ bucket,
                                                                                                          const float* __restrict__ xyz,
                                                                                                          uint64_t n_pixels, uint64_t stride) {
    const uint64_t n2 = n_pixels / 2;
    double2* px = (double2*)bucket;
    double2* py = (double2*)(bucket + stride);
    double2* pz = (double2*)(bucket + 2 * stride);
    const float2* in = (const float2*)xyz;
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const float2 a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2]; // x0 y0 | z0 x1 | y1 z1
        double2 x = px[i], y = py[i], z = pz[i];
        x.x = x.x + (double)a.x;
        x.y = x.y + (double)b.y;
        px[i] = x;
        y.x = y.x + (double)a.y;
        y.y = y.y + (double)c.x;
        py[i] = y;
        z.x = z.x + (double)b.x;
        z.y = z.y + (double)c.y;
        pz[i] = z;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n_pixels & 1)) {
        const uint64_t p = n_pixels - 1;
        bucket[p] = bucket[p] + (double)xyz[3 * p];
        bucket[stride + p] = bucket[stride + p] + (double)xyz[3 * p + 1];
        bucket[2 * stride + p] = bucket[2 * stride + p] + (double)xyz[3 * p + 2];
    }
}

// The resolve: one pixel per lane.  The 3 M sums are read plane by plane (coalesced across lanes), divided by their bucket's path
// count and kept in LDS as mean[c][j][lane]: a lane only ever touches its own column, so consecutive lanes hit consecutive bank
// pairs whatever row each of them reads (the rank walk reads rows that differ from lane to lane), there is nothing to conflict and
// nothing to synchronise -- no barrier in the kernel.  The rank of bucket j is M compares of its Y mean against the column, M^2 LDS
// reads per pixel; perm[rank][lane] = j goes to LDS as bytes, and the sums then walk the ranks in order.  No register is indexed
// dynamically: no scratch.
//   LDS: M * 64 lanes * (24 + 1) bytes per wave, 24,000 B at M = 15 and 51,200 B at M = 32.  The workgroup is ONE wave: lanes share
// nothing, so a larger workgroup buys nothing and only coarsens what the CU's 160 KiB are handed out in -- at M = 32 three 64-lane
// workgroups fit a CU (12 waves at M = 8, 6 at M = 15), where a 128-lane workgroup would leave one (2 waves) and the habitual 256
// lanes would not fit at all.  All three means sit in LDS rather than the Y means alone: with the keys only, the X and Z sums of
// the kept buckets would be read again in rank order, a gather in which neighbouring lanes read different planes.  Measured
// (tools/robust_bench.py, profiles/robust_bench.txt, 1280 x 720 on an MI355X) against a device copy of the bytes the kernel moves:
// 0.271 ms at M = 15 and 1.469 ms at M = 32, 4.4 and 11.7 times the copy -- the rank loop's M^2 dependent LDS reads at this
// occupancy, not the planes' traffic, are what it waits for.  Once per image; DESIGN.md section 4 names the next step.
//   trim[p] = c, with bit 7 set for an untrimmable pixel (c is then 0): the host takes the counts from these bytes.
__global__ __launch_bounds__(RL_ROBUST_LANES) void rl_robust_resolve_kernel(const double* __restrict__ sums, uint64_t stride, uint64_t n_pixels,
                                                                            uint32_t m_buckets, RlRobustCounts counts, double n_total, double gain,
                                                                            uint32_t cmax, float* __restrict__ dst, uint8_t* __restrict__ trim) {
    extern __shared__ double rl_robust_lds[];
    const uint32_t lane = threadIdx.x, M = m_buckets;
    double* mean = rl_robust_lds + lane;                                                    // mean[(c * M + j) * 64]
    double* key = mean + (size_t)M * RL_ROBUST_LANES;                                       // the Y means
    uint8_t* perm = (uint8_t*)(rl_robust_lds + (size_t)3 * M * RL_ROBUST_LANES) + lane;     // perm[r * 64]
    const double md = (double)M;
    for (uint64_t p = (uint64_t)blockIdx.x * RL_ROBUST_LANES + lane; p < n_pixels; p += (uint64_t)gridDim.x * RL_ROBUST_LANES) {
        bool untrimmable = false;
        for (uint32_t j = 0; j < M; ++j) {
            const double n = counts.n[j];
            const double* s = sums + (uint64_t)j * 3 * stride + p;
            const double x = s[0] / n, y = s[stride] / n, z = s[2 * stride] / n;
            mean[(size_t)j * RL_ROBUST_LANES] = x;
            key[(size_t)j * RL_ROBUST_LANES] = y;
            mean[(size_t)(2 * M + j) * RL_ROBUST_LANES] = z;
            untrimmable = untrimmable || !(y >= 0.0) || y == (double)INFINITY; // not finite, or < 0
        }
        for (uint32_t j = 0; j < M; ++j) {
            const double kj = key[(size_t)j * RL_ROBUST_LANES];
            uint32_t rank = 0;
            for (uint32_t i = 0; i < M; ++i) {
                const double ki = key[(size_t)i * RL_ROBUST_LANES];
                rank += (ki < kj || (ki == kj && i < j)) ? 1u : 0u;
            }
            perm[(size_t)(untrimmable ? j : rank) * RL_ROBUST_LANES] = (uint8_t)j; // (an untrimmable pixel: bucket order)
        }
        uint32_t c = 0;
        if (!untrimmable) {
            double t = 0.0, w = 0.0;
            for (uint32_t r = 0; r < M; ++r) {
                const double k = key[(size_t)perm[(size_t)r * RL_ROBUST_LANES] * RL_ROBUST_LANES];
                t = t + k;
                w = w + (double)(2 * (int)r - (int)M + 1) * k;
            }
            if (!(t > 0.0)) {
                untrimmable = true;
            } else {
                const double g = w / (md * t);
                const double v = ((gain * g) * md) * 0.5;
                c = !(v >= 0.0) ? 0u : (v >= (double)cmax ? cmax : (uint32_t)v); // (0 <= v < cmax: the conversion truncates = floor)
            }
        }
        const double kept = (double)(M - 2 * c);
        for (uint32_t comp = 0; comp < 3; ++comp) {
            const double* column = mean + (size_t)comp * M * RL_ROBUST_LANES;
            double a = 0.0;
            for (uint32_t r = c; r < M - c; ++r) a = a + column[(size_t)perm[(size_t)r * RL_ROBUST_LANES] * RL_ROBUST_LANES];
            dst[p * 3u + comp] = (float)((a / kept) * n_total);
        }
        trim[p] = (uint8_t)(c | (untrimmable ? 0x80u : 0u));
    }
}

// The estimate (rl_robust_unit_estimate): the standard error of the trimmed film's Y from the M bucket means -- the winsorized sum
// of squares over K (K - 1), K = M - 2 c kept buckets -- per pixel and, through rl_error_tile_trees, per RL_ERROR_TILE tile in the
// error unit's output format.  One 256-thread workgroup per tile, thread t on the tile's pixel (t % 16, t / 16) as in
// rl_error_estimate_kernel.  Only the Y planes are read, a third of the resolve's traffic.  The keys of a thread sit in LDS as
// key[j][t] and the rank permutation as bytes perm[r][t]: a thread touches its own column only, so there is nothing to conflict and,
// until the trees, nothing to synchronise.  M * 256 * 9 bytes: 34,560 B at M = 15 (four workgroups per CU), 73,728 B at M = 32
// (two); the 4 KB of the two trees reuse the first 512 doubles after a barrier (M >= 3: 6,912 B at least).  The ranking and the
// trim are the resolve's forty lines once more, with the keys alone and the estimate's cap: shared code would have to leave
// rl_robust_resolve_kernel instruction-identical, and its one-wave layout (a stride of 64, three means per bucket) differs in every
// address.  No register is indexed dynamically: no scratch.  A thread outside the image skips the pixel and adds +0.0 to both trees.
__global__ __launch_bounds__(RL_ERROR_TILE_PIXELS) void rl_robust_estimate_kernel(const double* __restrict__ sums, uint64_t stride, uint32_t width,
                                                                                   uint32_t height, uint32_t tiles_x, uint32_t m_buckets,
                                                                                   RlRobustCounts counts, double n_total, double gain, uint32_t cmax,
                                                                                   float* __restrict__ se_out, double* __restrict__ tiles,
                                                                                   uint8_t* __restrict__ trim) {
    extern __shared__ double rl_robust_lds[];
    const uint32_t t = threadIdx.x, M = m_buckets;
    const uint32_t tile = blockIdx.x; // tiles in raster order, one workgroup each
    const uint32_t x = (tile % tiles_x) * RL_ERROR_TILE + (t % RL_ERROR_TILE), y = (tile / tiles_x) * RL_ERROR_TILE + (t / RL_ERROR_TILE);
    double* key = rl_robust_lds + t;                                                          // key[j * 256]
    uint8_t* perm = (uint8_t*)(rl_robust_lds + (size_t)M * RL_ERROR_TILE_PIXELS) + t;         // perm[r * 256]
    const double md = (double)M;
    double vse = 0.0, vy = 0.0;
    if (x < width && y < height) {
        const uint64_t p = (uint64_t)y * width + x;
        bool untrimmable = false;
        for (uint32_t j = 0; j < M; ++j) {
            const double k = sums[((uint64_t)j * 3 + 1) * stride + p] / counts.n[j];
            key[(size_t)j * RL_ERROR_TILE_PIXELS] = k;
            untrimmable = untrimmable || !(k >= 0.0) || k == (double)INFINITY; // not finite, or < 0
        }
        for (uint32_t j = 0; j < M; ++j) {
            const double kj = key[(size_t)j * RL_ERROR_TILE_PIXELS];
            uint32_t rank = 0;
            for (uint32_t i = 0; i < M; ++i) {
                const double ki = key[(size_t)i * RL_ERROR_TILE_PIXELS];
                rank += (ki < kj || (ki == kj && i < j)) ? 1u : 0u;
            }
            perm[(size_t)(untrimmable ? j : rank) * RL_ERROR_TILE_PIXELS] = (uint8_t)j; // (an untrimmable pixel: bucket order)
        }
        uint32_t c = 0;
        if (!untrimmable) {
            double ts = 0.0, w = 0.0;
            for (uint32_t r = 0; r < M; ++r) {
                const double k = key[(size_t)perm[(size_t)r * RL_ERROR_TILE_PIXELS] * RL_ERROR_TILE_PIXELS];
                ts = ts + k;
                w = w + (double)(2 * (int)r - (int)M + 1) * k;
            }
            if (!(ts > 0.0)) {
                untrimmable = true;
            } else {
                const double g = w / (md * ts);
                const double v = ((gain * g) * md) * 0.5;
                c = !(v >= 0.0) ? 0u : (v >= (double)cmax ? cmax : (uint32_t)v); // (0 <= v < cmax: the conversion truncates = floor)
            }
        }
        const uint32_t K = M - 2 * c;
        const double cd = (double)c;
        const double lo = key[(size_t)perm[(size_t)c * RL_ERROR_TILE_PIXELS] * RL_ERROR_TILE_PIXELS];
        const double hi = key[(size_t)perm[(size_t)(M - c - 1) * RL_ERROR_TILE_PIXELS] * RL_ERROR_TILE_PIXELS];
        double a = 0.0;
        for (uint32_t r = c; r < M - c; ++r) a = a + key[(size_t)perm[(size_t)r * RL_ERROR_TILE_PIXELS] * RL_ERROR_TILE_PIXELS];
        double b = cd * lo + a;
        b = b + cd * hi;
        const double mw = b / md; // the winsorized mean
        double d = 0.0;
        for (uint32_t r = c; r < M - c; ++r) {
            const double e = key[(size_t)perm[(size_t)r * RL_ERROR_TILE_PIXELS] * RL_ERROR_TILE_PIXELS] - mw;
            d = d + e * e;
        }
        const double el = lo - mw;
        d = d + cd * (el * el);
        const double eh = hi - mw;
        d = d + cd * (eh * eh);
        const double var = d / (double)(K * (K - 1u));
        const double f = (a / (double)K) * n_total;
        const double v = (var * n_total) * n_total;
        const float se = rl_sqrtf((float)v);
        se_out[p] = se;
        trim[p] = (uint8_t)(c | (untrimmable ? 0x80u : 0u));
        vse = (double)se;
        vy = fabs(f);
    }
    __syncthreads(); // every thread is done with its column: the trees take the first 4 KB
    rl_error_tile_trees(rl_robust_lds, rl_robust_lds + RL_ERROR_TILE_PIXELS, t, tile, vse, vy, tiles);
}
