// rl_film.hip.h -- the kernels behind rl_plot_unit_plot_photons* and rl_plot_unit_render_samples*: PlotUnit::plot
// (plot_unit.rs:87-95) for photons a caller holds, and render_ray (trace_unit.rs:81-132) for a caller's camera samples with the
// splat at the point where a path ends.  Included by rl_api.hip after rl_paths.hip.h (rl_stage_scene).
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

// The kernel's `results` argument where it is tested for null and used.  Opaque, so that the test is made there, on the pointer's
// two scalar registers: as a loop invariant the compiler keeps its outcome in two more across the persistent loop, which put the
// variant that stages nothing and bounds its prisms twice one register pair over the path kernel's 32 spilled SGPRs.
__device__ __forceinline__ RlPathResult* rl_film_results(RlPathResult* results) {
    asm volatile("" : "+s"(results));
    return results;
}

// rl_ray_paths_kernel with a film: render_ray for samples[i].ray as path first_path + i, and a path that ends with a value is
// splatted at samples[i].x, .y under the lanes that ended (the CIE table is the staged scene's, sv.cie).  `results` may be null;
// `queue` is the counter of an RlFilmQueue.
// The loop is a copy of rl_ray_paths_kernel's, statement for statement up to the point where a path ends (its RL_PATHS_EMIT_QUEUE
// alternative left out): that kernel keeps its own text so that its instructions stay what they were measured as, the way
// rl_query_kernel keeps its prologue beside rl_stage_scene.  A change to either loop belongs in both.
// The screen position is not carried through the loop: a path that ends loads its eight bytes again, which keeps the loop's
// registers those of the path kernel.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_film_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlCameraSample* __restrict__ samples, RlPathResult* __restrict__ results,
    uint32_t n_rays, uint64_t seed, uint32_t stream, uint64_t first_path, uint32_t max_segments, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const RlSceneView& sv = staged.sv;
    const RlF4* base = staged.base;
    const uint32_t tab0 = staged.tab0;
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the diagnostic build: reported to rl_stat_counters at the end, as the trace kernel does)
#endif
    uint64_t chunk_next = 0; // wave-uniform: this wave's slice of the queue is [chunk_next, chunk_next + chunk_left)
    uint32_t chunk_left = 0;
    bool active = false;
    uint32_t my_ray = 0, segments = 0;
    RlPath p;
    p.origin = p.direction = rl_f3(0.0f, 0.0f, 0.0f);
    p.wavelength = p.intensity = p.continue_chance = p.sx = p.sy = 0.0f;
    p.ior = 1.0f;
    p.bounce = 0;
    RL_T0(t_total);
    for (;;) {
        // ---- hand ray indices to the lanes without a path ----
        RL_T0(t_refill);
        const uint64_t need = __builtin_amdgcn_ballot_w64(!active);
        // (the queue only grows: once this wave's next index is past the end, so is every index it could still take)
        const bool drained = chunk_next >= n_rays;
        if (need != 0 && !drained) {
            RL_STAT(RL_ST_REFILLS, 1);
            const uint32_t wanted = (uint32_t)__popcll(need);
            const uint32_t avail = chunk_left;
            const uint32_t rank = rl_mbcnt(need);
            uint64_t idx = chunk_next + rank;
            if (avail >= wanted) {
                chunk_next += wanted;
                chunk_left -= wanted;
            } else { // the rest of the slice, then a new one (64 or more indices: enough for every lane)
                // Small calls (fewer than 16 rays per lane of the grid) take 64 indices at a time, so that every wave gets work.
                const uint32_t chunk = (uint64_t)n_rays >= (uint64_t)gridDim.x * (RL_TRACE_BLOCK * 16ull) ? (uint32_t)RL_CHUNK : 64u;
                unsigned long long b = 0;
                if (lane == 0) b = atomicAdd(queue, (unsigned long long)chunk);
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
                const uint64_t b0 = ((uint64_t)hi << 32) | lo;
                if (rank >= avail) idx = b0 + (rank - avail);
                chunk_next = b0 + (wanted - avail);
                chunk_left = chunk - (wanted - avail);
            }
            RL_T0(t_camera); // (the new rays' loads and their SF10 index)
            if (!active && idx < n_rays) {
                const RlSpectralRay r = samples[idx].ray;
                if (fabsf(r.wavelength) < INFINITY) {
                    active = true;
                    my_ray = (uint32_t)idx;
                    segments = 0;
                    p.origin = rl_f3(r.origin.x, r.origin.y, r.origin.z);
                    p.direction = rl_f3(r.direction.x, r.direction.y, r.direction.z);
                    p.wavelength = r.wavelength;
                    p.intensity = 1.0f;
                    p.continue_chance = 1.0f;
                    p.ior = rl_sf10_ior(r.wavelength);
                    p.bounce = 0;
                } else if (RlPathResult* res = rl_film_results(results)) { // a NaN or infinite wavelength: no path (include/robigo_luculenta.h)
                    RlPathResult out;
                    out.value = 0.0f;
                    out.segments = 0u;
                    out.object = RL_OBJECT_NONE;
                    out.end = RL_PATH_END_INVALID;
                    res[idx] = out;
                }
            }
            RL_T1(RL_ST_T_CAMERA, t_camera);
        }
        RL_T1(RL_ST_T_REFILL, t_refill);
        if (__builtin_amdgcn_ballot_w64(active) == 0) {
            if (chunk_next >= n_rays) break;
            continue; // (every ray handed out was invalid: take more)
        }
        RL_STAT(RL_ST_ITER, 1);
        RL_STAT(RL_ST_SCAN_LANES, __popcll(__builtin_amdgcn_ballot_w64(active)));

        // ---- Scene::intersect for every lane's segment ----
        // Segments the scan's culls are not sized for (rl_query_exhaustive): |direction|^2 further than 2^-20 from 1, or a NaN /
        // infinite component.  They scan a null ray as idle lanes and take the linear scan after the wave's scan.
        const RlF3 o = p.origin, d = p.direction;
        const float d2 = d.x * d.x + d.y * d.y + d.z * d.z;
        const bool exhaustive = active && !(fabsf(d2 - 1.0f) <= 0x1p-20f && fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY);
        const bool scanned = active && !exhaustive;
        RlHit hit = rl_scan_wave<CYL, RL_LEAN_SPLIT, STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_NONE && RL_W_S && RL_LEAN_HOIST, STAGE == RL_STAGE_ALL,
                                 STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_ALL>(sv, base + (lay.off_cull - tab0), CYL ? base + (lay.off_prism_cyl - tab0) : nullptr,
                                                                                lay.group_gc, lay.small_ordered, lay.cull_cmax2, lay.n_cluster_groups,
                                                                                lay.n_prism_groups, lay.n_cluster_supers, lay.super_g, staged.ring_t,
                                                                                scanned ? o : rl_f3(0.0f, 0.0f, 0.0f), scanned ? d : rl_f3(0.0f, 0.0f, 0.0f),
                                                                                scanned ? 0u : 0x80000000u, ws, lane RL_TACC_ARG);
        RL_T0(t_exhaustive);
        RL_STAT(RL_ST_X_LANES, __popcll(__builtin_amdgcn_ballot_w64(exhaustive)));
        RL_STAT(RL_ST_X_ITERS, __builtin_amdgcn_ballot_w64(exhaustive) != 0);
        if (exhaustive) hit = rl_query_exhaustive(sv, o, d);
        RL_T1(RL_ST_T_EXHAUSTIVE, t_exhaustive);

        // ---- the rest of the loop body (trace_unit.rs:92-126), and the result and the splat of a path that ends ----
        RL_T0(t_shade);
        int status = RL_PATH_CONTINUES;
        uint32_t emitter = RL_OBJECT_NONE;
        float value = 0.0f;
        if (active) {
            segments += 1;
            status = rl_bounce(sv, seed, stream, first_path + my_ray, &p, hit, &value, &emitter);
        }
        RL_T1(RL_ST_T_SHADE, t_shade);
        RL_T0(t_emit);
        const bool on_light = status == RL_PATH_ENDED_ON_EMITTER;
        RL_STAT(RL_ST_END_EMITTER, __popcll(__builtin_amdgcn_ballot_w64(on_light)));
        if (on_light) value = rl_emission(sv, p.intensity, p.wavelength, emitter);
        const bool ended = active && (status != RL_PATH_CONTINUES || segments >= max_segments);
        float sx = 0.0f, sy = 0.0f;
        if (ended) {
            if (status == RL_PATH_CONTINUES) value = 0.0f; // (stopped by max_segments: no value)
            if (RlPathResult* res = rl_film_results(results)) {
                uint32_t end = RL_PATH_END_LIMIT;
                if (on_light) end = RL_PATH_END_EMITTER;
                else if (status == RL_PATH_ENDED) end = hit.obj == RL_HIT_NONE ? RL_PATH_END_VOID : RL_PATH_END_ROULETTE;
                RlPathResult out;
                out.value = value;
                out.segments = segments;
                out.object = on_light ? emitter : RL_OBJECT_NONE;
                out.end = end;
                res[my_ray] = out;
            }
            sx = samples[my_ray].x;
            sy = samples[my_ray].y;
            active = false;
        }
        // The splat, under the lanes whose path ended with a value.  Adding +0 is the identity; a NaN or infinite position is traced,
        // not splatted.
        if (ended && value != 0.0f && fabsf(sx) < INFINITY && fabsf(sy) < INFINITY) {
            const RlFilm film = ((const RlFilmQueue*)queue)->film; // (written before the launch, never by the kernel)
            const RlF3 c = rl_mul(rl_tristimulus(sv.records + film.off_cie, p.wavelength), value); // (sv.cie)
            rl_film_splat(film.plot, c, rl_splat_weights(film.width, film.height, film.wm1, film.hm1, film.aspect_ratio, sx, sy));
        }
        RL_T1(RL_ST_T_EMIT, t_emit);
        rl_wave_sync(); // (the next iteration's scan rewrites the wave's scratch)
    }
    RL_T1(RL_ST_T_TOTAL, t_total);
#ifdef RL_STATS
    if (lane == 0)
        for (int k = 0; k < RL_ST_COUNT; ++k) atomicAdd(&rl_stat_counters[k], st[k]);
#endif
}
