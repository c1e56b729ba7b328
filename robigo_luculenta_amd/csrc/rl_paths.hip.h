// rl_paths.hip.h -- the kernels behind rl_scene_camera_rays*, rl_scene_render_rays* and rl_plot_unit_render_samples*: the two
// halves of a path of TraceUnit::render (trace_unit.rs:136-158 and 81-132), on rays a caller supplies, with or without a film.
// Included by rl_api.hip after rl_query.hip.h (rl_intersect_segment), rl_film.hip.h (RlFilmQueue, rl_film_splat) and the public
// header (RlSpectralRay, RlCameraSample, RlPathResult).
#pragma once
#include <type_traits>

// The camera half: what rl_begin_path makes of a path's first two RNG blocks (grid-stride, one path per lane).  Only the scene's
// camera record is read.
__global__ __launch_bounds__(RL_BLOCK) void rl_camera_rays_kernel(const RlF4* __restrict__ scene, RlSceneLayout lay, float aspect_ratio,
                                                                  uint64_t seed, uint32_t stream, uint64_t first_path,
                                                                  RlCameraSample* __restrict__ samples, uint32_t n) {
    RlSceneView sv = {};
    sv.camera_rec = scene + lay.off_camera;
    // (64-bit: a 32-bit index plus the grid's stride wraps past 2^32 for n near 2^32, and a wrapped lane would start over)
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        RlPath p;
        rl_begin_path(sv, aspect_ratio, seed, stream, first_path + i, &p);
        RlCameraSample s;
        s.ray.origin = RlVector3{p.origin.x, p.origin.y, p.origin.z};
        s.ray.wavelength = p.wavelength;
        s.ray.direction = RlVector3{p.direction.x, p.direction.y, p.direction.z};
        s.ray.reserved = 0u;
        s.x = p.sx;
        s.y = p.sy;
        s.reserved0 = s.reserved1 = 0u;
        samples[i] = s;
    }
}


// A kernel's optional output pointer (`results` of the film kernel, `hits` of the step kernel) where it is tested for null and
// used.  Opaque, so that the test is made there, on the pointer's two scalar registers: as a loop invariant the compiler keeps its
// outcome in two more across the persistent loop, which put the film variant that stages nothing and bounds its prisms twice one
// register pair over the path kernel's 32 spilled SGPRs.
template <typename T>
__device__ __forceinline__ T* rl_opaque(T* p) {
    asm volatile("" : "+s"(p));
    return p;
}

// How the step, list-step and light kernels hand out their work: chunks of 64 records (or list positions) from one counter
// (`queue`, zero at launch), every wave taking a slice of them per atomic.  The counter is in chunks.  Large calls (16 records or
// more per lane of the grid) take RL_CHUNK / 64 chunks per atomic, as the path kernel takes its ray indices: one atomic per chunk,
// all on one address, cost more than the chunk's scan; small calls take one, so that every wave gets work.
// Everything here is wave-uniform.
struct RlChunkCursor {
    uint32_t n_chunks;   // ceil(n / 64): chunk c is records c * 64 .. c * 64 + 63, and c * 64 + lane stays under 2^32
    uint32_t slice;      // chunks per atomic
    uint32_t first, left; // this wave's slice of the counter: `left` chunks from `first`
    __device__ __forceinline__ explicit RlChunkCursor(uint32_t n)
        : n_chunks((uint32_t)(((uint64_t)n + 63u) / 64u)),
          slice((uint64_t)n >= (uint64_t)gridDim.x * (RL_TRACE_BLOCK * 16ull) ? (uint32_t)(RL_CHUNK / 64ull) : 1u), first(0), left(0) {}
    // This wave's next chunk in *c; false when the call's chunks are used up (the counter only grows).
    __device__ __forceinline__ bool next(unsigned long long* queue, uint32_t lane, uint32_t* c) {
        if (left == 0) {
            unsigned long long taken = 0;
            if (lane == 0) taken = atomicAdd(queue, (unsigned long long)slice);
            first = __builtin_amdgcn_readfirstlane((uint32_t)taken); // (the counter stays below n_chunks + slice x waves of the grid)
            left = slice;
        }
        *c = first;
        first += 1;
        left -= 1;
        return *c < n_chunks; // (past the end the cursor's state no longer matters: the caller leaves its loop)
    }
    // The chunk next() gave last, again, from the cursor's own copy: for use behind a scan, where the caller's `c` would be one
    // more register held across it.
    __device__ __forceinline__ uint32_t last() const {
        uint32_t done = first;
        asm volatile("" : "+s"(done));
        return done - 1u;
    }
};

__device__ __forceinline__ RlPathResult rl_path_result(float value, uint32_t segments, uint32_t object, uint32_t end) {
    RlPathResult out;
    out.value = value;
    out.segments = segments;
    out.object = object;
    out.end = end;
    return out;
}
// The result of a path that ends after rl_bounce returned `status` for `hit` (`value`: zero where max_segments stopped it).
__device__ __forceinline__ RlPathResult rl_ended_path_result(int status, const RlHit& hit, float value, uint32_t segments, uint32_t emitter) {
    const bool on_light = status == RL_PATH_ENDED_ON_EMITTER;
    uint32_t end = RL_PATH_END_LIMIT;
    if (on_light) end = RL_PATH_END_EMITTER;
    else if (status == RL_PATH_ENDED) end = hit.obj == RL_HIT_NONE ? RL_PATH_END_VOID : RL_PATH_END_ROULETTE;
    return rl_path_result(value, segments, on_light ? emitter : RL_OBJECT_NONE, end);
}

// The path half: TraceUnit::render_ray for in[i] (a ray, or with FILM a camera sample's ray) as path first_path + i.  Persistent
// workgroups laid out as the query kernel's (rl_stage_scene; the same scan), every wave a pool of 64 lanes that refill as their
// paths end: at the top of every iteration, with the wave converged, the lanes without a path take the next ray indices of the
// wave's slice of the call's queue (`queue`, zero at launch; a slice is RL_CHUNK or 64 indices, as the trace kernel takes them),
// assigned by mbcnt.  Without the refill a wave would run as long as its longest path (glass paths have long tails).  Per
// iteration: every lane's segment (rl_intersect_segment; free lanes idle), rl_bounce, and for a path that hit a light the emitter
// term (the f64 Planck evaluation) inline, under the few lanes that need it.  A path that ends writes its RlPathResult.
// max_segments: 1 .. RL_PATH_MAX_SEGMENTS_CAP (the host resolves 0).
// FILM: `results` may be null, `queue` is the counter of an RlFilmQueue, and a path that ends with a value is splatted at
// in[i].x, .y under the lanes that ended.  The screen position is not carried through the loop: a path that ends loads its
// eight bytes again, which keeps the loop's registers those of the kernel without a film.
template <int STAGE, bool CYL, bool FILM>
__device__ __forceinline__ void rl_paths_body(const RlF4* __restrict__ scene, const RlSceneLayout& lay,
                                              const std::conditional_t<FILM, RlCameraSample, RlSpectralRay>* __restrict__ in,
                                              RlPathResult* __restrict__ results, uint32_t n_rays, uint64_t seed, uint32_t stream, uint64_t first_path,
                                              uint32_t max_segments, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const RlSceneView& sv = staged.sv;
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
                RlSpectralRay r;
                if constexpr (FILM) r = in[idx].ray;
                else r = in[idx];
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
                } else if (RlPathResult* res = FILM ? rl_opaque(results) : results; !FILM || res) {
                    // a NaN or infinite wavelength: no path (include/robigo_luculenta.h)
                    res[idx] = rl_path_result(0.0f, 0u, RL_OBJECT_NONE, RL_PATH_END_INVALID);
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
        const RlHit hit = rl_intersect_segment<STAGE, CYL>(staged, lay, active, p.origin, p.direction, ws, lane RL_TACC_ARG);

        // ---- the rest of the loop body (trace_unit.rs:92-126), and the result (and the splat) of a path that ends ----
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
            if (RlPathResult* res = FILM ? rl_opaque(results) : results; !FILM || res)
                res[my_ray] = rl_ended_path_result(status, hit, value, segments, emitter);
            if constexpr (FILM) {
                sx = in[my_ray].x;
                sy = in[my_ray].y;
            }
            active = false;
        }
        // The splat, under the lanes whose path ended with a value.  Adding +0 is the identity; a NaN or infinite position is traced,
        // not splatted.
        if (FILM && ended && value != 0.0f && fabsf(sx) < INFINITY && fabsf(sy) < INFINITY) {
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

template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_ray_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlSpectralRay* __restrict__ rays, RlPathResult* __restrict__ results,
    uint32_t n_rays, uint64_t seed, uint32_t stream, uint64_t first_path, uint32_t max_segments, unsigned long long* __restrict__ queue) {
    rl_paths_body<STAGE, CYL, false>(scene, lay, rays, results, n_rays, seed, stream, first_path, max_segments, queue);
}

// rl_ray_paths_kernel with a film: the rays are samples[i].ray, and the splat goes to the plot unit the RlFilmQueue names.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_film_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlCameraSample* __restrict__ samples, RlPathResult* __restrict__ results,
    uint32_t n_rays, uint64_t seed, uint32_t stream, uint64_t first_path, uint32_t max_segments, unsigned long long* __restrict__ queue) {
    rl_paths_body<STAGE, CYL, true>(scene, lay, samples, results, n_rays, seed, stream, first_path, max_segments, queue);
}
