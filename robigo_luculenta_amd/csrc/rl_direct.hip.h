// rl_direct.hip.h -- the kernel behind rl_plot_unit_render_direct: camera paths of the RNG with direct light, into a film, in one
// persistent launch.  The path kernel's loop (rl_paths.hip.h: rl_paths_body) with the light kernel's middle (rl_light.hip.h:
// rl_light_body): every wave is a pool of 64 lanes that refill as their paths end; per iteration every lane's segment
// (rl_intersect_segment), rl_bounce and the emitter term, then one direct-light sample at the vertex (rl_light_sample on the
// state as rl_scene_step_paths would leave it and the hit record rl_ray_hit_of makes), the wave's shadow rays in one bounded scan
// (rl_occluded_segment, in the scratch the first scan has left), and the splat.  What the loop of public calls keeps in
// RlPathState, RlRayHit, RlLightSample and the `sampled` byte stays in the wave here: in registers, and in the part of its scratch
// that no scan uses (rl_direct_counters, rl_direct_parked).  Included by rl_api.hip after
// rl_light.hip.h (rl_occluded_segment, RlFilm, rl_film_splat, rl_opaque, rl_ended_path_result, rl_ray_hit_of).
#pragma once

// What a launch reads beside the scene, behind its queue counter as RlLightFilmQueue's block is and for its reason: launch
// constants passed as kernel arguments are scalar registers held across the persistent loop, and those spill.  The loop loads
// each word where it uses it.
struct RlDirectJob {
    RlPathResult* results;        // null, or n_paths records
    const RlF4* emitters;         // the scene's emitter table (rl_core.h: RL_EMITTER_STRIDE records per emitter)
    const uint8_t* emitter_flags; // null (a scene without a sampleable emitter), or one byte per object: 1 for the emitters of the table
    uint64_t seed;
    uint64_t first_path;          // the launch's path i is path first_path + i of the stream
    uint32_t n_paths;             // of this launch
    uint32_t stream;
    uint32_t max_segments;        // resolved: 1 .. RL_PATH_MAX_SEGMENTS_CAP
    uint32_t n_emitters;
    uint32_t n_objects;           // the length of emitter_flags
    float aspect_ratio;           // the camera's: the film's
    RlFilm film;
};
// The counters of RlDirectStats but `paths`, in its order.
enum { RL_DIRECT_SEGMENTS, RL_DIRECT_LIGHT_SAMPLES, RL_DIRECT_SHADOW_RAYS, RL_DIRECT_VISIBLE, RL_DIRECT_KEPT, RL_DIRECT_DROPPED, RL_DIRECT_COUNTERS };
struct RlDirectQueue {
    unsigned long long next; // the queue counter, in path indices of the launch: zero at launch
    RlDirectJob job;
    // Every wave adds its totals here when it leaves the loop (RL_DIRECT_VISIBLE: the BLOCKED rays, rl_direct_body).  The host
    // zeroes them once per call, not per launch: the launches of one call add up.
    unsigned long long stats[RL_DIRECT_COUNTERS];
};

// Where the counters of a wave live between its iterations: one 64-bit total per lane and counter in the part of the wave's scratch
// that only the trace kernel uses (RlWaveScratch::stash and ::emit, its camera stash and emitter queue: no scan touches them),
// so that they cost no register across the two scans.  Row RL_DIRECT_VISIBLE counts the BLOCKED rays there: the visible ones are
// the cast ones less those.  No LDS is added.
static_assert(offsetof(RlWaveScratch, emit) == offsetof(RlWaveScratch, stash) + sizeof(((RlWaveScratch*)0)->stash) &&
                  sizeof(((RlWaveScratch*)0)->stash) + sizeof(((RlWaveScratch*)0)->emit) >= RL_DIRECT_COUNTERS * 64 * sizeof(unsigned long long) &&
                  offsetof(RlWaveScratch, stash) % 8 == 0,
              "the direct kernel's counters take the trace kernel's stash and emitter queue");
__device__ __forceinline__ RlLdsU64* rl_direct_counters(RlWaveScratch* ws) { return (RlLdsU64*)&ws->stash[0][0]; }
// Behind the counters, in the rest of ::emit: what a path carries from bounce to bounce and no scan reads -- its intensity, its
// continue chance and its index of refraction -- one slot per lane each, written where the value is made and read before the
// bounce, so that they too cost no register across the scans (the two scans of an iteration left the variants that do not stage
// the whole scene without one to spare).
enum { RL_DIRECT_INTENSITY, RL_DIRECT_CONTINUE, RL_DIRECT_IOR, RL_DIRECT_PARKED };
static_assert(sizeof(((RlWaveScratch*)0)->stash) + sizeof(((RlWaveScratch*)0)->emit) >= RL_DIRECT_COUNTERS * 64 * sizeof(unsigned long long) + RL_DIRECT_PARKED * 64 * sizeof(float),
              "the direct kernel's parked path state takes the rest of the trace kernel's emitter queue");
__device__ __forceinline__ RlLdsF* rl_direct_parked(RlWaveScratch* ws, int k, uint32_t lane) {
    return (RlLdsF*)(rl_direct_counters(ws) + RL_DIRECT_COUNTERS * 64) + (k * 64 + lane);
}
// One more for the lanes of `flag`, in row K.
__device__ __forceinline__ void rl_direct_count(RlWaveScratch* ws, uint32_t lane, int k, bool flag) {
    __hip_atomic_fetch_add(rl_direct_counters(ws) + (k * 64 + lane), flag ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// A 64-bit launch constant that a lane has loaded, in scalar registers (rl_rng.h wants the seed there).  The builtin returns an
// int: each half goes through uint32_t, or a low word with its top bit set would extend into the high one.
__device__ __forceinline__ uint64_t rl_direct_uniform64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// In `segments`, above the count (at most RL_PATH_MAX_SEGMENTS_CAP): the lane has no path; and the `sampled` byte of the loop of
// public calls: did the vertex before get a sample (any status but RL_LIGHT_SKIPPED)?
#define RL_DIRECT_FREE 0x40000000u
#define RL_DIRECT_SAMPLED 0x80000000u

// Termination: a lane's path makes at most max_segments segments (`ended` below), every iteration with a path in some lane makes
// a segment for it, and an iteration without one either takes indices from the queue, which only grows, or leaves.  A wave waits
// for nothing but its own loads: no spins, no flags, no grid barrier.
template <int STAGE, bool CYL>
__device__ __forceinline__ void rl_direct_body(const RlF4* __restrict__ scene, const RlSceneLayout& lay, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const RlSceneView& sv = staged.sv;
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif
#pragma unroll
    for (int k = 0; k < RL_DIRECT_COUNTERS; ++k) rl_direct_counters(ws)[k * 64 + lane] = 0ull; // (the LDS holds whatever the kernel before left)
    // Wave-uniform: the next index of this wave's slice of the queue.  A slice is `chunk` indices from a multiple of `chunk`, so what
    // is left of it follows from the index (none when it stands on a multiple).  32 bits: a launch has at most 2^30 paths
    // (rl_api.hip: RL_DIRECT_LAUNCH), and the counter stays below that plus a slice for every wave of the grid.
    uint32_t chunk_next = 0;
    uint32_t my_path = 0, segments = RL_DIRECT_FREE;
    // What of the path crosses the scans in registers: the segment and the wavelength (rl_direct_parked has the rest).
    RlF3 origin = rl_f3(0.0f, 0.0f, 0.0f), direction = rl_f3(0.0f, 0.0f, 0.0f);
    float wavelength = 0.0f;
    for (;;) {
        // ---- hand path indices to the lanes without a path (rl_paths_body's refill) ----
        const uint64_t need = __builtin_amdgcn_ballot_w64((segments & RL_DIRECT_FREE) != 0u);
        if (need != 0) {
            const RlDirectJob* job = &((const RlDirectQueue*)rl_opaque(queue))->job;
            const uint32_t n_paths = __builtin_amdgcn_readfirstlane(job->n_paths);
            if (chunk_next < n_paths) { // (the queue only grows: once this wave's next index is past the end, so is every index it could still take)
                // Small launches (fewer than 16 paths per lane of the grid) take 64 indices at a time, so that every wave gets work.
                const uint32_t chunk = (uint64_t)n_paths >= (uint64_t)gridDim.x * (RL_TRACE_BLOCK * 16ull) ? (uint32_t)RL_CHUNK : 64u;
                const uint32_t wanted = (uint32_t)__popcll(need);
                const uint32_t avail = (0u - chunk_next) & (chunk - 1u);
                const uint32_t rank = rl_mbcnt(need);
                uint32_t idx = chunk_next + rank;
                if (avail >= wanted) {
                    chunk_next += wanted;
                } else { // the rest of the slice, then a new one (64 or more indices: enough for every lane)
                    unsigned long long b = 0;
                    if (lane == 0) b = atomicAdd(queue, (unsigned long long)chunk);
                    const uint32_t b0 = __builtin_amdgcn_readfirstlane((uint32_t)b);
                    if (rank >= avail) idx = b0 + (rank - avail);
                    chunk_next = b0 + (wanted - avail);
                }
                if ((segments & RL_DIRECT_FREE) != 0u && idx < n_paths) {
                    const uint64_t seed = rl_direct_uniform64(job->seed);
                    const uint64_t first = rl_direct_uniform64(job->first_path);
                    my_path = idx;
                    segments = 0; // (and both bits)
                    RlPath fresh;
                    rl_begin_path(sv, job->aspect_ratio, seed, __builtin_amdgcn_readfirstlane(job->stream), first + idx, &fresh);
                    origin = fresh.origin;
                    direction = fresh.direction;
                    wavelength = fresh.wavelength;
                    *rl_direct_parked(ws, RL_DIRECT_INTENSITY, lane) = fresh.intensity;
                    *rl_direct_parked(ws, RL_DIRECT_CONTINUE, lane) = fresh.continue_chance;
                    *rl_direct_parked(ws, RL_DIRECT_IOR, lane) = fresh.ior;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64((segments & RL_DIRECT_FREE) == 0u) == 0) break; // (nothing was handed out: the wave's slice is past the end)

        // ---- Scene::intersect for every lane's segment ----
        const RlHit hit = rl_intersect_segment<STAGE, CYL>(staged, lay, (segments & RL_DIRECT_FREE) == 0u, origin, direction, ws, lane RL_TACC_ARG);
        rl_wave_sync(); // (the shadow scan rewrites the wave's scratch)

        // ---- the rest of the path's loop body, the result of a path that ends, and the sample at the vertex ----
        RlLightDraw s;
        s.direction = s.origin = rl_f3(0.0f, 0.0f, 0.0f);
        s.distance = s.weight = s.t_max = 0.0f;
        s.emitter = RL_OBJECT_NONE;
        s.status = RL_LIGHT_SKIPPED;
        float splat = 0.0f; // what the lane puts on the film in this iteration: an ending's value, or the sample's unless its ray is blocked
        bool kept = false, dropped = false;
        const bool stepped = (segments & RL_DIRECT_FREE) == 0u; // the lanes that make a segment in this iteration
        if (stepped) {
            const RlDirectJob* job = &((const RlDirectQueue*)rl_opaque(queue))->job;
            const uint64_t seed = rl_direct_uniform64(job->seed);
            const uint64_t first = rl_direct_uniform64(job->first_path);
            const uint32_t stream = __builtin_amdgcn_readfirstlane(job->stream);
            RlPath p;
            p.origin = origin;
            p.direction = direction;
            p.wavelength = wavelength;
            p.intensity = *rl_direct_parked(ws, RL_DIRECT_INTENSITY, lane);
            p.continue_chance = *rl_direct_parked(ws, RL_DIRECT_CONTINUE, lane);
            p.ior = *rl_direct_parked(ws, RL_DIRECT_IOR, lane);
            p.sx = p.sy = 0.0f;
            // the hit record, as the step kernels write it for this segment: the sample's vertex
            const RlRayHit vertex = rl_ray_hit_of(sv, p.origin, p.direction, hit, hit.obj != RL_HIT_NONE);
            const bool sampled = (segments & RL_DIRECT_SAMPLED) != 0u;
            p.bounce = segments & ~RL_DIRECT_SAMPLED; // (the bounce draws block 2 + segments, as the step kernel has it: not held across the scans)
            segments = p.bounce + 1u;
            uint32_t emitter = RL_OBJECT_NONE;
            float value = 0.0f;
            const int status = rl_bounce(sv, seed, stream, first + my_path, &p, hit, &value, &emitter);
            origin = p.origin;
            direction = p.direction;
            *rl_direct_parked(ws, RL_DIRECT_INTENSITY, lane) = p.intensity;
            *rl_direct_parked(ws, RL_DIRECT_CONTINUE, lane) = p.continue_chance;
            const bool on_light = status == RL_PATH_ENDED_ON_EMITTER;
            if (on_light) value = rl_emission(sv, p.intensity, p.wavelength, emitter);
            const bool ended = status != RL_PATH_CONTINUES || segments >= __builtin_amdgcn_readfirstlane(job->max_segments);
            if (ended) {
                if (status == RL_PATH_CONTINUES) value = 0.0f; // (stopped by max_segments: no value)
                if (RlPathResult* res = job->results) res[my_path] = rl_ended_path_result(status, hit, value, segments, emitter);
            }
            if (on_light) {
                // the ending, unless the sample at the vertex before has counted this light
                if (value != 0.0f) {
                    bool counted = false;
                    if (sampled && emitter < job->n_objects) {
                        if (const uint8_t* flags = job->emitter_flags) counted = flags[emitter] != 0;
                    }
                    kept = !counted;
                    dropped = counted;
                    if (kept) splat = value;
                }
            } else {
                // `end` as it would stand in an RlPathState: a path that max_segments stops is live there
                const uint32_t end = status == RL_PATH_CONTINUES ? (uint32_t)RL_PATH_LIVE : hit.obj == RL_HIT_NONE ? (uint32_t)RL_PATH_END_VOID : (uint32_t)RL_PATH_END_ROULETTE;
                s = rl_light_sample(sv.objects, sv.n_objects, job->emitters, __builtin_amdgcn_readfirstlane(job->n_emitters), seed, stream, first + my_path, segments,
                                    end, p.wavelength, p.direction, rl_f3(vertex.isect.position.x, vertex.isect.position.y, vertex.isect.position.z),
                                    rl_f3(vertex.isect.normal.x, vertex.isect.normal.y, vertex.isect.normal.z), vertex.object);
                splat = p.intensity * s.weight; // state.intensity * weight: the sample's value unless the ray is blocked
            }
            if (s.status != (uint32_t)RL_LIGHT_SKIPPED) segments |= RL_DIRECT_SAMPLED;
            if (ended) segments |= RL_DIRECT_FREE; // (my_path and the wavelength stay for the splat: the refill comes behind it)
        }
        const bool cast = s.status == (uint32_t)RL_LIGHT_VISIBLE;
        rl_direct_count(ws, lane, RL_DIRECT_SEGMENTS, stepped);
        rl_direct_count(ws, lane, RL_DIRECT_LIGHT_SAMPLES, s.status != (uint32_t)RL_LIGHT_SKIPPED);
        rl_direct_count(ws, lane, RL_DIRECT_SHADOW_RAYS, cast);
        rl_direct_count(ws, lane, RL_DIRECT_KEPT, kept);
        rl_direct_count(ws, lane, RL_DIRECT_DROPPED, dropped);

        // ---- rl_scene_occluded for every lane's shadow ray ----
        const bool blocked = rl_occluded_segment<STAGE, CYL>(staged, lay, cast, s.origin, s.direction, s.t_max, ws, lane RL_TACC_ARG);
        rl_direct_count(ws, lane, RL_DIRECT_VISIBLE, blocked); // (only a ray that was cast is blocked: `cast` itself does not cross the scan)

        // ---- the splat, at the screen position the path's first draws give (rl_begin_path: p.sx, p.sy) ----
        if (blocked) splat = 0.0f;
        if (splat != 0.0f) {
            const RlDirectJob* job = &((const RlDirectQueue*)rl_opaque(queue))->job;
            const uint64_t seed = rl_direct_uniform64(job->seed);
            const uint64_t first = rl_direct_uniform64(job->first_path);
            const RlRngBlock b0 = rl_rng_block(seed, __builtin_amdgcn_readfirstlane(job->stream), first + my_path, 0);
            const float sx = rl_get_bi_unit(b0.w[1]);
            const float sy = rl_get_bi_unit(b0.w[2]) / job->aspect_ratio;
            const RlFilm film = job->film; // (written before the launch, never by the kernel)
            const RlF3 colour = rl_mul(rl_tristimulus(sv.records + film.off_cie, wavelength), splat); // (sv.cie)
            rl_film_splat(film.plot, colour, rl_splat_weights(film.width, film.height, film.wm1, film.hm1, film.aspect_ratio, sx, sy));
        }
        rl_wave_sync(); // (the next iteration's scan rewrites the wave's scratch)
    }
    // ---- the wave's totals, one atomic per counter ----
    rl_wave_sync();
    if (lane < (uint32_t)RL_DIRECT_COUNTERS) {
        unsigned long long total = 0;
        for (uint32_t i = 0; i < 64u; ++i) total += rl_direct_counters(ws)[lane * 64u + i];
        // (row RL_DIRECT_VISIBLE holds the blocked rays: the host takes them off the cast ones)
        if (total != 0ull) atomicAdd(((RlDirectQueue*)rl_opaque(queue))->stats + lane, total);
    }
}

template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_direct_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    rl_direct_body<STAGE, CYL>(scene, lay, queue);
}
