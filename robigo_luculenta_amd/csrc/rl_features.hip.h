// rl_features.hip.h -- the kernel behind rl_scene_render_features: the denoising guides of camera paths of the RNG -- albedo,
// shading normal and depth of what each pixel shows -- into up to three films, in one persistent launch.  rl_direct_body
// (rl_direct.hip.h) without the light: every wave is a pool of 64 lanes that refill as their feature paths end; per iteration
// every lane's segment (rl_intersect_segment), the hit record rl_ray_hit_of makes and rl_bounce, whose roulette is ignored
// (RL_STEP_NO_ROULETTE); then, under the lanes whose feature path has ended -- in the void, on a light, on a diffuse surface or at
// max_segments -- the record and the splats.  What the loop of public calls keeps in RlPathState and RlRayHit stays in the wave
// here: in registers, and in the part of its scratch that no scan uses (rl_feature_counters, rl_feature_parked).  Included by
// rl_api.hip after rl_direct.hip.h (rl_direct_uniform64; and what that header needs: RlFilm's splat, rl_opaque, rl_ray_hit_of).
#pragma once

// What a launch reads beside the scene, behind its queue counter as RlDirectQueue's block is and for its reason: the loop loads
// each word where it uses it.  The three films have one size, so one set of splat constants serves them.
struct RlFeatureJob {
    RlFeatureSample* records; // null, or n_paths records
    float* albedo;            // null, or a plot unit's buffer, width x height x 3
    float* normal;
    float* aux;
    uint64_t seed;
    uint64_t first_path;      // the launch's path i is path first_path + i of the stream
    uint32_t n_paths;         // of this launch
    uint32_t stream;
    uint32_t max_segments;    // resolved: 1 .. RL_PATH_MAX_SEGMENTS_CAP
    uint32_t width, height;
    float wm1, hm1;           // (float)width - 1, (float)height - 1 (plot_unit.rs:60-61)
    float aspect_ratio;       // the camera's and the films': (float)width / (float)height
    uint32_t off_cie;         // RlSceneLayout::off_cie
};
// The counters of RlFeatureStats but `paths`, in its order: the segments, then one per RlFeatureKind.
enum { RL_FEATURE_SEGMENTS, RL_FEATURE_KINDS, RL_FEATURE_COUNTERS = RL_FEATURE_KINDS + 4 };
struct RlFeatureQueue {
    unsigned long long next; // the queue counter, in path indices of the launch: zero at launch
    RlFeatureJob job;
    // Every wave adds its totals here when it leaves the loop.  The host zeroes them once per call, not per launch: the launches
    // of one call add up.
    unsigned long long stats[RL_FEATURE_COUNTERS];
};

// Where the counters of a wave live between its iterations: one 64-bit total per lane and counter in the part of the wave's
// scratch that only the trace kernel uses (RlWaveScratch::stash and ::emit, as rl_direct_counters has them).  Behind them, one
// slot per lane each: what a path carries from bounce to bounce and no scan reads -- its intensity, its continue chance, its
// index of refraction -- and the distance of its first segment's hit, which waits there for the record.  No LDS is added.
enum { RL_FEATURE_INTENSITY, RL_FEATURE_CONTINUE, RL_FEATURE_IOR, RL_FEATURE_DEPTH, RL_FEATURE_PARKED };
static_assert(sizeof(((RlWaveScratch*)0)->stash) + sizeof(((RlWaveScratch*)0)->emit) >=
                  RL_FEATURE_COUNTERS * 64 * sizeof(unsigned long long) + RL_FEATURE_PARKED * 64 * sizeof(float),
              "the feature kernel's counters and parked path state take the trace kernel's stash and emitter queue");
__device__ __forceinline__ RlLdsU64* rl_feature_counters(RlWaveScratch* ws) { return (RlLdsU64*)&ws->stash[0][0]; }
__device__ __forceinline__ RlLdsF* rl_feature_parked(RlWaveScratch* ws, int k, uint32_t lane) {
    return (RlLdsF*)(rl_feature_counters(ws) + RL_FEATURE_COUNTERS * 64) + (k * 64 + lane);
}

// In `segments`, above the count (at most RL_PATH_MAX_SEGMENTS_CAP): the lane has no path.
#define RL_FEATURE_FREE 0x40000000u

// Termination: a lane's feature path makes at most max_segments segments (`ended` below), every iteration with a path in some lane
// makes a segment for it, and an iteration without one either takes indices from the queue, which only grows, or leaves.  A wave
// waits for nothing but its own loads: no spins, no flags, no grid barrier.
template <int STAGE, bool CYL>
__device__ __forceinline__ void rl_feature_body(const RlF4* __restrict__ scene, const RlSceneLayout& lay, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const RlSceneView& sv = staged.sv;
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif
#pragma unroll
    for (int k = 0; k < RL_FEATURE_COUNTERS; ++k) rl_feature_counters(ws)[k * 64 + lane] = 0ull; // (the LDS holds whatever the kernel before left)
#pragma unroll
    for (int k = 0; k < RL_FEATURE_PARKED; ++k) *rl_feature_parked(ws, k, lane) = 0.0f;
    // Wave-uniform: the next index of this wave's slice of the queue (rl_direct_body).  32 bits: a launch has at most 2^30 paths
    // (rl_api.hip: RL_FEATURE_LAUNCH), and the counter stays below that plus a slice for every wave of the grid.
    uint32_t chunk_next = 0;
    uint32_t my_path = 0, segments = RL_FEATURE_FREE;
    // What of the path crosses the scan in registers: the segment and the wavelength (rl_feature_parked has the rest).
    RlF3 origin = rl_f3(0.0f, 0.0f, 0.0f), direction = rl_f3(0.0f, 0.0f, 0.0f);
    float wavelength = 0.0f;
    for (;;) {
        // ---- hand path indices to the lanes without a path (rl_direct_body's refill) ----
        const uint64_t need = __builtin_amdgcn_ballot_w64((segments & RL_FEATURE_FREE) != 0u);
        if (need != 0) {
            const RlFeatureJob* job = &((const RlFeatureQueue*)rl_opaque(queue))->job;
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
                if ((segments & RL_FEATURE_FREE) != 0u && idx < n_paths) {
                    const uint64_t seed = rl_direct_uniform64(job->seed);
                    const uint64_t first = rl_direct_uniform64(job->first_path);
                    my_path = idx;
                    segments = 0;
                    RlPath fresh;
                    rl_begin_path(sv, job->aspect_ratio, seed, __builtin_amdgcn_readfirstlane(job->stream), first + idx, &fresh);
                    origin = fresh.origin;
                    direction = fresh.direction;
                    wavelength = fresh.wavelength;
                    *rl_feature_parked(ws, RL_FEATURE_INTENSITY, lane) = fresh.intensity;
                    *rl_feature_parked(ws, RL_FEATURE_CONTINUE, lane) = fresh.continue_chance;
                    *rl_feature_parked(ws, RL_FEATURE_IOR, lane) = fresh.ior;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64((segments & RL_FEATURE_FREE) == 0u) == 0) break; // (nothing was handed out: the wave's slice is past the end)

        // ---- Scene::intersect for every lane's segment ----
        const bool stepped = (segments & RL_FEATURE_FREE) == 0u; // the lanes that make a segment in this iteration
        const RlHit hit = rl_intersect_segment<STAGE, CYL>(staged, lay, stepped, origin, direction, ws, lane RL_TACC_ARG);

        // ---- the step (rl_step_chunk under RL_STEP_NO_ROULETTE), and which rule ends the feature path ----
        __hip_atomic_fetch_add(rl_feature_counters(ws) + (RL_FEATURE_SEGMENTS * 64 + lane), stepped ? 1ull : 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (stepped) {
            const RlFeatureJob* job = &((const RlFeatureQueue*)rl_opaque(queue))->job;
            const uint64_t seed = rl_direct_uniform64(job->seed);
            const uint64_t first = rl_direct_uniform64(job->first_path);
            const uint32_t stream = __builtin_amdgcn_readfirstlane(job->stream);
            RlPath p;
            p.origin = origin;
            p.direction = direction;
            p.wavelength = wavelength;
            p.intensity = *rl_feature_parked(ws, RL_FEATURE_INTENSITY, lane);
            p.continue_chance = *rl_feature_parked(ws, RL_FEATURE_CONTINUE, lane);
            p.ior = *rl_feature_parked(ws, RL_FEATURE_IOR, lane);
            p.sx = p.sy = 0.0f;
            const bool found = hit.obj != RL_HIT_NONE;
            if (segments == 0u) *rl_feature_parked(ws, RL_FEATURE_DEPTH, lane) = found ? hit.t : 0.0f; // (the camera ray is unit length)
            // the hit record, as the step kernels write it for this segment: the feature vertex's normal
            const RlRayHit vertex = rl_ray_hit_of(sv, p.origin, p.direction, hit, found);
            const RlF3 arriving = p.direction;
            p.bounce = segments; // (the bounce draws block 2 + segments, as the step kernel has it)
            segments += 1u;
            uint32_t emitter = RL_OBJECT_NONE;
            float value = 0.0f;
            const int status = rl_bounce(sv, seed, stream, first + my_path, &p, hit, &value, &emitter); // (RL_PATH_ENDED on a hit: the roulette, ignored)
            origin = p.origin;
            direction = p.direction;
            *rl_feature_parked(ws, RL_FEATURE_INTENSITY, lane) = p.intensity;
            *rl_feature_parked(ws, RL_FEATURE_CONTINUE, lane) = p.continue_chance;
            // the first rule that applies
            bool diffuse = false;
            if (found) {
                const uint32_t material = rl_object_material(rl_f2u(sv.objects[hit.obj].w));
                diffuse = material == RL_MATERIAL_DIFFUSE_GREY || material == RL_MATERIAL_DIFFUSE_COLOURED;
            }
            const bool limit = segments >= __builtin_amdgcn_readfirstlane(job->max_segments);
            const uint32_t kind = !found ? (uint32_t)RL_FEATURE_VOID : status == RL_PATH_ENDED_ON_EMITTER ? (uint32_t)RL_FEATURE_EMITTER : diffuse ? (uint32_t)RL_FEATURE_DIFFUSE : (uint32_t)RL_FEATURE_LIMIT;
            const bool ended = kind != (uint32_t)RL_FEATURE_LIMIT || limit;
            if (ended) {
                const bool surface = kind == (uint32_t)RL_FEATURE_EMITTER || kind == (uint32_t)RL_FEATURE_DIFFUSE;
                // state.intensity: what reached the light (the step leaves it as it was), or the product up to and including the diffuse bounce
                const float albedo = surface ? p.intensity : 0.0f;
                RlF3 n = rl_f3(0.0f, 0.0f, 0.0f);
                if (surface) {
                    n = rl_f3(vertex.isect.normal.x, vertex.isect.normal.y, vertex.isect.normal.z);
                    if (!(rl_dot(arriving, n) < 0.0f)) n = rl_neg(n); // rl_bounce's `facing`
                }
                const float depth = *rl_feature_parked(ws, RL_FEATURE_DEPTH, lane);
                // the screen position the path's first draws give (rl_begin_path: p.sx, p.sy)
                const RlRngBlock b0 = rl_rng_block(seed, stream, first + my_path, 0);
                const float sx = rl_get_bi_unit(b0.w[1]);
                const float sy = rl_get_bi_unit(b0.w[2]) / job->aspect_ratio;
                if (RlFeatureSample* records = job->records) {
                    RlF4* rec = (RlF4*)(records + my_path);
                    rec[0] = RlF4{sx, sy, wavelength, albedo};
                    rec[1] = RlF4{n.x, n.y, n.z, depth};
                    rec[2] = RlF4{rl_u2f(surface ? hit.obj : (uint32_t)RL_OBJECT_NONE), rl_u2f(segments), rl_u2f(kind), rl_u2f(0u)};
                }
                const RlSplat splat = rl_splat_weights(job->width, job->height, job->wm1, job->hm1, job->aspect_ratio, sx, sy);
                if (float* film = job->albedo) {
                    if (albedo != 0.0f) rl_film_splat(film, rl_mul(rl_tristimulus(sv.records + job->off_cie, wavelength), albedo), splat); // (sv.cie)
                }
                if (float* film = job->normal) {
                    if (surface) rl_film_splat(film, n, splat);
                }
                if (float* film = job->aux) rl_film_splat(film, rl_f3(1.0f, depth, (float)segments), splat);
                __hip_atomic_fetch_add(rl_feature_counters(ws) + ((RL_FEATURE_KINDS + kind) * 64u + lane), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                segments = RL_FEATURE_FREE;
            }
        }
        rl_wave_sync(); // (the next iteration's scan rewrites the wave's scratch)
    }
    // ---- the wave's totals, one atomic per counter ----
    rl_wave_sync();
    if (lane < (uint32_t)RL_FEATURE_COUNTERS) {
        unsigned long long total = 0;
        for (uint32_t i = 0; i < 64u; ++i) total += rl_feature_counters(ws)[lane * 64u + i];
        if (total != 0ull) atomicAdd(((RlFeatureQueue*)rl_opaque(queue))->stats + lane, total);
    }
}

template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_feature_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    rl_feature_body<STAGE, CYL>(scene, lay, queue);
}
