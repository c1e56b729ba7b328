// rl_light_film.hip.h -- the kernels behind rl_plot_unit_light_paths* and rl_plot_unit_render_samples_direct*: the light kernel
// (rl_light.hip.h) with a film.  What rl_light_kernel writes into a sample record this one splats where the value is produced, and it
// splats the value of a path that has just ended on a light unless the sample at the vertex before has already estimated it (the
// header's "counting light once").  Included by rl_api.hip after rl_light.hip.h, rl_film.hip.h (RlFilm, rl_film_splat) and
// rl_paths.hip.h (rl_opaque).
#pragma once

// What a launch reads beside the scene: RlLightJob's words, the three arrays a film needs and the film itself, all behind the
// launch's chunk counter for RlLightQueue's reason (launch constants passed as kernel arguments are scalar registers held across
// the persistent loop, and those spill).  A chunk loads each word where it uses it; nothing of the splat is held across the scan.
struct RlLightFilmJob {
    const RlPathState* states;    // n_states records; never written
    const RlRayHit* hits;         // n_states records, indexed by state; never written
    const uint32_t* list;         // null: the identity list
    const RlF4* emitters;         // the scene's emitter table (rl_core.h: RL_EMITTER_STRIDE records per emitter)
    RlLightSample* samples;       // null, or n_states records, indexed by state
    const RlCameraSample* camera; // n_states records, indexed by state: only x and y are read
    uint8_t* sampled;             // null, or n_states bytes, indexed by state: read, then written
    const uint8_t* emitter_flags; // null (a scene without a sampleable emitter), or one byte per object: 1 for the emitters of the table
    uint32_t n_list;
    uint32_t n_states;
    uint32_t n_emitters;
    uint32_t stream;
    uint64_t seed;
    uint32_t n_objects; // the length of emitter_flags
    uint32_t reserved;
    RlFilm film;
};
struct RlLightFilmQueue {
    unsigned long long next; // the chunk counter: zero at launch
    RlLightFilmJob job;
};

// rl_light_kernel's chunk (a copy of its text, as rl_list_step_chunk is of the step kernel's, so that the light kernel's
// instructions stay what they are) with three things behind the scan, under the listed lanes:
//   the sample record is stored only if `samples` is given;
//   the state's `sampled` byte is read and then written: 1 if a point was drawn (any status but RL_LIGHT_SKIPPED), else 0;
//   the splat: a visible sample's value; or the value of a state that ended on an emitter, unless the byte read was non-zero and
//   the emitter is one of the table's -- then the vertex before was sampled and that light has been counted.  A state gets one or
//   the other: a state that has ended on an emitter is never sampled.
// The splat's inputs -- the end, the value and the object of the state, its wavelength, the screen position -- are loaded again
// behind the scan from the buffers the block names: the loop's registers stay those of the light kernel.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_light_film_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif
    const uint32_t n_list = __builtin_amdgcn_readfirstlane(((const RlLightFilmQueue*)queue)->job.n_list); // (used up before the loop)
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_list + 63u) / 64u);
    const uint32_t slice = (uint64_t)n_list >= (uint64_t)gridDim.x * (RL_TRACE_BLOCK * 16ull) ? (uint32_t)(RL_CHUNK / 64ull) : 1u;
    uint32_t chunk_next = 0, chunk_left = 0; // wave-uniform: this wave's slice of the counter
    for (;;) {
        if (chunk_left == 0) {
            unsigned long long taken = 0;
            if (lane == 0) taken = atomicAdd(queue, (unsigned long long)slice);
            chunk_next = __builtin_amdgcn_readfirstlane((uint32_t)taken);
            chunk_left = slice;
        }
        const uint32_t c = chunk_next;
        if (c >= n_chunks) break;
        chunk_next += 1;
        chunk_left -= 1;
        const uint32_t k = c * 64u + lane; // the list position
        uint32_t i = k;
        bool listed;
        RlLightDraw s;
        float value = 0.0f;
        {
            const RlLightFilmJob* job = &((const RlLightFilmQueue*)rl_opaque(queue))->job;
            listed = k < job->n_list;
            if (const uint32_t* entries = job->list) {
                if (listed) i = entries[k];
            }
            listed = listed && i < job->n_states;
            if (!listed) i = 0u; // (no address is formed from an entry that was not checked)
            s.direction = s.origin = rl_f3(0.0f, 0.0f, 0.0f);
            s.distance = s.weight = s.t_max = 0.0f;
            s.emitter = RL_OBJECT_NONE;
            s.status = RL_LIGHT_SKIPPED;
            if (listed) {
                const RlF4* rec = (const RlF4*)(job->states + i);
                const RlF4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                const RlRayHit* h = job->hits + i;
                const RlF3 x = rl_f3(h->isect.position.x, h->isect.position.y, h->isect.position.z);
                const RlF3 normal = rl_f3(h->isect.normal.x, h->isect.normal.y, h->isect.normal.z);
                const uint64_t path = ((uint64_t)rl_f2u(q3.y) << 32) | rl_f2u(q3.x);
                // (the same in every lane: rl_rng.h wants the launch constants in scalar registers)
                const uint64_t seed = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(job->seed >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)job->seed);
                s = rl_light_sample(staged.sv.objects, staged.sv.n_objects, job->emitters, __builtin_amdgcn_readfirstlane(job->n_emitters), seed,
                                    __builtin_amdgcn_readfirstlane(job->stream), path, rl_f2u(q2.y), rl_f2u(q2.z), q0.w, rl_f3(q1.x, q1.y, q1.z), x,
                                    normal, h->object);
                value = q1.w * s.weight; // state.intensity * weight: the sample's value unless the ray is blocked
            }
        }
        const bool cast = listed && s.status == RL_LIGHT_VISIBLE;

        // ---- rl_scene_occluded for every lane's shadow ray ----
        const bool blocked = rl_occluded_segment<STAGE, CYL>(staged, lay, cast, s.origin, s.direction, s.t_max, ws, lane RL_TACC_ARG);

        if (listed) {
            const RlLightFilmJob* job = &((const RlLightFilmQueue*)rl_opaque(queue))->job;
            const bool lit = cast && !blocked;
            const uint32_t status = cast && blocked ? (uint32_t)RL_LIGHT_OCCLUDED : s.status;
            if (RlLightSample* samples = job->samples) {
                RlF4* out = (RlF4*)(samples + i);
                RlF4 r0, r1;
                r0.x = s.direction.x, r0.y = s.direction.y, r0.z = s.direction.z, r0.w = s.distance;
                r1.x = lit ? value : 0.0f;
                r1.y = s.weight;
                r1.z = rl_u2f(s.emitter);
                r1.w = rl_u2f(status);
                out[0] = r0;
                out[1] = r1;
            }
            uint32_t before = 0u; // the byte the call before this one left: was the vertex before this state's last segment sampled?
            if (uint8_t* sampled = job->sampled) {
                before = sampled[i];
                sampled[i] = status != (uint32_t)RL_LIGHT_SKIPPED ? (uint8_t)1 : (uint8_t)0;
            }
            // ---- the splat (none of its inputs crossed the scan but `value`, which the sample record needs anyway) ----
            const RlF4* rec = (const RlF4*)(job->states + i);
            const RlF4 q2 = rec[2];
            float splat = lit ? value : 0.0f;
            if (rl_f2u(q2.z) == (uint32_t)RL_PATH_END_EMITTER) {
                const uint32_t object = rl_f2u(rec[3].z);
                bool counted = false;
                if (before != 0u && object < job->n_objects) {
                    if (const uint8_t* flags = job->emitter_flags) counted = flags[object] != 0;
                }
                splat = counted ? 0.0f : q2.w;
            }
            if (splat != 0.0f) {
                const RlCameraSample* at = job->camera + i;
                const float sx = at->x, sy = at->y;
                // (a NaN or infinite position is sampled, not splatted: rl_film_photons_kernel's rule)
                if (fabsf(sx) < INFINITY && fabsf(sy) < INFINITY) {
                    const RlFilm film = job->film; // (written before the launch, never by the kernel)
                    const RlF3 colour = rl_mul(rl_tristimulus(staged.sv.records + film.off_cie, rec[0].w), splat); // (sv.cie)
                    rl_film_splat(film.plot, colour, rl_splat_weights(film.width, film.height, film.wm1, film.hm1, film.aspect_ratio, sx, sy));
                }
            }
        }
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
}

// ---- the two ends of rl_plot_unit_render_samples_direct*'s loop (grid-stride, one record per lane) ----

// rl_begin_paths_kernel for the rays of camera samples (48-byte records), which also clears the states' `sampled` bytes.
__global__ __launch_bounds__(RL_BLOCK) void rl_direct_begin_kernel(const RlCameraSample* __restrict__ camera, uint64_t first_path,
                                                                   RlPathState* __restrict__ states, uint8_t* __restrict__ sampled, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlF4* in = (const RlF4*)(camera + i);
        const RlF4 r0 = in[0], r1 = in[1];
        const uint64_t path = first_path + i;
        RlF4 q1 = r1, q2, q3;
        q1.w = 1.0f;           // intensity, trace_unit.rs:88
        q2.x = 1.0f;           // continue chance, trace_unit.rs:84
        q2.y = rl_u2f(0u);     // segments
        q2.z = rl_u2f(fabsf(r0.w) < INFINITY ? RL_PATH_LIVE : (uint32_t)RL_PATH_END_INVALID);
        q2.w = 0.0f;           // value
        q3.x = rl_u2f((uint32_t)path);
        q3.y = rl_u2f((uint32_t)(path >> 32));
        q3.z = rl_u2f(RL_OBJECT_NONE);
        q3.w = rl_u2f(0u);
        RlF4* out = (RlF4*)(states + i);
        out[0] = r0;
        out[1] = q1;
        out[2] = q2;
        out[3] = q3;
        sampled[i] = 0;
    }
}

// What rl_ray_paths_kernel writes for a path, from the state the loop left: a state that is still live used up max_segments.
__global__ __launch_bounds__(RL_BLOCK) void rl_direct_results_kernel(const RlPathState* __restrict__ states, RlPathResult* __restrict__ results,
                                                                     uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlF4* rec = (const RlF4*)(states + i);
        const RlF4 q2 = rec[2];
        const uint32_t end = rl_f2u(q2.z);
        const bool live = end == RL_PATH_LIVE;
        results[i] = rl_path_result(live ? 0.0f : q2.w, rl_f2u(q2.y), live ? RL_OBJECT_NONE : rl_f2u(rec[3].z), live ? (uint32_t)RL_PATH_END_LIMIT : end);
    }
}
