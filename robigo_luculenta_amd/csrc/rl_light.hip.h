// rl_light.hip.h -- the kernel behind rl_scene_light_paths*: one direct-light sample for the path states an index list names.  The
// list-step kernel's chunk loop (rl_path_list.hip.h) around the occlusion kernel's bounded any-hit scan (rl_occlusion.hip.h): a
// lane loads its state and the hit record of the state's last segment, draws an emitter and a point on it (rl_core.h:
// rl_light_sample, the arithmetic of the header's contract), the wave scans every lane's shadow ray at once, and the lane stores
// its 32-byte sample.  With a film (rl_light_film.hip.h: rl_light_film_kernel is the same body) the lane also splats.  Included by
// rl_api.hip after rl_occlusion.hip.h (rl_occluded_segment), rl_film.hip.h (RlFilm, rl_film_splat), rl_paths.hip.h (rl_opaque,
// RlChunkCursor) and rl_path_list.hip.h (rl_listed_index).
#pragma once

// What a launch reads beside the scene: its buffers too (with the states and the hits as kernel arguments the variants that do not
// stage the whole scene spilled 32, 35, 19 and 19 scalar registers; with them in the block 22, 23, 14 and 15, against the list-step
// kernel's 22, 24, 15 and 16).  Behind the launch's chunk counter, as RlPathListQueue's block
// is and for its reason: launch constants passed as kernel arguments are scalar registers held across the persistent loop, and
// those spill (rl_path_list.hip.h).  A chunk loads each word where it uses it.
struct RlLightJob {
    const RlPathState* states; // n_states records; never written
    const RlRayHit* hits;      // n_states records, indexed by state; never written
    const uint32_t* list;   // null: the identity list
    const RlF4* emitters;   // the scene's emitter table: RL_EMITTER_STRIDE records per emitter (rl_core.h)
    RlLightSample* samples; // n_states records, indexed by state
    uint32_t n_list;
    uint32_t n_states;
    uint32_t n_emitters;
    uint32_t stream;
    uint64_t seed;
};
struct RlLightQueue {
    unsigned long long next; // the chunk counter: zero at launch
    RlLightJob job;
};

// What a launch with a film reads: RlLightJob's words, then the three arrays a film needs and the film itself, behind the chunk
// counter for the same reason.  Nothing of the splat is held across the scan.
struct RlLightFilmJob {
    RlLightJob light;             // (`samples` may be null here)
    const RlCameraSample* camera; // n_states records, indexed by state: only x and y are read
    uint8_t* sampled;             // null, or n_states bytes, indexed by state: read, then written
    const uint8_t* emitter_flags; // null (a scene without a sampleable emitter), or one byte per object: 1 for the emitters of the table
    uint32_t n_objects;           // the length of emitter_flags
    uint32_t reserved;
    RlFilm film;
};
struct RlLightFilmQueue {
    unsigned long long next; // the chunk counter: zero at launch
    RlLightFilmJob job;
};
// rl_light_body reads either queue as an RlLightFilmQueue: without a film only job.light is there.
static_assert(offsetof(RlLightFilmQueue, job.light) == offsetof(RlLightQueue, job) && offsetof(RlLightFilmJob, light) == 0 &&
                  sizeof(RlLightJob) == 64 && offsetof(RlLightFilmJob, camera) == 64 && offsetof(RlLightJob, samples) == 32 &&
                  offsetof(RlLightJob, n_list) == 40 && offsetof(RlLightJob, seed) == 56,
              "an RlLightQueue is the beginning of an RlLightFilmQueue");

// The body of rl_light_kernel (FILM == false) and rl_light_film_kernel (rl_light_film.hip.h).  Chunk c is list positions c * 64 ..
// c * 64 + 63; lane l samples for states[list[c * 64 + l]] (state c * 64 + l when the list is null).  An entry that is not below
// n_states is skipped like a position past the end of the list: the lane idles through the scan and touches no memory.  The
// emitter record is a per-lane gather from the table in global memory (the lanes draw different emitters; the table is a few
// records and stays in L2).  Lanes that cast no ray -- skipped states, points that do not face the vertex -- go through the scan
// inactive, as the occlusion kernel's lanes past the end do.
// FILM: three things more behind the scan, under the listed lanes:
//   the sample record is stored only if `samples` is given;
//   the state's `sampled` byte is read and then written: 1 if a point was drawn (any status but RL_LIGHT_SKIPPED), else 0;
//   the splat: a visible sample's value; or the value of a state that ended on an emitter, unless the byte read was non-zero and
//   the emitter is one of the table's -- then the vertex before was sampled and that light has been counted (the header's
//   "counting light once").  A state gets one or the other: a state that has ended on an emitter is never sampled.
// The splat's inputs -- the end, the value and the object of the state, its wavelength, the screen position -- are loaded again
// behind the scan from the buffers the block names: the loop's registers are the same with and without a film.
template <int STAGE, bool CYL, bool FILM>
__device__ __forceinline__ void rl_light_body(const RlF4* __restrict__ scene, const RlSceneLayout& lay, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif
    RlChunkCursor chunks(__builtin_amdgcn_readfirstlane(((const RlLightQueue*)queue)->job.n_list)); // (n_list: used up before the loop)
    for (;;) {
        uint32_t c;
        if (!chunks.next(queue, lane, &c)) break;
        RlListed entry;
        RlLightDraw s;
        float value = 0.0f;
        {
            const RlLightJob* job = &((const RlLightFilmQueue*)rl_opaque(queue))->job.light;
            entry = rl_listed_index(job, c * 64u + lane);
            s.direction = s.origin = rl_f3(0.0f, 0.0f, 0.0f);
            s.distance = s.weight = s.t_max = 0.0f;
            s.emitter = RL_OBJECT_NONE;
            s.status = RL_LIGHT_SKIPPED;
            if (entry.listed) {
                const RlF4* rec = (const RlF4*)(job->states + entry.i);
                const RlF4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                const RlRayHit* h = job->hits + entry.i;
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
        const bool cast = entry.listed && s.status == RL_LIGHT_VISIBLE;

        // ---- rl_scene_occluded for every lane's shadow ray ----
        const bool blocked = rl_occluded_segment<STAGE, CYL>(staged, lay, cast, s.origin, s.direction, s.t_max, ws, lane RL_TACC_ARG);

        if (entry.listed) {
            const RlLightFilmJob* job = &((const RlLightFilmQueue*)rl_opaque(queue))->job;
            const bool lit = cast && !blocked;
            const uint32_t status = cast && blocked ? (uint32_t)RL_LIGHT_OCCLUDED : s.status;
            if (RlLightSample* samples = job->light.samples; !FILM || samples) {
                RlF4* out = (RlF4*)(samples + entry.i);
                RlF4 r0, r1;
                r0.x = s.direction.x, r0.y = s.direction.y, r0.z = s.direction.z, r0.w = s.distance;
                r1.x = lit ? value : 0.0f;
                r1.y = s.weight;
                r1.z = rl_u2f(s.emitter);
                r1.w = rl_u2f(status);
                out[0] = r0;
                out[1] = r1;
            }
            if constexpr (FILM) {
                uint32_t before = 0u; // the byte the call before this one left: was the vertex before this state's last segment sampled?
                if (uint8_t* sampled = job->sampled) {
                    before = sampled[entry.i];
                    sampled[entry.i] = status != (uint32_t)RL_LIGHT_SKIPPED ? (uint8_t)1 : (uint8_t)0;
                }
                // ---- the splat (none of its inputs crossed the scan but `value`, which the sample record needs anyway) ----
                const RlF4* rec = (const RlF4*)(job->light.states + entry.i);
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
                    const RlCameraSample* at = job->camera + entry.i;
                    const float sx = at->x, sy = at->y;
                    // (a NaN or infinite position is sampled, not splatted: rl_film_photons_kernel's rule)
                    if (fabsf(sx) < INFINITY && fabsf(sy) < INFINITY) {
                        const RlFilm film = job->film; // (written before the launch, never by the kernel)
                        const RlF3 colour = rl_mul(rl_tristimulus(staged.sv.records + film.off_cie, rec[0].w), splat); // (sv.cie)
                        rl_film_splat(film.plot, colour, rl_splat_weights(film.width, film.height, film.wm1, film.hm1, film.aspect_ratio, sx, sy));
                    }
                }
            }
        }
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
}

template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_light_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    rl_light_body<STAGE, CYL, false>(scene, lay, queue);
}
