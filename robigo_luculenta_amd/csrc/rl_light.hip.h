// rl_light.hip.h -- the kernel behind rl_scene_light_paths*: one direct-light sample for the path states an index list names.  The
// list-step kernel's chunk loop (rl_path_list.hip.h) around the occlusion kernel's bounded any-hit scan (rl_occlusion.hip.h): a
// lane loads its state and the hit record of the state's last segment, draws an emitter and a point on it (rl_core.h:
// rl_light_sample, the arithmetic of the header's contract), the wave scans every lane's shadow ray at once, and the lane stores
// its 32-byte sample.  Nothing but `samples` is written.  Included by rl_api.hip after rl_occlusion.hip.h (rl_occluded_segment)
// and rl_path_list.hip.h.
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

// Chunk c is list positions c * 64 .. c * 64 + 63; lane l samples for states[list[c * 64 + l]] (state c * 64 + l when the list is
// null).  An entry that is not below n_states is skipped like a position past the end of the list: the lane idles through the
// scan and touches no memory.  The emitter record is a per-lane gather from the table in global memory (the lanes draw different
// emitters; the table is a few records and stays in L2).  Lanes that cast no ray -- skipped states, points that do not face the
// vertex -- go through the scan inactive, as the occlusion kernel's lanes past the end do.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_light_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif
    const uint32_t n_list = __builtin_amdgcn_readfirstlane(((const RlLightQueue*)queue)->job.n_list); // (used up before the loop)
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
            const RlLightJob* job = &((const RlLightQueue*)rl_opaque(queue))->job;
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
            const bool lit = cast && !blocked;
            RlF4* out = (RlF4*)(((const RlLightQueue*)rl_opaque(queue))->job.samples + i);
            RlF4 r0, r1;
            r0.x = s.direction.x, r0.y = s.direction.y, r0.z = s.direction.z, r0.w = s.distance;
            r1.x = lit ? value : 0.0f;
            r1.y = s.weight;
            r1.z = rl_u2f(s.emitter);
            r1.w = rl_u2f(cast && blocked ? (uint32_t)RL_LIGHT_OCCLUDED : s.status);
            out[0] = r0;
            out[1] = r1;
        }
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
}
