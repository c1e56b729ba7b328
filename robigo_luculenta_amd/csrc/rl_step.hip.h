// rl_step.hip.h -- the kernels behind rl_scene_begin_paths* and rl_scene_step_paths*: one turn of TraceUnit::render_ray's loop
// body (trace_unit.rs:92-126) for path states a caller holds between segments (RlPathState).  Included by rl_api.hip after
// rl_query.hip.h (rl_intersect_segment, rl_ray_hit_of) and rl_paths.hip.h (rl_opaque, RlChunkCursor).
#pragma once

// RlPathState as the kernels move it: four 16-byte words.
//   q0 = origin.xyz, wavelength      q1 = direction.xyz, intensity
//   q2 = continue_chance, segments, end, value      q3 = path_index (low, high), object, reserved
static_assert(sizeof(RlPathState) == 64 && offsetof(RlPathState, wavelength) == 12 && offsetof(RlPathState, direction) == 16 &&
                  offsetof(RlPathState, intensity) == 28 && offsetof(RlPathState, continue_chance) == 32 &&
                  offsetof(RlPathState, segments) == 36 && offsetof(RlPathState, end) == 40 && offsetof(RlPathState, value) == 44 &&
                  offsetof(RlPathState, path_index) == 48 && offsetof(RlPathState, object) == 56 && offsetof(RlPathState, reserved) == 60,
              "RlPathState is frozen: 16 words");

// The state of path `path` before its first segment, from the two 16-byte words of its ray (r0 = origin, wavelength; r1 =
// direction, a word that is not read).  A ray whose wavelength is NaN or infinite becomes a state that has ended
// (RL_PATH_END_INVALID), as rl_ray_paths_kernel ends it.
__device__ __forceinline__ void rl_store_begun_state(RlPathState* state, const RlF4& r0, const RlF4& r1, uint64_t path) {
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
    RlF4* out = (RlF4*)state;
    out[0] = r0;
    out[1] = q1;
    out[2] = q2;
    out[3] = q3;
}

// rl_scene_begin_paths: rays[i] as the state of path first_path + i before its first segment (grid-stride, one ray per lane).
__global__ __launch_bounds__(RL_BLOCK) void rl_begin_paths_kernel(const RlSpectralRay* __restrict__ rays, uint64_t first_path,
                                                                  RlPathState* __restrict__ states, uint32_t n) {
    // (64-bit: a 32-bit index plus the grid's stride wraps past 2^32 for n near 2^32, rl_camera_rays_kernel)
    for (uint64_t i = (uint64_t)blockIdx.x * RL_BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RL_BLOCK) {
        const RlF4* in = (const RlF4*)(rays + i);
        const RlF4 r0 = in[0], r1 = in[1];
        rl_store_begun_state(states + i, r0, r1, first_path + i);
    }
}

// One segment for the state a lane holds, the body of a chunk of rl_step_kernel and of rl_list_step_kernel (rl_path_list.hip.h):
// lane `lane` of the wave steps states[i] when `in_range` and the state is live, and idles through the scan as a null ray
// otherwise, as the path kernel's free lanes do, writing nothing.  The state's four 16-byte loads, every lane's segment
// (rl_intersect_segment), rl_bounce with RNG block 2 + segments, the emitter term inline under the lanes on a light, the hit
// record as the query kernel writes it (when `hits` is not null: tested through rl_opaque), and the state's four stores.  p.ior
// is a function of the wavelength alone: it is evaluated under the lanes whose hit is glass, which gives the bits the path
// kernel's per-path evaluation gives.  Returns whether the lane's state is live after the step.
// `consts` is where the launch's seed(), stream() and flags() come from, asked for where the value is used: kernel arguments
// (RlStepArgs) or words of a block in memory that are loaded there and not held across the scan (RlPathListConsts).
// flags: RL_STEP_NO_ROULETTE leaves a state live whose bounce the roulette would have ended.
template <int STAGE, bool CYL, class CONSTS>
__device__ __forceinline__ bool rl_step_chunk(const RlStagedScene& staged, const RlSceneLayout& lay, RlWaveScratch* ws, uint32_t lane,
                                              RlPathState* __restrict__ states, RlRayHit* __restrict__ hits, uint32_t i, bool in_range,
                                              const CONSTS& consts RL_TACC_PARAM) {
    const RlSceneView& sv = staged.sv;
    RL_T0(t_load);
    RlF4* rec = (RlF4*)(states + i);
    RlF4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, q1 = q0, q2 = q0, q3 = q0;
    bool live = false, live_after = false;
    if (in_range) {
        q0 = rec[0];
        q1 = rec[1];
        q2 = rec[2];
        q3 = rec[3];
        live = rl_f2u(q2.z) == RL_PATH_LIVE;
    }
    RL_T1(RL_ST_T_REFILL, t_load);
    RL_STAT(RL_ST_ITER, 1);
    RL_STAT(RL_ST_SCAN_LANES, __popcll(__builtin_amdgcn_ballot_w64(live)));
    RlPath p;
    p.origin = rl_f3(q0.x, q0.y, q0.z);
    p.direction = rl_f3(q1.x, q1.y, q1.z);
    p.wavelength = q0.w;
    p.intensity = q1.w;
    p.continue_chance = q2.x;
    p.sx = p.sy = 0.0f;
    p.ior = 1.0f;
    p.bounce = rl_f2u(q2.y); // the bounce draws block 2 + segments

    // ---- Scene::intersect for every lane's segment ----
    const RlHit hit = rl_intersect_segment<STAGE, CYL>(staged, lay, live, p.origin, p.direction, ws, lane RL_TACC_ARG);

    // ---- the hit record, as rl_query_kernel writes it for t_max = INFINITY ----
    RL_T0(t_camera);
    if (live) {
        if (RlRayHit* out_hits = rl_opaque(hits)) out_hits[i] = rl_ray_hit_of(sv, p.origin, p.direction, hit, hit.obj != RL_HIT_NONE);
    }
    RL_T1(RL_ST_T_CAMERA, t_camera);

    // ---- the rest of the loop body (trace_unit.rs:92-126) ----
    RL_T0(t_shade);
    int status = RL_PATH_CONTINUES;
    uint32_t emitter = RL_OBJECT_NONE;
    float value = 0.0f;
    if (live) {
        if (hit.obj != RL_HIT_NONE && rl_object_material(rl_f2u(sv.objects[hit.obj].w)) == RL_MATERIAL_SF10_GLASS)
            p.ior = rl_sf10_ior(p.wavelength);
        const uint64_t path = ((uint64_t)rl_f2u(q3.y) << 32) | rl_f2u(q3.x);
        status = rl_bounce(sv, consts.seed(), consts.stream(), path, &p, hit, &value, &emitter);
    }
    RL_T1(RL_ST_T_SHADE, t_shade);
    RL_T0(t_emit);
    const bool on_light = status == RL_PATH_ENDED_ON_EMITTER;
    RL_STAT(RL_ST_END_EMITTER, __popcll(__builtin_amdgcn_ballot_w64(on_light)));
    if (on_light) value = rl_emission(sv, p.intensity, p.wavelength, emitter);
    if (live) {
        uint32_t end = RL_PATH_LIVE;
        if (on_light) end = RL_PATH_END_EMITTER;
        else if (hit.obj == RL_HIT_NONE) end = RL_PATH_END_VOID;
        else if (status == RL_PATH_ENDED && !(consts.flags() & RL_STEP_NO_ROULETTE)) end = RL_PATH_END_ROULETTE;
        q0.x = p.origin.x, q0.y = p.origin.y, q0.z = p.origin.z;
        q1.x = p.direction.x, q1.y = p.direction.y, q1.z = p.direction.z;
        q1.w = p.intensity;
        q2.x = p.continue_chance;
        q2.y = rl_u2f(rl_f2u(q2.y) + 1u);
        q2.z = rl_u2f(end);
        live_after = end == RL_PATH_LIVE;
        q2.w = on_light ? value : 0.0f;
        q3.z = rl_u2f(on_light ? emitter : RL_OBJECT_NONE);
        q3.w = rl_u2f(0u);
        rec[0] = q0;
        rec[1] = q1;
        rec[2] = q2;
        rec[3] = q3;
    }
    RL_T1(RL_ST_T_EMIT, t_emit);
    return live_after;
}

// The step kernel's launch constants: its arguments.
struct RlStepArgs {
    uint64_t seed_;
    uint32_t stream_, flags_;
    __device__ __forceinline__ uint64_t seed() const { return seed_; }
    __device__ __forceinline__ uint32_t stream() const { return stream_; }
    __device__ __forceinline__ uint32_t flags() const { return flags_; }
};

// One segment for every live state of states[0, n).  The work per call is one scan per record, so the kernel has the query kernel's
// shape, not the path kernel's: persistent workgroups of RL_TRACE_BLOCK threads that stage the scene once (rl_stage_scene), every
// wave taking chunks of 64 states from one counter (`queue`, zeroed on the call's stream: RlChunkCursor) and scanning them
// together (rl_step_chunk), no refill.  Lanes past the end idle.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_step_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, RlPathState* __restrict__ states, RlRayHit* __restrict__ hits, uint32_t n_states,
    uint64_t seed, uint32_t stream, uint32_t flags, unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the diagnostic build: reported to rl_stat_counters at the end, as the path kernel does)
#endif
    const RlStepArgs consts = {seed, stream, flags};
    RlChunkCursor chunks(n_states);
    RL_T0(t_total);
    for (;;) {
        RL_T0(t_refill);
        uint32_t c;
        if (!chunks.next(queue, lane, &c)) break;
        const uint32_t i = c * 64u + lane;
        RL_T1(RL_ST_T_REFILL, t_refill);
        rl_step_chunk<STAGE, CYL>(staged, lay, ws, lane, states, hits, i, i < n_states, consts RL_TACC_ARG);
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
    RL_T1(RL_ST_T_TOTAL, t_total);
#ifdef RL_STATS
    if (lane == 0)
        for (int k = 0; k < RL_ST_COUNT; ++k) atomicAdd(&rl_stat_counters[k], st[k]);
#endif
}
