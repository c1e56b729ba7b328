// rl_paths.hip.h -- the kernels behind rl_scene_camera_rays* and rl_scene_render_rays*: the two halves of a path of
// TraceUnit::render (trace_unit.rs:136-158 and 81-132), on rays a caller supplies.  Included by rl_api.hip after rl_query.hip.h
// (rl_stage_scene, rl_query_exhaustive) and the public header (RlSpectralRay, RlCameraSample, RlPathResult).
#pragma once

// Paths that hit a light: 0 evaluates their emitter term (the f64 Planck evaluation) inline, under the lanes that need it, in the
// iteration they end in; 1 queues them as the trace kernel does and evaluates 64 at a time.  Measured in DESIGN.md.
#ifndef RL_PATHS_EMIT_QUEUE
#define RL_PATHS_EMIT_QUEUE 0
#endif

// The path kernel's prologue: rl_query_kernel's, statement for statement (and the trace kernel's own, rl_trace_body): the
// workgroup stages the whole scene, its tables or nothing in LDS, ring T goes in front of the per-wave scratch where the cull table
// has a third level, and the scene view points into whichever copy holds each array.  (The query kernel keeps its copy: called
// from it, this function changed the query kernel's instructions.)
struct RlStagedScene {
    RlSceneView sv;
    const RlF4* base;       // the tables
    uint32_t tab0;          // blob offset of `base`'s first record
    RlWaveScratch* scratch; // RL_TRACE_BLOCK / 64 blocks, 512-byte aligned
    RlLdsU32* ring_t;       // this wave's ring T, or null
};
template <int STAGE>
__device__ __forceinline__ RlStagedScene rl_stage_scene(const RlF4* __restrict__ scene, const RlSceneLayout& lay) {
    extern __shared__ __attribute__((aligned(512))) RlF4 smem[]; // (512: the ring pushes OR slot offsets into a wave's scratch address)
    const RlF4* base = scene; // the tables
    const RlF4* big = scene;  // the per-sphere and per-object arrays
    RlWaveScratch* scratch = (RlWaveScratch*)smem;
    if (STAGE == RL_STAGE_ALL) {
        for (uint32_t i = threadIdx.x; i < lay.total_f4; i += RL_TRACE_BLOCK) smem[i] = scene[i];
        __syncthreads();
        base = big = smem;
        scratch = (RlWaveScratch*)(smem + ((lay.total_f4 + 31u) & ~31u));
    } else if (STAGE == RL_STAGE_TABLES) {
        const uint32_t n_staged = lay.off_objects - lay.off_planes;
        for (uint32_t i = threadIdx.x; i < n_staged; i += RL_TRACE_BLOCK) smem[i] = scene[lay.off_planes + i];
        __syncthreads();
        base = smem;
        scratch = (RlWaveScratch*)(smem + ((n_staged + 31u) & ~31u));
    }
    RlLdsU32* ring_t = nullptr;
    if (STAGE != RL_STAGE_ALL && lay.n_cluster_supers != 0u) {
        ring_t = (RlLdsU32*)scratch + 128u * (threadIdx.x >> 6);
        scratch = (RlWaveScratch*)((RlF4*)scratch + 32u * (RL_TRACE_BLOCK / 64));
    }
    const uint32_t tab0 = STAGE == RL_STAGE_TABLES ? lay.off_planes : 0u; // blob offset of `base`'s first record

    RlSceneView sv;
    sv.spheres = big;
    sv.planes = base + (lay.off_planes - tab0);
    sv.parabs = base + (lay.off_parabs - tab0);
    sv.prisms = base + (lay.off_prisms - tab0);
    sv.objects = big + lay.off_objects;
    sv.cie = big + lay.off_cie;
    sv.sphere_obj = (const uint32_t*)(big + lay.off_sphere_obj);
    sv.sphere_r2 = (const float*)(big + lay.off_sphere_r2);
    sv.n_direct = lay.n_direct;
    sv.n_direct_padded = lay.n_direct_padded;
    sv.cluster_base = lay.cluster_base;
    sv.n_clusters = lay.n_clusters;
    sv.cluster_k = lay.cluster_k;
    sv.n_planes = lay.n_planes;
    sv.n_parabs = lay.n_parabs;
    sv.n_prisms = lay.n_prisms;
    sv.n_objects = lay.n_objects;
    sv.camera_rec = base + (lay.off_camera - tab0);
    sv.records = big;
    RlStagedScene st;
    st.sv = sv;
    st.base = base;
    st.tab0 = tab0;
    st.scratch = scratch;
    st.ring_t = ring_t;
    return st;
}

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

// The path half: TraceUnit::render_ray for rays[i] as path first_path + i.  Persistent workgroups laid out as the query kernel's
// (rl_stage_scene; the same scan options), every wave a pool of 64 lanes that refill as their paths end: at the top of every
// iteration, with the wave converged, the lanes without a path take the next ray indices of the wave's slice of the call's queue
// (`queue`, zeroed on the call's stream; a slice is RL_CHUNK or 64 indices, as the trace kernel takes them), assigned by mbcnt.
// Without the refill a wave would run as long as its longest path (glass paths have long tails).  Per iteration: the wave's scan
// with the full exec mask (free lanes and lanes on the exhaustive path idle), the exact linear scan for the segments the culls do
// not cover (decided per segment: refraction and reflection keep a non-unit direction's length), rl_bounce, and for a path that
// hit a light the emitter term (the f64 Planck evaluation) inline, under the few lanes that need it.  A path that ends writes its
// RlPathResult.  max_segments: 1 .. RL_PATH_MAX_SEGMENTS_CAP (the host resolves 0).
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_ray_paths_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlSpectralRay* __restrict__ rays, RlPathResult* __restrict__ results,
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
#if RL_PATHS_EMIT_QUEUE
    // The trace kernel's emitter queue (measured against the inline form): paths that hit a light wait in the wave's
    // scratch (rows: ray index, segments, wavelength, intensity, emitter) until 64 can be evaluated with a full exec mask.
    typedef __attribute__((address_space(3))) float RlLdsF32;
    RlLdsF32* emit = (RlLdsF32*)&ws->emit[0][0];
    uint32_t e_head = 0, e_tail = 0; // wave-uniform
    auto process_emitted = [&](uint32_t count) {
        RL_STAT(RL_ST_EMIT_BATCHES, 1);
        RL_STAT(RL_ST_EMIT_LANES, count);
        rl_wave_sync();
        if (lane < count) {
            const uint32_t slot = (e_head + lane) & 63u;
            const uint32_t obj = rl_f2u(emit[4 * 64 + slot]);
            RlPathResult out;
            out.value = rl_emission(sv, emit[3 * 64 + slot], emit[2 * 64 + slot], obj);
            out.segments = rl_f2u(emit[1 * 64 + slot]);
            out.object = obj;
            out.end = RL_PATH_END_EMITTER;
            results[rl_f2u(emit[0 * 64 + slot])] = out;
        }
        rl_wave_sync();
    };
#endif
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
                const RlSpectralRay r = rays[idx];
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
                } else { // a NaN or infinite wavelength: no path (include/robigo_luculenta.h)
                    RlPathResult out;
                    out.value = 0.0f;
                    out.segments = 0u;
                    out.object = RL_OBJECT_NONE;
                    out.end = RL_PATH_END_INVALID;
                    results[idx] = out;
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

        // ---- the rest of the loop body (trace_unit.rs:92-126), and the result of a path that ends ----
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
#if RL_PATHS_EMIT_QUEUE
        {
            const uint64_t m = __builtin_amdgcn_ballot_w64(on_light);
            if (m != 0) {
                const uint32_t n_new = (uint32_t)__popcll(m);
                if (RL_UNLIKELY(e_tail - e_head + n_new > 64u)) {
                    process_emitted(e_tail - e_head);
                    e_head = e_tail;
                }
                if (on_light) {
                    const uint32_t slot = rl_mbcnt_from(m, e_tail) & 63u;
                    emit[0 * 64 + slot] = rl_u2f(my_ray);
                    emit[1 * 64 + slot] = rl_u2f(segments);
                    emit[2 * 64 + slot] = p.wavelength;
                    emit[3 * 64 + slot] = p.intensity;
                    emit[4 * 64 + slot] = rl_u2f(emitter);
                    active = false;
                }
                e_tail += n_new;
                if (RL_UNLIKELY(e_tail - e_head == 64u)) {
                    process_emitted(64u);
                    e_head += 64u;
                }
            }
        }
#else
        if (on_light) value = rl_emission(sv, p.intensity, p.wavelength, emitter);
#endif
        if (active && (status != RL_PATH_CONTINUES || segments >= max_segments)) {
            uint32_t end = RL_PATH_END_LIMIT;
            if (on_light) end = RL_PATH_END_EMITTER;
            else if (status == RL_PATH_ENDED) end = hit.obj == RL_HIT_NONE ? RL_PATH_END_VOID : RL_PATH_END_ROULETTE;
            RlPathResult out;
            out.value = status == RL_PATH_CONTINUES ? 0.0f : value;
            out.segments = segments;
            out.object = on_light ? emitter : RL_OBJECT_NONE;
            out.end = end;
            results[my_ray] = out;
            active = false;
        }
        RL_T1(RL_ST_T_EMIT, t_emit);
        rl_wave_sync(); // (the next iteration's scan rewrites the wave's scratch)
    }
#if RL_PATHS_EMIT_QUEUE
    if (e_tail != e_head) process_emitted(e_tail - e_head);
#endif
    RL_T1(RL_ST_T_TOTAL, t_total);
#ifdef RL_STATS
    if (lane == 0)
        for (int k = 0; k < RL_ST_COUNT; ++k) atomicAdd(&rl_stat_counters[k], st[k]);
#endif
}
