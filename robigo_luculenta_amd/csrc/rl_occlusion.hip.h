// rl_occlusion.hip.h -- the occlusion kernel behind rl_scene_occluded / rl_scene_occluded_device: "would rl_scene_intersect report
// an object for this ray?" as one byte per ray.  The query kernel's shape (rl_query.hip.h) around the any-hit form of the wave's
// scan (rl_scan_wave, BOUNDED): the scan starts from the ray's own t_max instead of 1e12, so a short shadow ray culls everything
// beyond its end, and a lane stops as soon as it holds any hit below its bound.  No hit record is completed: no rl_finish_hit, no
// tangent.  Included by rl_api.hip after rl_query.hip.h (rl_query_exhaustive).
#pragma once

// Is there a hit with distance < t_max (and < 1e12) on every lane's ray?  rl_intersect_segment's per-ray rule with a bound: lanes
// whose t_max is NaN, zero or negative are decided already (nothing blocks them) and scan nothing, like the lanes that are not
// `active`; lanes whose direction is not a unit vector (|d|^2 further than 2^-20 from 1) or whose ray has a non-finite component
// take the exact linear scan (rl_query_exhaustive) and are filtered afterwards; every other lane scans with its bound.  "Some hit
// below t_max" and "the nearest hit is below t_max" are the same predicate, so the bounded scan's early stop and the filter agree
// -- whatever the batch split, the fetch mode, the variant or the order the wave's rounds ran in.
template <int STAGE, bool CYL>
__device__ __forceinline__ bool rl_occluded_segment(const RlStagedScene& staged, const RlSceneLayout& lay, bool active, RlF3 o, RlF3 d, float t_max, RlWaveScratch* ws,
                                                    uint32_t lane RL_TACC_PARAM) {
    const RlF4* base = staged.base;
    const uint32_t tab0 = staged.tab0;
    const bool wanted = active && t_max > 0.0f; // (false for NaN)
    const float d2 = d.x * d.x + d.y * d.y + d.z * d.z;
    const bool exhaustive = wanted && !(fabsf(d2 - 1.0f) <= 0x1p-20f && fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY);
    const bool scanned = wanted && !exhaustive;
    RlHit hit = rl_scan_wave<CYL, true, STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_NONE, STAGE == RL_STAGE_ALL,
                             STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_ALL, true>(staged.sv, base + (lay.off_cull - tab0), CYL ? base + (lay.off_prism_cyl - tab0) : nullptr,
                                                                                  lay.group_gc, lay.small_ordered, lay.cull_cmax2, lay.n_cluster_groups,
                                                                                  lay.n_prism_groups, lay.n_cluster_supers, lay.super_g, staged.ring_t,
                                                                                  scanned ? o : rl_f3(0.0f, 0.0f, 0.0f), scanned ? d : rl_f3(0.0f, 0.0f, 0.0f),
                                                                                  scanned ? 0u : 0x80000000u, ws, lane RL_TACC_ARG, scanned ? fminf(t_max, 1.0e12f) : 0.0f);
    if (exhaustive) hit = rl_query_exhaustive(staged.sv, o, d);
    // The predicate is the query kernel's filter, not the scan's seed: a hit at exactly t_max does not block.
    return wanted && hit.obj != RL_HIT_NONE && hit.t < t_max;
}

// Persistent workgroups as the query kernel's: the scene staged once per workgroup, chunk c of 64 rays to wave c mod (waves of the
// grid), lanes past the end idle.  One byte per ray, stored under `active` alone: bytes past n_rays belong to somebody else.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_occlusion_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlRay* __restrict__ rays, uint8_t* __restrict__ occluded, uint32_t n_rays) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, as the query kernel does)
#endif

    const uint32_t wave = blockIdx.x * (RL_TRACE_BLOCK / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (RL_TRACE_BLOCK / 64);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_rays + 63u) / 64u); // (c * 64 + lane below stays under 2^32)
    for (uint32_t c = wave; c < n_chunks; c += n_waves) {
        const uint32_t i = c * 64u + lane;
        const bool active = i < n_rays;
        RlF3 o = rl_f3(0.0f, 0.0f, 0.0f), d = rl_f3(0.0f, 0.0f, 0.0f);
        float t_max = 0.0f;
        if (active) {
            const RlRay r = rays[i];
            o = rl_f3(r.origin.x, r.origin.y, r.origin.z);
            d = rl_f3(r.direction.x, r.direction.y, r.direction.z);
            t_max = r.t_max;
        }
        const bool blocked = rl_occluded_segment<STAGE, CYL>(staged, lay, active, o, d, t_max, ws, lane RL_TACC_ARG);
        if (active) occluded[i] = blocked ? (uint8_t)1 : (uint8_t)0;
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
}
