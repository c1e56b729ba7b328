// rl_query.hip.h -- the query kernel behind rl_scene_intersect / rl_scene_intersect_device: Scene::intersect (scene.rs:39-60)
// for a batch of independent rays, through the trace kernel's own scan (rl_scan_wave) and hit completion (rl_finish_hit).
// Also what the path, film and step kernels share with it: one segment's intersection (rl_intersect_segment) and the hit record
// (rl_ray_hit_of).  Included by rl_api.hip after rl_kernels.hip.h (rl_stage_scene) and the public header (RlRay, RlRayHit).
#pragma once

// Scene::intersect for one ray by the linear scan of rl_scan (rl_core.h) WITHOUT the cull of the sphere clusters, for the rays the
// scan's culls do not cover: the reference's sphere test takes the direction as a unit vector (a = 1, geometry.rs:204-216), so for
// |direction| != 1 its "hits" and distances are not those of the geometric ray the conservative bounds (and the far bound) are
// sized for -- a ray of length 2 "hits" spheres whose cluster bound it geometrically misses -- and a non-finite origin or direction
// makes every cull term NaN.  The renderer's rays are unit vectors up to rounding (glass: ~1e-7), the scan's slack covers those.
// Every sphere (radius^2 from RlSceneView::sphere_r2: a clustered sphere's record holds its cull term), then the small primitives
// and the prisms (their bound is a plane-based, parametric test: valid for any direction) in rl_scan's order and arithmetic.
__device__ __forceinline__ RlHit rl_query_exhaustive(const RlSceneView& sv, RlF3 o, RlF3 dir) {
    RlHit best;
    best.t = 1.0e12f; // scene.rs:43
    best.obj = RL_HIT_NONE;
    best.sub = 0;
    auto sphere_test = [&](uint32_t pos) {
        const RlF4 s = sv.spheres[pos];
        const float cox = s.x - o.x, coy = s.y - o.y, coz = s.z - o.z;
        const float dd = dir.x * cox + dir.y * coy + dir.z * coz;
        const float c = (cox * cox + coy * coy + coz * coz) - sv.sphere_r2[pos];
        const float q = dd * dd - c;
        if (q >= 0.0f && dd > 0.0f) {
            const float sq = sqrtf(q);
            const float t1 = dd - sq;
            const float t2 = dd + sq;
            const uint32_t obj = sv.sphere_obj[pos];
            if (t1 > 0.0f && t1 < t2 && rl_nearer(t1, obj, best)) {
                best.t = t1;
                best.obj = obj;
            }
        }
    };
    for (uint32_t i = 0; i < sv.n_direct; ++i) sphere_test(i);
    for (uint32_t k = 0; k < sv.n_clusters; ++k) {
        const uint32_t base = sv.cluster_base + (sv.cluster_k + 1u) * k;
        for (uint32_t j = 1; j <= sv.cluster_k; ++j) sphere_test(base + j);
    }
    for (uint32_t i = 0; i < sv.n_parabs; ++i) {
        const RlF4 r0 = sv.parabs[3 * i], r1 = sv.parabs[3 * i + 1], r2 = sv.parabs[3 * i + 2];
        const float t = rl_paraboloid_t(rl_xyz(r0), rl_xyz(r1), rl_xyz(r2), o, dir);
        const uint32_t obj = rl_f2u(r0.w);
        if (!(t < 0.0f) && rl_nearer(t, obj, best)) {
            best.t = t;
            best.obj = obj;
        }
    }
    for (uint32_t i = 0; i < sv.n_planes; ++i) {
        const RlF4 r0 = sv.planes[2 * i], r1 = sv.planes[2 * i + 1];
        float dn;
        const float t = rl_plane_t(rl_xyz(r0), rl_xyz(r1), o, dir, &dn);
        bool hit = t > 0.0f;
        if (hit && r0.w >= 0.0f) {
            const RlF3 dp = rl_sub(rl_add(o, rl_mul(dir, t)), rl_xyz(r1));
            hit = rl_dot(dp, dp) <= r0.w;
        }
        const uint32_t obj = rl_f2u(r1.w);
        if (hit && rl_nearer(t, obj, best)) {
            best.t = t;
            best.obj = obj;
        }
    }
    for (uint32_t i = 0; i < sv.n_prisms; ++i) {
        const RlF4* pr = sv.prisms + RL_PRISM_STRIDE * i;
        if (!rl_bound_pass(pr[16], o, dir)) continue;
        const RlCand c = rl_hex_prism_decided(pr, o, dir);
        const uint32_t obj = rl_f2u(pr[1].w);
        if (c.t >= 0.0f && rl_nearer(c.t, obj, best)) {
            best.t = c.t;
            best.obj = obj;
            best.sub = c.k;
        }
    }
    return best;
}

// Scene::intersect for every lane's segment, as the query, path, film and step kernels make it: the wave's scan with a full exec
// mask and the plain launches' options (128 registers, the template arguments of the non-open rl_trace_kernel of the same stage),
// then the exact linear scan under the lanes the scan's culls are not sized for (rl_query_exhaustive): |direction|^2 further than
// 2^-20 from 1, or a NaN / infinite component -- decided per segment, refraction and reflection keep a non-unit direction's
// length.  Those lanes, and the lanes that are not `active`, scan a null ray, muted by the idle bit (rl_scan_wave wants exec all ones).
template <int STAGE, bool CYL>
__device__ __forceinline__ RlHit rl_intersect_segment(const RlStagedScene& staged, const RlSceneLayout& lay, bool active, RlF3 o, RlF3 d, RlWaveScratch* ws,
                                                      uint32_t lane RL_TACC_PARAM) {
    const RlF4* base = staged.base;
    const uint32_t tab0 = staged.tab0;
    const float d2 = d.x * d.x + d.y * d.y + d.z * d.z;
    const bool exhaustive = active && !(fabsf(d2 - 1.0f) <= 0x1p-20f && fabsf(o.x) < INFINITY && fabsf(o.y) < INFINITY && fabsf(o.z) < INFINITY);
    const bool scanned = active && !exhaustive;
    RlHit hit = rl_scan_wave<CYL, true, STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_NONE, STAGE == RL_STAGE_ALL,
                             STAGE != RL_STAGE_NONE, STAGE != RL_STAGE_ALL>(staged.sv, base + (lay.off_cull - tab0), CYL ? base + (lay.off_prism_cyl - tab0) : nullptr,
                                                                            lay.group_gc, lay.small_ordered, lay.cull_cmax2, lay.n_cluster_groups,
                                                                            lay.n_prism_groups, lay.n_cluster_supers, lay.super_g, staged.ring_t,
                                                                            scanned ? o : rl_f3(0.0f, 0.0f, 0.0f), scanned ? d : rl_f3(0.0f, 0.0f, 0.0f),
                                                                            scanned ? 0u : 0x80000000u, ws, lane RL_TACC_ARG);
    RL_T0(t_exhaustive);
    RL_STAT(RL_ST_X_LANES, __popcll(__builtin_amdgcn_ballot_w64(exhaustive)));
    RL_STAT(RL_ST_X_ITERS, __builtin_amdgcn_ballot_w64(exhaustive) != 0);
    if (exhaustive) hit = rl_query_exhaustive(staged.sv, o, d);
    RL_T1(RL_ST_T_EXHAUSTIVE, t_exhaustive);
    return hit;
}

// The RlRayHit of a segment's nearest hit (`found`: there is one that counts; all zero and RL_OBJECT_NONE otherwise).
__device__ __forceinline__ RlRayHit rl_ray_hit_of(const RlSceneView& sv, RlF3 o, RlF3 d, const RlHit& hit, bool found) {
    RlRayHit out;
    out.isect.position = out.isect.normal = out.isect.tangent = RlVector3{0.0f, 0.0f, 0.0f};
    out.isect.distance = 0.0f;
    out.object = RL_OBJECT_NONE;
    out.reserved = 0u;
    if (found) {
        const uint32_t kinds = rl_f2u(sv.objects[hit.obj].w);
        const uint32_t surface_kind = rl_object_surface(kinds);
        const RlIsect is = rl_finish_hit(sv, o, d, hit, surface_kind, rl_object_group(kinds));
        // Intersection.tangent: normalise(cross((0, 1, 0), normal)) on spheres (geometry.rs:250-251), the zero vector on every
        // other surface -- which normalise returns unchanged (the soap bubble's form, rl_core.h: rl_bounce)
        const RlF3 axis = surface_kind == RL_SURFACE_SPHERE ? rl_cross(rl_f3(0.0f, 1.0f, 0.0f), is.normal) : rl_f3(0.0f, 0.0f, 0.0f);
        const RlF3 tangent = rl_normalise(axis);
        out.isect.position = RlVector3{is.position.x, is.position.y, is.position.z};
        out.isect.normal = RlVector3{is.normal.x, is.normal.y, is.normal.z};
        out.isect.tangent = RlVector3{tangent.x, tangent.y, tangent.z};
        out.isect.distance = hit.t;
        out.object = hit.obj; // the flattened object table is in description order
    }
    return out;
}

// Persistent workgroups of RL_TRACE_BLOCK threads, laid out like the trace kernel's plain launches: each stages the scene once
// (rl_stage_scene), then every wave takes chunks of 64 rays -- chunk c goes to wave c mod (waves of the grid) -- and scans them
// together (rl_intersect_segment); lanes past the end idle.  The body around the scan is far lighter than a path's.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_query_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, const RlRay* __restrict__ rays, RlRayHit* __restrict__ hits, uint32_t n_rays) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {}; // (the scan's event counters: kept per wave and dropped, the query reports none)
#endif

    const uint32_t wave = blockIdx.x * (RL_TRACE_BLOCK / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (RL_TRACE_BLOCK / 64);
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_rays + 63u) / 64u); // (c * 64 + lane below stays under 2^32)
    for (uint32_t c = wave; c < n_chunks; c += n_waves) {
        const uint32_t i = c * 64u + lane;
        const bool active = i < n_rays;
        RlF3 o = rl_f3(0.0f, 0.0f, 0.0f), d = rl_f3(0.0f, 0.0f, 0.0f); // (an idle lane scans a null ray, muted by the idle bit)
        float t_max = 0.0f;
        if (active) {
            const RlRay r = rays[i];
            o = rl_f3(r.origin.x, r.origin.y, r.origin.z);
            d = rl_f3(r.direction.x, r.direction.y, r.direction.z);
            t_max = r.t_max;
        }
        const RlHit hit = rl_intersect_segment<STAGE, CYL>(staged, lay, active, o, d, ws, lane RL_TACC_ARG);
        // Filtering after the scan is exact: when the nearest hit is at or beyond t_max no other hit can count.  (`<`: a hit at
        // exactly t_max misses, and so does every hit for a t_max that is NaN, zero or negative.)
        const RlRayHit out = rl_ray_hit_of(staged.sv, o, d, hit, hit.obj != RL_HIT_NONE && hit.t < t_max);
        if (active) hits[i] = out;
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
}
