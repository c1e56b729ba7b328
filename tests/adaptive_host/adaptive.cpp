// Host compile of the adaptive sampler's plan rule (rl_adaptive_plan.h) and per-sample arithmetic (rl_adaptive.hip.h), for the tests
// that run without a GPU.  Test-only: the product never runs this code on the CPU.
#include <cstring>
#include <vector>

#include "../../robigo_luculenta_amd/csrc/rl_cie1931.h"
#include "../../robigo_luculenta_amd/csrc/rl_core.h"
#include "../../robigo_luculenta_amd/csrc/rl_scene.h"
#include "../../robigo_luculenta_amd/csrc/rl_adaptive.hip.h"

struct AdaptiveScene {
    RlFlatScene flat;
    RlSceneView view;
};

extern "C" {

void* adaptive_scene_create(const RlObjectDesc* objs, uint32_t n, const RlCameraDesc* cam) {
    RlSceneDesc d;
    d.n_objects = n;
    d.objects = objs;
    d.camera = *cam;
    AdaptiveScene* s = new AdaptiveScene();
    const char* err;
    if (rl_flatten_scene(&d, &s->flat, &err) != 0) {
        delete s;
        return nullptr;
    }
    // the whole view, as tests/host_mirror makes it: adaptive_render scans the scene
    RlSceneView& v = s->view;
    v = RlSceneView{};
    v.spheres = s->flat.spheres.data();
    v.planes = s->flat.planes.data();
    v.parabs = s->flat.parabs.data();
    v.prisms = s->flat.prisms.data();
    v.objects = s->flat.objects.data();
    v.sphere_obj = s->flat.sphere_obj.data();
    v.sphere_r2 = nullptr; // host view: every sphere record is {centre, radius^2}
    v.cie = (const RlF4*)RL_CIE1931_XYZ0;
    v.n_direct = s->flat.n_direct;
    v.n_direct_padded = s->flat.n_direct_padded;
    v.cluster_base = s->flat.cluster_base;
    v.n_clusters = s->flat.n_clusters;
    v.cluster_k = s->flat.cluster_k;
    v.n_planes = (uint32_t)(s->flat.planes.size() / 2);
    v.n_parabs = (uint32_t)(s->flat.parabs.size() / 3);
    v.n_prisms = (uint32_t)(s->flat.prisms.size() / RL_PRISM_STRIDE);
    v.n_objects = (uint32_t)s->flat.objects.size();
    v.camera_rec = s->flat.camera_rec.data();
    return s;
}
void adaptive_scene_destroy(void* s) { delete (AdaptiveScene*)s; }

// rl_adaptive_plan_rule as it stands: 0, or the rule's refusal.
int adaptive_plan(uint32_t width, uint32_t height, const double* importance, double uniform_share, uint64_t n_paths, uint32_t* counts,
                  float* weights, float* cells4, double* importance_sum) {
    return rl_adaptive_plan_rule(width, height, importance, uniform_share, n_paths, counts, weights, (RlAdaptiveCell*)cells4, importance_sum);
}

// What rl_adaptive_samples_kernel writes for samples first_sample .. first_sample + n - 1 of the plan (off, cells4, weights) of a
// width x height film, with the launch constants the library computes.
void adaptive_samples(void* scene, uint32_t width, uint32_t height, const uint32_t* off, const float* cells4, const float* weights,
                      uint32_t n_tiles, uint64_t seed, uint32_t stream, uint64_t first_path, uint32_t first_sample, uint32_t n,
                      RlCameraSample* out) {
    const RlSceneView& sv = ((AdaptiveScene*)scene)->view;
    const float wm1 = (float)(int)width - 1.0f, hm1 = (float)(int)height - 1.0f, aspect = (float)width / (float)height;
    const RlAdaptiveCell* cells = (const RlAdaptiveCell*)cells4;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t j = first_sample + i;
        const uint32_t tile = rl_adaptive_tile_of(off, n_tiles, j);
        uint32_t bits;
        memcpy(&bits, &weights[tile], 4);
        const RlAdaptiveDraw d = rl_adaptive_draw(wm1, hm1, aspect, cells[tile], seed, stream, first_path + j);
        out[i].ray = rl_adaptive_ray(sv, d, seed, stream, first_path + j);
        out[i].x = d.x;
        out[i].y = d.y;
        out[i].reserved0 = tile;
        out[i].reserved1 = bits;
    }
}

// The photons rl_plot_unit_render_adaptive splats for the samples (adaptive_samples' records): each ray traced as path
// first_path + first_sample + i by the host compile of the kernel's per-path header (the loop of tests/host_mirror's mirror_render,
// from the sample's ray on), probability = value * w_t in one f32 multiply.  values, if given, receives the unweighted values.
void adaptive_render(void* scene, const RlCameraSample* samples, uint64_t seed, uint32_t stream, uint64_t first_path, uint32_t first_sample,
                     uint32_t n, RlMappedPhoton* photons, float* values) {
    const RlSceneView& sv = ((AdaptiveScene*)scene)->view;
    for (uint32_t i = 0; i < n; ++i) {
        const RlCameraSample& c = samples[i];
        const uint64_t path = first_path + (first_sample + i);
        RlPath p;
        p.origin = rl_f3(c.ray.origin.x, c.ray.origin.y, c.ray.origin.z);
        p.direction = rl_f3(c.ray.direction.x, c.ray.direction.y, c.ray.direction.z);
        p.wavelength = c.ray.wavelength;
        p.intensity = 1.0f;
        p.continue_chance = 1.0f;
        p.sx = c.x;
        p.sy = c.y;
        p.ior = rl_sf10_ior(c.ray.wavelength);
        p.bounce = 0;
        float value = 0.0f;
        for (;;) {
            const RlHit hit = rl_scan(sv, p.origin, p.direction);
            uint32_t emitter = 0;
            const int status = rl_bounce(sv, seed, stream, path, &p, hit, &value, &emitter);
            if (status == RL_PATH_ENDED_ON_EMITTER) value = rl_emission(sv, p.intensity, p.wavelength, emitter);
            if (status != RL_PATH_CONTINUES) break;
        }
        float weight;
        memcpy(&weight, &c.reserved1, 4);
        photons[i].x = c.x;
        photons[i].y = c.y;
        photons[i].probability = value * weight;
        photons[i].wavelength = c.ray.wavelength;
        if (values) values[i] = value;
    }
}
}
