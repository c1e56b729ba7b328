// Host compile of the wavelength table's rule and per-path arithmetic (rl_wavelength.h), for the tests that run without a GPU and as
// the byte-for-byte reference of the ones that run with one.  Test-only: the product never runs this code on the CPU.
#include <cstring>
#include <vector>

#include "../../robigo_luculenta_amd/csrc/rl_cie1931.h"
#include "../../robigo_luculenta_amd/csrc/rl_core.h"
#include "../../robigo_luculenta_amd/csrc/rl_scene.h"
#include "../../robigo_luculenta_amd/csrc/rl_wavelength.h"

struct WavelengthScene {
    RlFlatScene flat;
    RlSceneView view;
};

extern "C" {

void* wavelength_scene_create(const RlObjectDesc* objs, uint32_t n, const RlCameraDesc* cam) {
    RlSceneDesc d;
    d.n_objects = n;
    d.objects = objs;
    d.camera = *cam;
    WavelengthScene* s = new WavelengthScene();
    const char* err;
    if (rl_flatten_scene(&d, &s->flat, &err) != 0) {
        delete s;
        return nullptr;
    }
    // the whole view, as tests/host_mirror makes it
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
void wavelength_scene_destroy(void* s) { delete (WavelengthScene*)s; }

// rl_wavelength_table_rule as it stands: 0, or the rule's refusal.  table: 513 floats.
int wavelength_table(const double* importance, uint32_t n_nodes, double uniform_share, float* table) {
    return rl_wavelength_table_rule(importance, n_nodes, uniform_share, table);
}
void wavelength_cie_importance(double* out81) { rl_wavelength_cie_importance(out81); }

// What a path makes of the words w0[0..n): its wavelength, the bin found again from the wavelength, and its weight.
void wavelength_draws(const float* table, const uint32_t* w0, uint64_t n, float* wavelength, uint32_t* bin, float* weight) {
    for (uint64_t i = 0; i < n; ++i) {
        wavelength[i] = rl_wavelength_draw(table, w0[i]);
        if (bin) bin[i] = rl_wavelength_bin(table, wavelength[i]);
        if (weight) weight[i] = rl_wavelength_weight(table, wavelength[i]);
    }
}

// The camera half of paths first .. first + n - 1 with the table (null: rl_begin_path): rays8 = {origin, wavelength, direction, ior}
// per path, xy = the screen position.
void wavelength_camera(void* scene, uint32_t w, uint32_t h, const float* table, uint64_t seed, uint32_t stream, uint64_t first, uint64_t n,
                       float* rays8, float* xy) {
    const RlSceneView& sv = ((WavelengthScene*)scene)->view;
    const float aspect = (float)w / (float)h;
    for (uint64_t i = 0; i < n; ++i) {
        RlPath p;
        if (table) rl_begin_path_wl(sv, aspect, seed, stream, first + i, table, &p);
        else rl_begin_path(sv, aspect, seed, stream, first + i, &p);
        float* r = rays8 + 8 * i;
        r[0] = p.origin.x; r[1] = p.origin.y; r[2] = p.origin.z; r[3] = p.wavelength;
        r[4] = p.direction.x; r[5] = p.direction.y; r[6] = p.direction.z; r[7] = p.ior;
        xy[2 * i] = p.sx;
        xy[2 * i + 1] = p.sy;
    }
}

// The photons a trace unit with the table writes for paths first .. first + n - 1 (tests/host_mirror's mirror_render with the table's
// draw and weight; null table: mirror_render itself), their segments, and, if asked for, the unweighted values.
void wavelength_render(void* scene, uint32_t w, uint32_t h, const float* table, uint64_t seed, uint32_t stream, uint64_t first, uint64_t n,
                       RlMappedPhoton* photons, uint64_t* segments, float* values) {
    const RlSceneView& sv = ((WavelengthScene*)scene)->view;
    const float aspect = (float)w / (float)h;
    uint64_t segs = 0;
    for (uint64_t i = 0; i < n; ++i) {
        RlPath p;
        if (table) rl_begin_path_wl(sv, aspect, seed, stream, first + i, table, &p);
        else rl_begin_path(sv, aspect, seed, stream, first + i, &p);
        float value = 0.0f;
        bool emitted = false;
        for (;;) {
            const RlHit hit = rl_scan(sv, p.origin, p.direction);
            segs += 1;
            uint32_t emitter = 0;
            const int status = rl_bounce(sv, seed, stream, first + i, &p, hit, &value, &emitter);
            if (status == RL_PATH_ENDED_ON_EMITTER) value = rl_emission(sv, p.intensity, p.wavelength, emitter), emitted = true;
            if (status != RL_PATH_CONTINUES) break;
        }
        if (values) values[i] = value;
        if (table && emitted) value = value * rl_wavelength_weight(table, p.wavelength);
        photons[i].x = p.sx;
        photons[i].y = p.sy;
        photons[i].probability = value;
        photons[i].wavelength = p.wavelength;
    }
    if (segments) *segments = segs;
}
}
