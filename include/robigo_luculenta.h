/* robigo_luculenta.h -- C ABI of the MI355X-native hot path of robigo-luculenta.
 *
 * The reference has no FFI; its seam is the `Task` enum and the four unit structs that worker
 * threads execute (app.rs:113-164).  Each entry point below replaces one unit method (cited), so a
 * Rust host keeps task_scheduler.rs untouched and swaps the bodies of App::execute_*_task for these
 * calls (INTEGRATION.md shows the `extern "C"` block and the #[repr(C)] structs).
 *
 * Conventions: every function returns 0 on success or a negative RL_E_* code; the message is
 * available through rl_last_error() (thread-local).  Nothing throws or aborts across the boundary
 * (the reference panics instead: app.rs:107,163; gather_unit.rs:69-70).  Handles are opaque, own
 * their device buffers, and are used by one host thread at a time -- the same exclusive ownership
 * the reference gets by moving Box<Unit> through Task (task_scheduler.rs:26-41).  A scene handle is
 * immutable after creation and may be shared (Arc<Scene>, app.rs:63).
 *
 * There is no CPU implementation behind this ABI: every compute entry point runs hand-written
 * gfx950 kernels and fails with RL_E_NO_DEVICE when no GPU is present.
 */
#ifndef ROBIGO_LUCULENTA_H
#define ROBIGO_LUCULENTA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- frozen data layouts ------------------------------------------------------------------ */

/* vector3.rs:20-25 (12 bytes; gather_unit.rs:75 relies on that size). */
typedef struct RlVector3 {
    float x, y, z;
} RlVector3;

/* trace_unit.rs:23-37. */
typedef struct RlMappedPhoton {
    float x, y, probability, wavelength;
} RlMappedPhoton;

/* Surfaces (geometry.rs) and materials (material.rs) as plain data.  The reference hard-codes its
 * scene in Rust (app.rs:166-363); here a scene is an array of RlObjectDesc in scan order. */
enum RlSurfaceKind {
    RL_SURFACE_SPHERE = 0,     /* Sphere::new(position = v0, radius = f0)              geometry.rs:195-200 */
    RL_SURFACE_PLANE = 1,      /* Plane::new(normal = v0, offset = v1)                 geometry.rs:44-51   */
    RL_SURFACE_CIRCLE = 2,     /* Circle::new(normal = v0, position = v1, radius = f0) geometry.rs:142-150 */
    RL_SURFACE_PARABOLOID = 3, /* Paraboloid::new(normal = v0, offset = v1, focal_distance = f0) :286-295  */
    RL_SURFACE_HEX_PRISM = 4   /* new_hexagonal_prism(axis = v0, offset = v1, edge_length = f0,
                                  bevel_size = f1, angle = f2, height = f3)            geometry.rs:493-515 */
};

enum RlMaterialKind {
    RL_MATERIAL_BLACK_BODY = 0,       /* emissive; BlackBodyMaterial::new(kelvins = m0, intensity = m1) material.rs:93-99 */
    RL_MATERIAL_DIFFUSE_GREY = 1,     /* DiffuseGreyMaterial::new(reflectance = m0)             material.rs:115-119 */
    RL_MATERIAL_DIFFUSE_COLOURED = 2, /* DiffuseColouredMaterial::new(refl = m0, wavel = m1, dev = m2)  :145-152 */
    RL_MATERIAL_GLOSSY_MIRROR = 3,    /* GlossyMirrorMaterial::new(gloss = m0)                  material.rs:177-182 */
    RL_MATERIAL_SF10_GLASS = 4,       /* Sf10GlassMaterial                                      material.rs:199 */
    RL_MATERIAL_SOAP_BUBBLE = 5       /* SoapBubbleMaterial                                     material.rs:265 */
};

typedef struct RlObjectDesc {
    uint32_t surface_kind;  /* enum RlSurfaceKind */
    uint32_t material_kind; /* enum RlMaterialKind */
    RlVector3 v0, v1;       /* surface constructor vectors, see RlSurfaceKind */
    float f0, f1, f2, f3;   /* surface constructor scalars */
    float m0, m1, m2;       /* material constructor scalars, see RlMaterialKind */
} RlObjectDesc;

/* The camera as a function of time t in [0,1]; parametrises make_camera (app.rs:327-357):
 *   phi = PI * (phi0 + phi1 * t);  alpha = PI * (alpha0 + alpha1 * t);  distance = dist0 + dist1 * t
 *   position = (cos(alpha) sin(phi), cos(alpha) cos(phi), sin(alpha)) * distance
 *   orientation = rotation((0,0,-1), phi + PI) * rotation((1,0,0), -alpha)
 *   field_of_view = PI * fov_over_pi;  focal_distance = distance * focal_factor */
typedef struct RlCameraDesc {
    float phi0, phi1;
    float alpha0, alpha1;
    float dist0, dist1;
    float fov_over_pi;
    float focal_factor;
    float depth_of_field;
    float chromatic_abberation;
} RlCameraDesc;

typedef struct RlSceneDesc {
    uint32_t n_objects;
    const RlObjectDesc* objects;
    RlCameraDesc camera;
} RlSceneDesc;

/* Built-in scene generators. */
enum RlBuiltinScene {
    RL_SCENE_DEMO = 0,         /* App::set_up_scene, app.rs:166-363; param = seeds (0 -> 100 as in app.rs:238) */
    RL_SCENE_GLASS_STRESS = 1, /* fixed objects 0-6 + three rings of SF10 prisms (BASELINE config 3); param unused */
};

/* Where the trace kernel reads the primitive list from. */
// RL_FETCH_LDS stages as much as fits beside the waves' scratch, which leaves 32 KB of the 160 (24 KB where the cull table has a
// third level, 2 KB less in a blocking render call): the whole scene (random spheres: up to about 670 objects; a prism takes as
// much as eight spheres), else its tables (planes, paraboloids, prisms, the cull table) with the spheres and objects read from
// L2 / HBM, else -- tables beyond those 32 or 24 KB: some 80 prisms beside 3,000 spheres, a thousand planes, tens of thousands of
// objects -- nothing.  RL_FETCH_GLOBAL never stages anything.  (tests/test_scene_extremes.py finds both thresholds and prints them.)
enum RlPrimitiveFetch {
    RL_FETCH_LDS = 0,   /* primitives + CIE tables staged in LDS by each workgroup */
    RL_FETCH_GLOBAL = 1 /* wave-uniform loads from HBM/L2 through the scalar cache */
};

enum RlError {
    RL_OK = 0,
    RL_E_INVALID = -1,   /* bad argument */
    RL_E_NO_DEVICE = -2, /* no gfx950 device / HIP runtime failure at start-up */
    RL_E_HIP = -3,       /* a HIP call failed; see rl_last_error() */
    RL_E_IO = -4,        /* checkpoint file could not be opened / written */
    RL_E_STATE = -5      /* handle used out of protocol (e.g. size mismatch between units) */
};

typedef struct RlScene RlScene;
typedef struct RlTraceUnit RlTraceUnit;
typedef struct RlPlotUnit RlPlotUnit;
typedef struct RlGatherUnit RlGatherUnit;
typedef struct RlTonemapUnit RlTonemapUnit;
typedef struct RlDenoiseUnit RlDenoiseUnit;
typedef struct RlSpectralUnit RlSpectralUnit;
typedef struct RlGlareUnit RlGlareUnit;
typedef struct RlRelightUnit RlRelightUnit;
typedef struct RlErrorUnit RlErrorUnit;
typedef struct RlRobustUnit RlRobustUnit;
typedef struct RlAdaptiveUnit RlAdaptiveUnit;
typedef struct RlWavelengthTable RlWavelengthTable;
typedef struct RlScheduler RlScheduler;
typedef struct RlComm RlComm;

const char* rl_last_error(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int rl_device_count(void);
/* The PCI bus id ("0000:c1:00.0") of visible device `device`: what tells two processes whether "device 0" is the same GPU
 * for both (ranks launched with a per-rank device mask) or not -- RCCL admits one rank per GPU. */
int rl_device_pci_bus_id(int device, char* out, uint32_t cap);
const char* rl_version(void);
/* 16 hex digits: a hash of the sources this library's device code was compiled from (csrc/Makefile).  Profiles
 * record it so that counter-derived figures are never quoted for a different build. */
const char* rl_build_id(void);

/* ---- scene (scene.rs:23-35, app.rs:166-363) ------------------------------------------------ */

/* Fills `objects` (capacity `cap`) with the built-in scene and writes the object count to
 * *n_objects and the camera to *camera.  Pure host code, needs no device.  When cap is too small
 * returns RL_E_INVALID with *n_objects set to the required count. */
int rl_scene_builtin_desc(int which, int param, RlObjectDesc* objects, uint32_t cap, uint32_t* n_objects,
                          RlCameraDesc* camera);
/* Scene descriptions as files (the reference hard-codes its scene, app.rs:166-363).  Little-endian binary:
 * "RLSC" magic, u32 version = 1, u32 n_objects, RlCameraDesc (40 bytes), n_objects x RlObjectDesc (60 bytes).
 * Host-only.  rl_scene_desc_load follows rl_scene_builtin_desc's capacity protocol. */
int rl_scene_desc_save(const char* path, const RlSceneDesc* desc);
int rl_scene_desc_load(const char* path, RlObjectDesc* objects, uint32_t cap, uint32_t* n_objects, RlCameraDesc* camera);
/* Flattens the description (hex prisms become 8 half-spaces, paraboloids get their derived
 * fields, black bodies their normalisation factor) and uploads it to `device`.  Replaces
 * App::set_up_scene + Arc::new (app.rs:63). */
int rl_scene_create(const RlSceneDesc* desc, int device, RlScene** out);
int rl_scene_destroy(RlScene* scene);

/* Ray (ray.rs:19-33) as a query: wavelength and probability do not affect Scene::intersect and are left out. */
typedef struct RlRay {
    RlVector3 origin;
    float t_max;         /* only hits with distance < t_max count (and < 1e12, scene.rs:43); INFINITY = Scene::intersect */
    RlVector3 direction; /* used as given, not normalised (the reference's glass rays are not normalised either) */
    uint32_t reserved;   /* ignored */
} RlRay;                 /* 32 bytes */

typedef struct RlIntersection { /* intersection.rs:20-32 */
    RlVector3 position, normal, tangent;
    float distance;
} RlIntersection;               /* 40 bytes */

#define RL_OBJECT_NONE 0xffffffffu

typedef struct RlRayHit {
    RlIntersection isect; /* all zero on a miss */
    uint32_t object;      /* index into RlSceneDesc::objects; RL_OBJECT_NONE on a miss */
    uint32_t reserved;    /* written 0 */
} RlRayHit;               /* 48 bytes */

/* Scene::intersect (scene.rs:39-60) for a batch of rays, on the scene's device: hits[i] is bit for bit what the
 * reference returns for rays[i] -- the nearest object (on equal distances the first one, scene.rs:51), the hit's
 * position, normal, tangent (normalise(cross((0,1,0), normal)) on spheres, geometry.rs:248-251; zero on every other
 * surface) and distance -- restricted to distance < t_max: a hit at exactly t_max, and any hit for a t_max that is NaN,
 * zero or negative, is a miss.  primitive_fetch (RL_FETCH_LDS / RL_FETCH_GLOBAL) has the meaning it has for
 * rl_trace_unit_set_fetch.  n_rays == 0 does nothing; NULL pointers with n_rays > 0, a NULL scene or an unknown fetch
 * mode are RL_E_INVALID.  Both calls return when the hits are written.
 *   rl_scene_intersect:        host arrays, staged through device buffers in chunks (any n_rays).
 *   rl_scene_intersect_device: device pointers on the scene's device (e.g. torch tensors); no host round trip.
 * Safe from several host threads at once on one scene.  Ordering against renders: a query kernel cannot share a CU with
 * a resident trace kernel, so a call made while an open launch runs on the device (a blocking render in flight, or one
 * begun with rl_trace_unit_render_begin / _fused_begin and not yet ended) waits until that launch drains.  An open launch
 * ends by itself once every call appended to it is complete and no new one arrived for its grace period (~150 us): it
 * does NOT wait for rl_trace_unit_render_end, so a query between _begin and _end completes, and the render is not
 * disturbed (its photons are those it computes alone).  While other threads keep appending render calls to the launch,
 * the query waits for as long as they do. */
int rl_scene_intersect(const RlScene* scene, int primitive_fetch, const RlRay* rays, uint32_t n_rays, RlRayHit* hits);
int rl_scene_intersect_device(const RlScene* scene, int primitive_fetch, const RlRay* device_rays, uint32_t n_rays,
                              RlRayHit* device_hits);

/* The any-hit form of the query above, for shadow rays, ambient occlusion and visibility between two points: occluded[i] is 1 if
 * rl_scene_intersect would return object != RL_OBJECT_NONE for rays[i], and 0 otherwise -- some object has a reference hit
 * distance d with d < t_max and d < 1e12.  A hit at exactly t_max does not block; a t_max that is NaN, zero or negative never
 * blocks; t_max = INFINITY asks whether the ray hits anything at all.  One byte per ray and nothing else is written: bytes past
 * n_rays are not touched.  The answer depends on the scene and the ray alone -- not on how a batch is split, the fetch mode, the
 * kernel variant, the order of evaluation or other callers: "some hit below t_max" and "the nearest hit is below t_max" are the
 * same predicate, so the kernel may stop at the first hit it finds below the ray's bound, and it scans no further than t_max (a
 * short ray in a large scene costs far less than rl_scene_intersect with the same t_max).  Rays are used as given: a ray with
 * |direction|^2 further than 2^-20 from 1, or with a non-finite component, is decided by the exact linear scan, as in
 * rl_scene_intersect.  Everything else is that call's: the argument checks in the same order (an unknown fetch mode, NULL rays
 * or NULL output with n_rays > 0, a NULL scene: RL_E_INVALID), n_rays == 0 does nothing, the host form stages in chunks of 2^20
 * rays, the _device form takes device pointers on the scene's device and refuses pageable host memory, both return when the
 * bytes are written, calls are safe from several host threads at once on one scene, and a call orders against open launches
 * as rl_scene_intersect does. */
int rl_scene_occluded(const RlScene* scene, int primitive_fetch, const RlRay* rays, uint32_t n_rays, uint8_t* occluded);
int rl_scene_occluded_device(const RlScene* scene, int primitive_fetch, const RlRay* device_rays, uint32_t n_rays,
                             uint8_t* device_occluded);

/* ---- TraceUnit::render_ray as a batched call: caller-supplied spectral rays ----------------- */

/* Ray (ray.rs:19-33) with its wavelength; the probability is folded into the path's intensity, which starts at 1. */
typedef struct RlSpectralRay {
    RlVector3 origin;
    float wavelength;    /* nm */
    RlVector3 direction; /* used as given, not normalised (like RlRay) */
    uint32_t reserved;   /* ignored */
} RlSpectralRay;         /* 32 bytes */

typedef struct RlCameraSample {
    RlSpectralRay ray;          /* the camera ray of the path: make_camera + Camera::get_ray (trace_unit.rs:136-158) */
    float x, y;                 /* screen position: RlMappedPhoton x, y of the same path */
    uint32_t reserved0, reserved1; /* written 0 */
} RlCameraSample;               /* 48 bytes */

enum RlPathEnd {
    RL_PATH_END_VOID = 0,     /* the path left the scene (trace_unit.rs:94) */
    RL_PATH_END_EMITTER = 1,  /* it hit a light: value = intensity * get_intensity(wavelength) (trace_unit.rs:99-101) */
    RL_PATH_END_ROULETTE = 2, /* Russian roulette ended it after a bounce (trace_unit.rs:122-125) */
    RL_PATH_END_LIMIT = 3,    /* it used max_segments segments without ending: value 0 (not in the reference) */
    RL_PATH_END_INVALID = 4   /* its wavelength is not finite: value 0, no segment (not in the reference) */
};

typedef struct RlPathResult {
    float value;       /* render_ray's return value (trace_unit.rs:81-132); 0 for every end but RL_PATH_END_EMITTER */
    uint32_t segments; /* Scene::intersect calls the path made */
    uint32_t object;   /* the emitter the path ended on; RL_OBJECT_NONE for any other end */
    uint32_t end;      /* enum RlPathEnd */
} RlPathResult;        /* 16 bytes */

#define RL_PATH_MAX_SEGMENTS 4096     /* max_segments = 0 */
#define RL_PATH_MAX_SEGMENTS_CAP 65536 /* the largest max_segments accepted */

/* rl_scene_camera_rays: the camera half of a path.  samples[i] is what path first_path_index + i of RNG stream `stream` under
 * `seed` draws from blocks 0 and 1 (rl_rng.h) for a width x height image, turned into a ray: its wavelength, its screen position
 * x, y and the camera ray (rl_trace_unit_render's camera for a trace unit of that size).  width or height 0, or
 * width * height > RL_MAX_PIXELS, is RL_E_INVALID.
 *
 * rl_scene_render_rays: the other half, TraceUnit::render_ray (trace_unit.rs:81-132) for rays[i] as path first_path_index + i of
 * stream `stream` under `seed`: bounce b draws from block 2 + b, which is what a camera path of that index draws after its camera
 * ray.  The path starts with intensity 1 and continue chance 1 and follows the reference's loop (Scene::intersect, the material's
 * new ray, the 1e-5 offset, continue chance * 0.96, Russian roulette) until it ends; results[i] says how (RlPathResult).
 *   Identity.  For any scene, image size, seed, stream and path range: feed rl_scene_camera_rays(...)[i].ray to
 *   rl_scene_render_rays with the same seed, stream and first_path_index; then results[i].value equals, bit for bit, the
 *   `probability` of photon i of rl_trace_unit_render for those paths, samples[i].x, .y and .ray.wavelength equal that photon's
 *   x, y and wavelength, and the sum of results[].segments equals the segments rl_trace_unit_stats reports for those paths.
 *   Determinism.  A result depends only on (scene, seed, stream, path index, ray, max_segments): not on how a batch is split, on
 *   primitive_fetch or the kernel variant, or on other callers.
 *   Rays as given.  A segment whose direction is not within 2^-20 of unit length (|d|^2 further than 2^-20 from 1), or whose
 *   origin or direction has a non-finite component, is intersected by an exact linear scan (the scan's culls assume a unit
 *   direction, see rl_scene_intersect).  This is decided per segment: glass refraction and mirror reflection keep a non-unit
 *   direction's length, so such a ray stays non-unit after those bounces.
 *   Invalid wavelength (a deviation from the reference).  A ray with a NaN or infinite wavelength returns {0, 0 segments,
 *   RL_OBJECT_NONE, RL_PATH_END_INVALID} without any scan: its intensity would be NaN, which never ends the roulette, and inside a
 *   closed scene the path would never end.  Finite wavelengths outside [380, 780] nm are traced as given.
 *   Segment limit (a deviation from the reference).  max_segments = 0 means RL_PATH_MAX_SEGMENTS (4096); otherwise it must be
 *   1 .. RL_PATH_MAX_SEGMENTS_CAP (65536), a larger value is RL_E_INVALID.  A path that has used max_segments segments and not
 *   ended returns value 0 and RL_PATH_END_LIMIT: the kernel's guarantee that it terminates.  At the default it changes no result
 *   of a path with a finite wavelength in practice: from bounce ~2,500 on its f32 continue chance sits at its floor (1.7e-44), and
 *   the path goes on only where a bounce's roulette draw is exactly 0 (probability 2^-24 each).
 * Both calls, and their _device forms, work as rl_scene_intersect* do: n = 0 does nothing; a NULL scene, an unknown fetch mode,
 * NULL buffers with n > 0 or path indices that reach 2^64 - 1 are RL_E_INVALID before any device work; the host forms stage the
 * arrays through device buffers in chunks of 2^20 records, the _device forms take device pointers on the scene's device and
 * refuse pageable host memory; all of them return when the results are written, are safe from several host threads at once on
 * one scene, and order against renders as a query does: a call made while an open launch runs on the device (a blocking render in
 * flight, or one begun with rl_trace_unit_render_begin / _fused_begin and not yet ended) waits until that launch drains, which it
 * does by itself (rl_scene_intersect), so a call between _begin and _end completes and does not disturb the render. */
int rl_scene_camera_rays(const RlScene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream,
                         uint64_t first_path_index, uint32_t n, RlCameraSample* samples);
int rl_scene_camera_rays_device(const RlScene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t stream,
                                uint64_t first_path_index, uint32_t n, RlCameraSample* device_samples);
int rl_scene_render_rays(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                         uint32_t max_segments, const RlSpectralRay* rays, uint32_t n_rays, RlPathResult* results);
int rl_scene_render_rays_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                uint64_t first_path_index, uint32_t max_segments, const RlSpectralRay* device_rays,
                                uint32_t n_rays, RlPathResult* device_results);

/* ---- one turn of render_ray's loop at a time: path states the caller holds ------------------- */

#define RL_PATH_LIVE 0xffffffffu /* RlPathState::end of a path that has not ended */
#define RL_STEP_NO_ROULETTE 1u   /* rl_scene_step_paths flags: the roulette's outcome is ignored */

/* Everything TraceUnit::render_ray carries from one turn of its loop to the next (trace_unit.rs:81-132), plus how the path
 * ended.  Frozen: 16 words. */
typedef struct RlPathState {
    RlVector3 origin;       /* the next segment's ray, as RlSpectralRay */
    float wavelength;       /* nm */
    RlVector3 direction;    /* used as given, not normalised */
    float intensity;        /* trace_unit.rs:88 */
    float continue_chance;  /* trace_unit.rs:84 */
    uint32_t segments;      /* Scene::intersect calls made so far; the next bounce draws RNG block 2 + segments.  That sum, the
                               light sample's 2^31 + segments and the step's segments + 1 are 32-bit: they wrap. */
    uint32_t end;           /* RL_PATH_LIVE, or an enum RlPathEnd value */
    float value;            /* RlPathResult::value once the path has ended, 0 while it is live */
    uint64_t path_index;    /* the RNG path of this state: it travels with the record */
    uint32_t object;        /* the emitter the path ended on, else RL_OBJECT_NONE */
    uint32_t reserved;      /* written 0 */
} RlPathState;              /* 64 bytes */

/* A wavefront form of rl_scene_render_rays: the path state lives in the caller's buffer, and every call makes one segment, so
 * that the caller can act between segments (end paths by a rule of their own, record vertices, cast shadow rays from a vertex
 * with rl_scene_occluded, re-weight or re-aim paths).
 *
 * rl_scene_begin_paths: states[i] is rays[i] as path first_path_index + i before its first segment: intensity 1, continue
 * chance 1, segments 0, value 0, object RL_OBJECT_NONE, end RL_PATH_LIVE.  A ray with a NaN or infinite wavelength gets end
 * RL_PATH_END_INVALID (rl_scene_render_rays' rule) and is never stepped.
 *
 * rl_scene_step_paths: every state with end == RL_PATH_LIVE makes exactly one segment, in place: Scene::intersect for the
 * state's ray (by the exact linear scan where rl_scene_render_rays takes it, decided per segment), segments += 1, then the
 * rest of the loop body as path path_index of stream `stream` under `seed`.
 *   The Void: end = RL_PATH_END_VOID.  An emitter: end = RL_PATH_END_EMITTER, value = intensity * get_intensity(wavelength),
 *   object = the emitter.  In both cases the ray, intensity and continue chance stay as they were.
 *   Any other hit: origin (with the 1e-5 offset), direction, intensity and continue chance (* 0.96) become what render_ray makes
 *   of them; if the roulette ends the path, end = RL_PATH_END_ROULETTE.
 *   A state that is not live is not written: every byte of the record stays as it is.
 *   hits may be NULL.  Otherwise hits[i] of every stepped state is, bit for bit, what rl_scene_intersect returns for that
 *   segment's ray with t_max = INFINITY; hits[i] of a state that was not stepped is left as it is.
 *   flags: 0 or RL_STEP_NO_ROULETTE.  With the flag the roulette's outcome is ignored and the state stays live; it is otherwise
 *   identical, including continue_chance * 0.96, so a caller who applies the reference's comparison themselves
 *   (`unit(word 2 of block 2 + segments - 1) * 0.85 > continue_chance * (1 - exp(intensity * -20))`) gets the reference's path.
 *   There is no segment limit: the caller's loop is the limit.
 * Identity.  For any scene, seed, stream, rays and first index: rl_scene_begin_paths, then rl_scene_step_paths with flags 0
 *   repeated until no state is live -- with or without the caller compacting or reordering the states between steps -- leaves
 *   {value, segments, object, end} of each state equal, bit for bit, to rl_scene_render_rays' RlPathResult for that ray, for
 *   every path that rl_scene_render_rays ends before its max_segments.
 * Determinism.  A stepped state depends only on the scene, seed, stream, flags and the state itself: not on its position in
 *   the batch, on how a batch is split, on primitive_fetch or the kernel variant, or on other callers.
 * The four calls work as rl_scene_render_rays* do: n == 0 does nothing; the arguments are checked in this order, each
 * failure RL_E_INVALID with a message before any device work: an unknown fetch mode, an unknown flag bit, NULL rays or states
 * with n > 0, a NULL scene, path indices that reach 2^64 - 1 (rl_scene_begin_paths).  The host forms stage the records through
 * device buffers in chunks of 2^20; the _device forms take device pointers on the scene's device (states 16-byte aligned) and
 * refuse pageable host memory.  All of them return when the states and hits are written, are safe from several host threads
 * at once on one scene (on different states), and order against renders as rl_scene_intersect does: a call waits for an open
 * launch to drain, so a call between rl_trace_unit_render_begin and _end completes and does not disturb the render. */
int rl_scene_begin_paths(const RlScene* scene, uint64_t first_path_index, const RlSpectralRay* rays, uint32_t n,
                         RlPathState* states);
int rl_scene_begin_paths_device(const RlScene* scene, uint64_t first_path_index, const RlSpectralRay* device_rays, uint32_t n,
                                RlPathState* device_states);
int rl_scene_step_paths(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                        RlPathState* states, uint32_t n, RlRayHit* hits);
int rl_scene_step_paths_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                               RlPathState* device_states, uint32_t n, RlRayHit* device_hits);

/* rl_scene_step_paths for the states an index list names, and the list of those that are still live: what a wavefront loop
 * needs between segments, so that it moves 4 bytes per live path instead of the 64-byte records.  The states stay where they are.
 *
 * The list.  list[k], k < n_list, names states[list[k]] of states[0, n_states).  list == NULL is the identity list
 *   0 .. n_list - 1; then n_list > n_states is RL_E_INVALID.  An entry >= n_states is skipped: nothing is read or written for it
 *   and it is not reported live; no content of the list makes the call touch memory outside the buffers.  Entries must be
 *   distinct: for a state named twice the call is memory-safe and that state's result is unspecified.  list is never written.
 * Stepping.  Every listed state with end == RL_PATH_LIVE makes exactly one segment, in place: bit for bit what
 *   rl_scene_step_paths makes of that record under the same seed, stream and flags.  hits may be NULL; otherwise hits[i] --
 *   indexed by STATE, not by list position, so it has room for n_states records -- is written for every stepped state i as that
 *   call writes it.  A listed state that is not live is not written.  A state that is not listed is neither read nor written, nor
 *   is its hits slot.
 * Survivors.  live_list may be NULL; otherwise it has room for n_list entries and receives the indices of the listed states that
 *   are live after the step: each exactly once, in the order they had in list (a stable compaction; ascending when list was),
 *   and nothing is written behind them.  *n_live (n_live may be NULL) receives their number on return, whether or not live_list
 *   is given.  The _device form accepts live_list == list.  The order is fixed so that the call is deterministic like every other
 *   call here, and so that neighbouring paths stay neighbours in the next step's waves.
 * Determinism.  States, hits, live_list and n_live depend only on the scene, seed, stream, flags, the states and the list: not
 *   on primitive_fetch or the kernel variant, on how the work is handed out, or on other callers.
 * Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: an unknown fetch mode, an
 *   unknown flag bit, NULL states with n_list > 0, a NULL scene, list == NULL with n_list > n_states.  n_list == 0 does nothing
 *   but *n_live = 0.
 * The _device form takes device pointers on the scene's device for states (16-byte aligned), list, hits and live_list (4-byte
 *   aligned) and refuses pageable host memory; n_live is a HOST pointer.  It returns when everything is written, is safe from
 *   several host threads at once on one scene (on different states), and orders against renders as rl_scene_intersect does.
 * The host form is a convenience and is NOT chunked: it copies the whole arrays (states, hits, list) into device buffers of the
 *   call's own, runs the device path, copies states, hits and the n_live entries of live_list back, and frees the buffers.
 * Scratch memory.  For the compaction (live_list or n_live given) the library keeps device scratch of at most 4 bytes per listed
 *   state plus 4 bytes per 64 listed states (rounded up), for the largest n_list seen: it lives with the query context the call
 *   runs on (one per concurrent caller and device), grows on demand and is reused. */
int rl_scene_step_path_list(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                            RlPathState* states, uint32_t n_states, const uint32_t* list, uint32_t n_list, RlRayHit* hits,
                            uint32_t* live_list, uint32_t* n_live);
int rl_scene_step_path_list_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, uint32_t flags,
                                   RlPathState* device_states, uint32_t n_states, const uint32_t* device_list, uint32_t n_list,
                                   RlRayHit* device_hits, uint32_t* device_live_list, uint32_t* n_live);

/* ---- direct light at a path vertex (not in the reference: "there is always an option of trying direct illumination, which
 * could be implemented here, but is not", trace_unit.rs:128-131) ---------------------------------------------------------- */

/* The sampleable emitters of a scene, fixed at rl_scene_create: the objects whose material is RL_MATERIAL_BLACK_BODY and whose
 * surface is an RL_SURFACE_SPHERE with a finite radius > 0, or an RL_SURFACE_CIRCLE with a finite radius > 0 and a normal whose
 * |n|^2 is within 2^-20 of 1.  Planes, paraboloids and prisms are unbounded or have no simple area measure: they are never
 * sampled, and paths still end on them as before.  rl_scene_emitters writes their object indices in scan order; host-only, no
 * device work; rl_scene_builtin_desc's capacity protocol: *n_emitters receives their number, and when cap is too small (or
 * objects is NULL with emitters to report) the call returns RL_E_INVALID with *n_emitters set.  A NULL scene or a NULL
 * n_emitters is RL_E_INVALID. */
int rl_scene_emitters(const RlScene* scene, uint32_t* objects, uint32_t cap, uint32_t* n_emitters);

enum RlLightStatus {
    RL_LIGHT_SKIPPED = 0,    /* no sample was drawn for this state (rule below) */
    RL_LIGHT_BACKFACING = 1, /* a point was drawn, but it is not in front of both surfaces: no ray cast */
    RL_LIGHT_OCCLUDED = 2,   /* the shadow ray is blocked */
    RL_LIGHT_VISIBLE = 3     /* it is not: value is the contribution */
};

typedef struct RlLightSample {
    RlVector3 direction; /* unit vector from the vertex to the sampled point; zero when SKIPPED */
    float distance;      /* from the vertex to the sampled point; 0 when SKIPPED */
    float value;         /* state.intensity * weight when VISIBLE, else 0 */
    float weight;        /* emitted intensity * geometry term * area * n_emitters / pi, whatever the ray found;
                            0 when SKIPPED or BACKFACING */
    uint32_t emitter;    /* object index of the sampled emitter; RL_OBJECT_NONE when SKIPPED */
    uint32_t status;     /* enum RlLightStatus */
} RlLightSample;         /* 32 bytes */

/* Next-event estimation for path states a step has just moved: for every listed state the call picks one of the scene's
 * sampleable emitters and a point on it, casts the shadow ray from the state's last vertex on rl_scene_occluded's bounded scan, and
 * writes the connection's contribution.  hits[i] must be the record rl_scene_step_paths* / rl_scene_step_path_list* wrote for
 * state i's last segment: the call trusts its position, normal and object, and no content of any buffer makes it touch memory
 * outside the buffers.
 *
 * The list is rl_scene_step_path_list's: list == NULL is the identity list 0 .. n_list - 1 (then n_list > n_states is
 *   RL_E_INVALID); an entry >= n_states is skipped with nothing read or written; entries must be distinct (a state named twice is
 *   memory-safe and its sample unspecified).  hits and samples are indexed by STATE and have room for n_states records.  states,
 *   hits and list are never written.  samples[i] is written, all 32 bytes, for every listed state i < n_states; samples[j] of a
 *   state that is not listed is not touched.
 * Which states get a sample.  State i is sampled if its end is RL_PATH_LIVE or RL_PATH_END_ROULETTE (the vertex exists either
 *   way), segments >= 1, hits[i].object < the scene's object count, that object's material is RL_MATERIAL_DIFFUSE_GREY or
 *   RL_MATERIAL_DIFFUSE_COLOURED (the two whose BRDF the library can state: glossy, glass and soap vertices are not sampled) and
 *   the scene has at least one sampleable emitter.  Every other listed state gets RL_LIGHT_SKIPPED: every field zero but
 *   emitter = RL_OBJECT_NONE.
 * The sample, all in f32 without contraction, in this order (csrc/rl_core.h: rl_light_sample, the same function on the device
 *   and in the host's rl_debug_light_sample):
 *   Draws.  w = Philox block 0x80000000 + state.segments (32-bit sum) of (seed, stream, state.path_index): disjoint from the
 *     path's own blocks (csrc/rl_rng.h).  k = ((uint64_t)w[2] * n_emitters) >> 32 picks emitter k of rl_scene_emitters' list;
 *     u = closed01(w[0]) in [0, 1]; phi = the half-open longitude of w[1] in [0, 2 pi); slot 3 is unused.
 *   A sphere (c, R): z = 1 - 2u, r = sqrt(max(0, 1 - z z)), nl = (r cos phi, r sin phi, z), q = c + nl R, area4 = 4 R R.
 *   A circle (n, p, R): r = R sqrt(u), q = p + rotate_towards((r cos phi, r sin phi, 0), n) (vector3.rs:69-83), nl = n,
 *     area4 = R R.
 *   The vertex: x = hits[i].position; facing = hits[i].normal if dot(state.direction, hits[i].normal) >= 0, else its negation --
 *     the side the path leaves on (the state holds the bounced ray, and a diffuse bounce leaves on the facing side);
 *     v = q - x, d2 = dot(v, v), distance = sqrt(d2), direction = normalise(v) (vector3.rs:56-67);
 *     cos_s = dot(facing, direction); cos_l = -dot(nl, direction) for a sphere and |dot(nl, direction)| for a circle, which emits
 *     from both faces as in the reference.
 *   RL_LIGHT_BACKFACING unless cos_s > 0, cos_l > 0 and d2 > 0 with all three finite: weight and value 0, no ray.  If d2 is not
 *     a finite number > 0 (a vertex on the sampled point, a hit record that is not finite), direction and distance are written
 *     zero as well.
 *   weight = (L * ((cos_s * cos_l) / d2)) * (area4 * (float)n_emitters), L = (float)planck(wavelength, kelvins) * normalisation:
 *     get_intensity of the emitter at the state's wavelength (material.rs:61-74,101-105).  The pi of the diffuse BRDF and the pi
 *     of the area cancel, and state.intensity already carries the reflectance (the reference's diffuse bounce is cosine-weighted
 *     with probability = reflectance).
 *   The shadow ray: origin x + direction * 1e-5 (the reference's offset, trace_unit.rs:114), the direction above,
 *     t_max = (distance - 1e-5) * 0.9990234375.  The factor 1 - 2^-10 keeps the emitter from blocking its own point: an occluder in
 *     the last 2^-10 of the segment is NOT seen.  The ray is blocked exactly when rl_scene_occluded returns 1 for that RlRay,
 *     including its rays-as-given rule for the exact linear scan.  Blocked: RL_LIGHT_OCCLUDED, value 0.  Otherwise
 *     RL_LIGHT_VISIBLE, value = state.intensity * weight.
 * Determinism.  A sample depends only on the scene, seed, stream, the state and its hit: not on primitive_fetch or the kernel
 *   variant, on the list, on how a batch is split, or on other callers.
 * Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: an unknown fetch mode; NULL
 *   states, hits or samples with n_list > 0; a NULL scene; list == NULL with n_list > n_states.  n_list == 0 does nothing.
 * The _device form takes device pointers on the scene's device -- states and samples 16-byte aligned, list 4-byte aligned, hits as
 *   the step calls take them -- refuses pageable host memory and returns when the samples are written.  The host form is NOT
 *   chunked: like rl_scene_step_path_list it copies the whole arrays (states, hits, list, samples) through device buffers of the
 *   call's own.  Both are safe from several host threads at once on one scene and order against open launches as
 *   rl_scene_intersect does.
 * Counting light once.  A path that ENDS on an emitter listed by rl_scene_emitters directly after a diffuse-grey or
 *   diffuse-coloured vertex carries light that this call's sample at that vertex has already estimated.  A caller who adds
 *   samples drops, or weights, that RlPathState::value.  The library does not do it for them. */
int rl_scene_light_paths(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream, const RlPathState* states,
                         uint32_t n_states, const uint32_t* list, uint32_t n_list, const RlRayHit* hits, RlLightSample* samples);
int rl_scene_light_paths_device(const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                const RlPathState* device_states, uint32_t n_states, const uint32_t* device_list, uint32_t n_list,
                                const RlRayHit* device_hits, RlLightSample* device_samples);

/* Largest image the units and rl_app_run accept: width * height <= RL_MAX_PIXELS = 2^31 - 1.  The kernels index
 * pixels in 32 bits: the splat's `py * width + px` is an int, the tonemap's pixel count and grid-stride index are
 * uint32_t.  rl_trace_unit_create, rl_plot_unit_create, rl_gather_unit_create, rl_tonemap_unit_create and rl_app_run
 * return RL_E_INVALID with a message naming the limit for a larger image, before they touch a device. */
#define RL_MAX_PIXELS 2147483647

/* ---- TraceUnit (trace_unit.rs:51-168) ------------------------------------------------------ */

/* TraceUnit::new(id, width, height) (trace_unit.rs:64-77); n_photons is the batch size the
 * reference fixes at 1024*512 (trace_unit.rs:67). */
int rl_trace_unit_create(int device, uint32_t id, uint32_t width, uint32_t height, uint32_t n_photons,
                         RlTraceUnit** out);
int rl_trace_unit_destroy(RlTraceUnit* unit);
/* Selects RL_FETCH_LDS (default) or RL_FETCH_GLOBAL for subsequent renders. */
int rl_trace_unit_set_fetch(RlTraceUnit* unit, int primitive_fetch);

/* ---- wavelength importance sampling (not in the reference, which draws every wavelength uniformly: trace_unit.rs:152) ----
 * A table turns a path's first random word into a wavelength whose density follows an importance, and gives the path the
 * reciprocal of that density (relative to uniform) as a weight, so the film's expectation is that of the uniform draw.
 *
 * The table.  M = RL_WAVELENGTH_BINS = 256.  `importance` is n_nodes doubles at equally spaced wavelengths from 380 to 780 nm
 * inclusive, 2 <= n_nodes <= 4096 (NULL: uniform); uniform_share = u in (0, 1] is the part of the density that stays uniform.
 * f64, in exactly this order, never contracted, divides correctly rounded:
 *   g_k = importance[k] if it is finite and > 0, else 0;  m_j = (g_j + g_{j+1}) * 0.5 for j < n - 1;
 *   G = the sequential sum of the m_j from +0.0 (an infinite G: RL_E_INVALID);
 *   d_j = 1 / (n - 1) for a NULL importance or G == 0, else u / (n - 1) + (1 - u) * (m_j / G);
 *   C_0 = 0, C_{j+1} = C_j + d_j;
 *   for i = 0 .. M:  T_i = ((double)i / M) * C_{n-1};  j = the largest index <= n - 2 with C_j <= T_i;
 *                    lambda_i = 380 + (400 / (n - 1)) * (j + (T_i - C_j) / d_j);  Q_i = (float)lambda_i,
 *                    with Q_0 = 380 and Q_M = 780 set exactly;
 *   Q must increase strictly, else RL_E_INVALID (the share is too small for f32);
 *   W_i = (float)(((double)Q_{i+1} - (double)Q_i) * M / 400.0).
 * The weight is taken from the ROUNDED quantiles: it is exactly the reciprocal of the density the device samples.
 *
 * A path.  f32, in this order, never contracted.  w0 = word 0 of the path's RNG block 0, v = w0 >> 8 (the 24 bits the uniform
 * draw reads), i = v >> 16, f = (float)(v & 0xffff) * 2^-16, lambda = Q[i] + (Q[i+1] - Q[i]) * f.  Every other draw of the
 * path, and everything made of lambda (the camera's chromatic zoom, the index of refraction), is the uniform path's word for
 * word.  bin_of(lambda) = the largest i <= M - 1 with Q[i] <= lambda; the path's weight is W[bin_of(lambda)], a function of
 * lambda alone, and enters once: value = emission * W, one f32 multiply.  RlMappedPhoton::probability carries it, so
 * rl_plot_unit_plot and rl_spectral_unit_plot of such photons stay unbiased as they are.
 *
 * rl_wavelength_table_create checks, each RL_E_INVALID and before any device work, in this order: NULL out; n_nodes outside
 * 2..4096; a share outside (0, 1] or NaN; the rule's own refusals.  _download: 257 quantiles and 256 weights, either pointer may
 * be NULL.  rl_wavelength_importance_cie1931: x-bar + y-bar + z-bar of the CIE 1931 observer at its 81 nodes (host only). */
#define RL_WAVELENGTH_BINS 256
int rl_wavelength_table_create(int device, const double* importance, uint32_t n_nodes, double uniform_share,
                               RlWavelengthTable** out);
int rl_wavelength_table_destroy(RlWavelengthTable* table);
int rl_wavelength_table_download(RlWavelengthTable* table, float* quantiles, float* weights);
int rl_wavelength_importance_cie1931(double* out);
/* Selects the table for subsequent renders of the unit -- every render call: render, _begin, _async, _fused, _fused_sync,
 * _fused_begin -- as rl_trace_unit_set_fetch selects the fetch mode; NULL restores the reference's uniform draw.  The table must
 * outlive the renders it was set for.  A table on another device than the unit's, or a call while a render begun on the unit
 * has not ended: RL_E_STATE.  The table joins the combination under which calls share an open launch (rl_trace_unit_render_begin);
 * a begun render for a fifth combination takes the plain launch described there, with the table. */
int rl_trace_unit_set_wavelengths(RlTraceUnit* unit, const RlWavelengthTable* table);
/* TraceUnit::render(&mut self, &Scene) (trace_unit.rs:151-168): fills the unit's mapped_photons.
 * Photon i of this call is path (first_path_index + i) of RNG stream `stream` under `seed`.
 * Complete on return: mapped_photons may be plotted or downloaded.  Calls made from several threads (the reference's
 * workers, app.rs:92-134) on units of one device with the same scene, seed, stream and image size share OPEN
 * LAUNCHES: a call whose batch is a multiple of 64 paths is appended to a trace kernel that is already running on
 * the device if there is one (otherwise it starts one), and returns as soon as ITS paths are finished while the
 * kernel goes on with the other callers' -- so nothing is launched per call and the drain tail of one batch overlaps
 * the next batches.  The results are bit-identical to separate launches.  Path and segment counters are kept per
 * call; the run time of an open launch is split among the units whose calls it carried, by paths, when it has ended. */
int rl_trace_unit_render(RlTraceUnit* unit, const RlScene* scene, uint64_t seed, uint32_t stream,
                         uint64_t first_path_index);
/* rl_trace_unit_render in two halves, for a host thread that has something else to do meanwhile (feeding other GPUs,
 * taking the next task: rl_app_run does both): _begin appends the call to the device's open launch (or starts one) and
 * returns at once, _end waits until the call's paths are finished (a no-op without a begun render).  One begun render
 * per unit at a time.  Everything that reads mapped_photons ends a begun render by itself: rl_plot_unit_plot (for the
 * units it plots), rl_trace_unit_photons, rl_trace_unit_sync, rl_trace_unit_stats, rl_trace_unit_destroy.  The thread
 * that ends a render need not be the one that began it, as long as the unit changes hands the way every unit must
 * (one user at a time, handed over through a lock or a channel -- the reference's Task does that).
 * A device runs at most FOUR open launches at a time, one per (scene, seed, stream, image size, fetch mode, fused or not)
 * combination in use.  A render begun for a fifth combination while begun-and-not-ended renders hold all four is not
 * refused and does not wait: it gets a plain launch of its own on the unit's stream (same results; _end waits for it). */
int rl_trace_unit_render_begin(RlTraceUnit* unit, const RlScene* scene, uint64_t seed, uint32_t stream,
                               uint64_t first_path_index);
int rl_trace_unit_render_end(RlTraceUnit* unit);
/* The same without the final wait: the launch is queued on the unit's stream and rl_trace_unit_sync() (or
 * rl_plot_unit_plot, which orders itself after it on the device) completes it.  Lets one host thread start the
 * same task on several GPUs before waiting for any of them. */
int rl_trace_unit_render_async(RlTraceUnit* unit, const RlScene* scene, uint64_t seed, uint32_t stream,
                               uint64_t first_path_index);
/* Fused TraceUnit::render + PlotUnit::plot (trace_unit.rs:151-168 + plot_unit.rs:87-95): traces
 * n_paths paths (any count, not limited to the unit's batch size) and splats every non-zero
 * contribution straight into `plot` with f32 atomics; mapped_photons is not written.  After this a
 * rl_plot_unit_plot for the same photons must NOT be issued.  Asynchronous on the unit's stream;
 * rl_trace_unit_sync() or any download waits for it. */
int rl_trace_unit_render_fused(RlTraceUnit* unit, const RlScene* scene, RlPlotUnit* plot, uint64_t seed,
                               uint32_t stream, uint64_t first_path_index, uint64_t n_paths);
/* The same, complete on return, for hosts whose workers wait for their task anyway (the reference's do): calls on
 * units of one device (same scene, seed, stream, image size; n_paths a multiple of 64) share open launches like
 * rl_trace_unit_render's, each splatting into its own call's plot unit.  Results are those of separate calls up to
 * the order of the float atomics. */
int rl_trace_unit_render_fused_sync(RlTraceUnit* unit, const RlScene* scene, RlPlotUnit* plot, uint64_t seed,
                                    uint32_t stream, uint64_t first_path_index, uint64_t n_paths);
/* Its first half.  The begun render belongs to `plot` -- the trace unit is free for the next call, on any thread, at
 * once and may even be destroyed -- and is ended by whatever uses the plot unit's buffer next: rl_plot_unit_sync,
 * rl_gather_unit_accumulate / _allreduce, rl_plot_unit_reduce / _add / _plot / _clear / _download / _upload /
 * _device_buffer / _destroy, or another render begun into it.  Its paths and segments appear in the trace unit's
 * rl_trace_unit_stats once it has ended. */
int rl_trace_unit_render_fused_begin(RlTraceUnit* unit, const RlScene* scene, RlPlotUnit* plot, uint64_t seed,
                                     uint32_t stream, uint64_t first_path_index, uint64_t n_paths);
int rl_trace_unit_sync(RlTraceUnit* unit);
/* Copies mapped_photons (trace_unit.rs:56) to host memory; `out` holds n_photons entries. */
int rl_trace_unit_photons(RlTraceUnit* unit, RlMappedPhoton* out);
/* Cumulative counters since creation: paths traced and path segments (= Scene::intersect calls,
 * scene.rs:39) and the device time spent in trace kernels in milliseconds. */
int rl_trace_unit_stats(RlTraceUnit* unit, uint64_t* paths, uint64_t* segments, double* kernel_ms);

/* ---- PlotUnit (plot_unit.rs:23-102) -------------------------------------------------------- */

/* PlotUnit::new(id, width, height) (plot_unit.rs:43-52).  If external_xyz is non-NULL it must be
 * a device pointer to width*height*3 floats on `device` that outlives the unit (lets the caller
 * run a collective on the buffer); otherwise the unit allocates and zeroes its own. */
int rl_plot_unit_create(int device, uint32_t id, uint32_t width, uint32_t height, float* external_xyz,
                        RlPlotUnit** out);
int rl_plot_unit_destroy(RlPlotUnit* unit);
/* PlotUnit::plot(&mut self, &[MappedPhoton]) for each given trace unit (app.rs:136-141).  ASYNCHRONOUS: the
 * splat kernels are queued on the plot unit's own (non-blocking) stream, after the trace units' renders; the
 * trace units may be rendered again at once (their next render waits for this plot on the device).  A later
 * rl_gather_unit_accumulate / rl_plot_unit_reduce / rl_plot_unit_download of this unit is ordered after it;
 * anything else that reads the buffer (rl_plot_unit_device_buffer) must call rl_plot_unit_sync first. */
int rl_plot_unit_plot(RlPlotUnit* unit, RlTraceUnit* const* trace_units, uint32_t n_trace_units);
/* PlotUnit::clear (plot_unit.rs:98-102); queued on the unit's stream. */
int rl_plot_unit_clear(RlPlotUnit* unit);
/* Blocks until everything queued into this plot unit so far (plots, fused renders, exchanges, clears) is done. */
int rl_plot_unit_sync(RlPlotUnit* unit);
/* Device pointer of tristimulus_buffer (plot_unit.rs:35): width*height RlVector3, row-major. */
int rl_plot_unit_device_buffer(RlPlotUnit* unit, float** device_xyz);
int rl_plot_unit_download(RlPlotUnit* unit, RlVector3* out);
/* Overwrites tristimulus_buffer from host memory (after everything queued into the unit): the host-staged form
 * of the exchange, for ranks that share a GPU, and the tests. */
int rl_plot_unit_upload(RlPlotUnit* unit, const RlVector3* in);
/* PlotUnit::plot(&mut self, &[MappedPhoton]) (plot_unit.rs:87-95) for photons the caller holds: for every photon with
 * probability != 0, get_tristimulus(wavelength) * probability (cie1931.rs:20-48) is added to the four pixels of
 * plot_pixel(x, y) (plot_unit.rs:56-84) with f32 atomics, onto what the buffer holds.  Photons are used as given: x, y outside
 * the screen clamp to the border pixels as in the reference, a wavelength outside [375, 785) nm contributes zero, a negative
 * probability subtracts, a non-finite probability or wavelength is plotted as the arithmetic gives (NaN or inf into at most four
 * pixels of the image).
 *   Non-finite position (a deviation from the reference).  A photon whose x or y is NaN or infinite is skipped: the reference's
 *   `floor() as isize` of such a value is not something to match, and no input ever indexes outside the buffer.
 * The host form takes any n and stages the photons through a device buffer in chunks of 2^20 records; the _device form takes a
 * device pointer on the plot unit's device and refuses pageable host memory (as rl_scene_render_rays_device does).  n = 0 does
 * nothing; a NULL unit, or NULL photons with n > 0, is RL_E_INVALID before any device work.
 *
 * rl_plot_unit_render_samples: rl_scene_render_rays with a film.  samples[i].ray is traced as path first_path_index + i under every
 * rule of rl_scene_render_rays (RNG blocks, the exact scan for non-unit or non-finite segments, RL_PATH_END_INVALID for a non-finite
 * wavelength, max_segments), and a path that ends with value != 0 is splatted at samples[i].x, .y with samples[i].ray.wavelength
 * into `unit` by the arithmetic above, in the same kernel: no photon record is written.  The image size and aspect ratio are the
 * plot unit's.  A sample whose x or y is not finite is traced, not splatted; reserved fields are ignored.  If `results` is non-NULL
 * it receives exactly what rl_scene_render_rays writes for the same rays, bit for bit; if NULL nothing but the film is written.
 * Argument checks, in this order, each RL_E_INVALID before any device work: NULL unit, NULL scene, unknown fetch mode, max_segments
 * > RL_PATH_MAX_SEGMENTS_CAP, path indices that reach 2^64 - 1, NULL samples with n > 0.  `unit` and `scene` on different devices
 * is RL_E_STATE.  n = 0 does nothing.  Host and _device forms as above (the _device form's results, if given, are device memory).
 *
 * Ordering, all four calls.  They first end a render begun into `unit` with rl_trace_unit_render_fused_begin, run after everything
 * queued into the unit (plots, fused renders, clears, exchanges) and return when their splats are in the buffer, so a following
 * rl_gather_unit_accumulate, rl_plot_unit_download, _reduce or _add sees them.  The render_samples forms order against open
 * launches as rl_scene_render_rays does.  One user per plot unit at a time; several threads may render samples into different
 * plot units on one scene at once. */
int rl_plot_unit_plot_photons(RlPlotUnit* unit, const RlMappedPhoton* photons, uint64_t n);
int rl_plot_unit_plot_photons_device(RlPlotUnit* unit, const RlMappedPhoton* device_photons, uint64_t n);
int rl_plot_unit_render_samples(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* samples, uint32_t n,
                                RlPathResult* results);
int rl_plot_unit_render_samples_device(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                       uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* device_samples,
                                       uint32_t n, RlPathResult* device_results);

/* rl_plot_unit_light_paths: rl_scene_light_paths with a film.  Everything that call says about the list, the states that get a
 * sample, the draws, the arithmetic and the shadow ray holds unchanged; what it writes into a sample record this call splats into
 * `unit` in the same kernel, and it splats the value of a path that has just ended on a light unless that light was already
 * counted at the vertex before.  camera, sampled and samples are indexed by STATE and have room for n_states records (bytes);
 * only camera[i].x and .y are read.
 *   samples may be NULL.  Otherwise samples[i] receives, for every listed state i < n_states, exactly what rl_scene_light_paths
 *   writes, bit for bit; the record of a state that is not listed is not touched.
 *   Vertex splat.  A listed state whose sample is RL_LIGHT_VISIBLE with value != 0 is splatted: get_tristimulus(state.wavelength)
 *   * value onto the four pixels of plot_pixel(camera[i].x, camera[i].y), by rl_plot_unit_plot_photons' arithmetic.  The image
 *   size and aspect ratio are the plot unit's.  A state whose x or y is not finite is sampled, not splatted.
 *   Ending splat.  A listed state with end == RL_PATH_END_EMITTER and value != 0 is splatted with state.value in the same way,
 *   unless sampled != NULL, sampled[i] != 0 and state.object is one of rl_scene_emitters' objects: then the vertex before was
 *   sampled, that light is counted already and the ending is dropped.  Endings on emitters that are never sampled (planes,
 *   paraboloids, prisms) and endings reached from the camera or from a glossy, glass or soap vertex are always splatted.
 *   sampled may be NULL: then nothing is dropped and nothing is recorded.  Otherwise, for every listed state i < n_states, the
 *   byte is read (for the rule above) and then written: 1 if the state got a sample with a status other than RL_LIGHT_SKIPPED,
 *   else 0.  The caller zeroes the bytes when the paths begin; bytes of states that are not listed are not touched.
 *   The caller's part.  Each state is listed exactly once per step, in the call that follows the step that moved it: pass the list
 *   that rl_scene_step_path_list was GIVEN, not its live_list, so that the states that have just ended are seen once.  A state
 *   listed again after its end is splatted again; the library does not track it.
 *   Determinism as rl_scene_light_paths'; the film differs by the order of the float atomics.
 * Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: a NULL unit; a NULL scene;
 *   an unknown fetch mode; NULL states, hits or camera with n_list > 0; list == NULL with n_list > n_states.  `unit` and `scene`
 *   on different devices is RL_E_STATE.  n_list == 0 does nothing.
 * Ordering is rl_plot_unit_render_samples': the call ends a fused render begun into `unit`, runs after everything queued into the
 *   unit, returns when the splats are in the buffer, and orders against open launches as rl_scene_light_paths does.
 * The host form is NOT chunked, like rl_scene_light_paths.  The _device form takes device pointers on the unit's device -- states,
 *   samples and camera 16-byte aligned, list 4-byte aligned -- and refuses pageable host memory.
 *
 * rl_plot_unit_render_samples_direct: rl_plot_unit_render_samples with direct light.  For chunks of at most 2^20 samples the call
 * begins the paths of samples[i].ray (path first_path_index + i), zeroes their `sampled` bytes and loops: rl_scene_step_path_list
 * with hits, rl_plot_unit_light_paths over the list that step was given, and the step's live list becomes the next list; until no
 * path is live or max_segments segments are made.  The film receives what that loop of public calls puts there: a path at the
 * segment limit contributes the samples of its vertices and nothing more.  `results`, if given, equals rl_scene_render_rays'
 * output for samples[i].ray bit for bit -- direct light does not change the paths -- RL_PATH_END_INVALID and RL_PATH_END_LIMIT
 * included.  Argument checks and ordering are rl_plot_unit_render_samples'; the _device form wants device_samples 16-byte aligned.
 *   Scratch memory.  The loop's states, hits, bytes and two lists, 121 bytes per sample of the largest chunk seen (127 MB at
 *   2^20), live with the query context the call runs on (one per concurrent caller and device), grow on demand and are reused. */
int rl_plot_unit_light_paths(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                             const RlPathState* states, uint32_t n_states, const uint32_t* list, uint32_t n_list,
                             const RlRayHit* hits, const RlCameraSample* camera, uint8_t* sampled, RlLightSample* samples);
int rl_plot_unit_light_paths_device(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                    const RlPathState* device_states, uint32_t n_states, const uint32_t* device_list, uint32_t n_list,
                                    const RlRayHit* device_hits, const RlCameraSample* device_camera, uint8_t* device_sampled,
                                    RlLightSample* device_samples);
int rl_plot_unit_render_samples_direct(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                                       uint64_t first_path_index, uint32_t max_segments, const RlCameraSample* samples, uint32_t n,
                                       RlPathResult* results);
int rl_plot_unit_render_samples_direct_device(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed,
                                              uint32_t stream, uint64_t first_path_index, uint32_t max_segments,
                                              const RlCameraSample* device_samples, uint32_t n, RlPathResult* device_results);

/* What one rl_plot_unit_render_direct call did; every field an exact count. */
typedef struct RlDirectStats {
    uint64_t paths;           /* n_paths */
    uint64_t segments;        /* Scene::intersect calls: the sum of RlPathResult::segments */
    uint64_t light_samples;   /* vertices at which a point was drawn: status != RL_LIGHT_SKIPPED */
    uint64_t shadow_rays;     /* of those, rays cast: RL_LIGHT_OCCLUDED or RL_LIGHT_VISIBLE */
    uint64_t visible;         /* of those, RL_LIGHT_VISIBLE */
    uint64_t endings_kept;    /* paths that ended on an emitter with value != 0 and were splatted */
    uint64_t endings_dropped; /* ... and were dropped because the vertex before was sampled ("counting light once") */
} RlDirectStats;              /* 56 bytes */

/* rl_plot_unit_render_direct: direct light over paths of the RNG, into a film, in one persistent launch -- what
 * rl_scene_camera_rays followed by rl_plot_unit_render_samples_direct does, without the samples, the loop of launches or its
 * per-path buffers.
 *   Paths.  Path first_path_index + i, for i < n_paths, is the camera path of that index of stream `stream` under `seed`.  The
 *   image size is the plot unit's, unit.width x unit.height.  The camera sample is the one rl_scene_camera_rays returns; the path
 *   from that sample is rl_scene_render_rays' under every one of its rules, max_segments and RL_PATH_END_LIMIT included.
 *   Film.  The film receives exactly what rl_scene_camera_rays followed by rl_plot_unit_render_samples_direct puts there for the
 *   same arguments, up to the order of the float atomics: the vertex after every segment gets rl_scene_light_paths' sample (the
 *   state as rl_scene_step_path_list leaves it, a state the roulette has just ended included); a visible sample with value != 0
 *   is splatted at the path's screen position, and so is an ending on an emitter under rl_plot_unit_light_paths' drop rule.  A
 *   path at the segment limit contributes the samples of its vertices and nothing more.
 *   Results.  device_results may be NULL.  Otherwise it is a device pointer on the unit's device, 16-byte aligned, with room for
 *   n_paths records; pageable host memory is refused as in the other _device forms.  device_results[i] is bit for bit what
 *   rl_scene_render_rays writes for that path: direct light does not change the paths.
 *   Stats.  `stats` may be NULL and is a HOST pointer, written on return.  It depends only on the scene, seed, stream, path range,
 *   image size and max_segments -- not on the fetch mode, the kernel variant, how the work is handed out or how a range is split
 *   into calls: each field of [a, b) plus the same field of [b, c) equals that field of [a, c).
 *   Determinism.  Results and stats are exact; the film differs only by the order of the atomics.
 *   Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: a NULL unit; a NULL scene;
 *   an unknown fetch mode; max_segments > RL_PATH_MAX_SEGMENTS_CAP; path indices that reach 2^64 - 1; device_results not 16-byte
 *   aligned.  `unit` and `scene` on different devices is RL_E_STATE.  With n_paths == 0 the call does nothing, except that *stats
 *   becomes all zero.
 *   n_paths.  Any n_paths is accepted: the host may split the range into several launches, which it queues back to back without
 *   a synchronise between them, and it reads the counters once at the end.
 *   Ordering is rl_plot_unit_render_samples': the call first ends a fused render begun into `unit`, runs after everything queued
 *   into the unit, returns when the splats are in the buffer, and waits for an open launch to drain, as a query does.  One user
 *   per plot unit at a time; several threads may render into different plot units on one scene at once.
 *   No scratch memory that grows with n_paths: the call keeps no per-path buffer. */
int rl_plot_unit_render_direct(RlPlotUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                               uint64_t first_path_index, uint64_t n_paths, uint32_t max_segments, RlPathResult* device_results,
                               RlDirectStats* stats);

/* ---- denoising guides: albedo, shading normal and depth films (rl_scene_render_features) ---- */

enum RlFeatureKind {
    RL_FEATURE_VOID = 0,    /* the feature path left the scene */
    RL_FEATURE_EMITTER = 1, /* it reached a light */
    RL_FEATURE_DIFFUSE = 2, /* it reached a diffuse surface */
    RL_FEATURE_LIMIT = 3    /* it was still in mirrors, glass or bubbles after max_segments segments */
};

typedef struct RlFeatureSample {
    float x, y;          /* screen position: RlCameraSample x, y of the path */
    float wavelength;    /* nm */
    float albedo;        /* below; 0 for VOID and LIMIT */
    RlVector3 normal;    /* below; zero for VOID and LIMIT */
    float depth;         /* distance of the path's FIRST segment's hit (the camera ray is unit length); 0 if it hit nothing */
    uint32_t object;     /* the object at the feature vertex (EMITTER, DIFFUSE); RL_OBJECT_NONE otherwise */
    uint32_t segments;   /* Scene::intersect calls made for this record */
    uint32_t kind;       /* enum RlFeatureKind */
    uint32_t reserved;   /* written 0 */
} RlFeatureSample;       /* 48 bytes */

/* What one rl_scene_render_features call did; every field an exact count. */
typedef struct RlFeatureStats {
    uint64_t paths, segments, kinds[4]; /* n_paths; the sum of RlFeatureSample::segments; records per RlFeatureKind */
} RlFeatureStats;                       /* 48 bytes */

#define RL_FEATURE_MAX_SEGMENTS 64 /* max_segments = 0 */

/* rl_scene_render_features: the per-pixel guide images a denoiser or an edge-aware filter wants beside a noisy image -- the
 * albedo, the shading normal and the depth of what each pixel shows -- for paths of the RNG, accumulated with the image's own
 * reconstruction, in one persistent launch.  A guide taken at the first hit would show glass, so the guide follows the path
 * through mirrors, glass and bubbles to the first diffuse surface or light.
 *   The feature path of path first_path_index + i, for i < n_paths, is defined by public calls: take the sample
 *   rl_scene_camera_rays(scene, width, height, seed, stream, ...) returns for that index, pass it through rl_scene_begin_paths,
 *   then call rl_scene_step_paths with RL_STEP_NO_ROULETTE and hits, one segment at a time.  After each step, the first rule that
 *   applies ends the feature path:
 *     state.end == RL_PATH_END_VOID: VOID.
 *     state.end == RL_PATH_END_EMITTER: EMITTER; albedo = state.intensity, the throughput that reached the light (the step leaves
 *       it as it was); object = hits.object.
 *     the hit object's material is RL_MATERIAL_DIFFUSE_GREY or RL_MATERIAL_DIFFUSE_COLOURED: DIFFUSE; albedo = state.intensity
 *       after that step, the product of every `probability` factor from the camera up to and including the diffuse bounce;
 *       object = hits.object.
 *     state.segments == max_segments: LIMIT.
 *     otherwise (glossy mirror, SF10 glass, soap bubble) the path goes on.
 *   The path follows the true path's RNG blocks, 2 + segments: the feature vertex is a vertex of the path the renderer traces for
 *   that index, up to the roulette.
 *   The normal is hits.normal of the feature vertex, turned to face the ray that arrived: with d the state's direction before
 *   that step, normal = dot(d, n) < 0 ? n : -n (strict; -n flips each component's sign bit, so +0 becomes -0).
 *   max_segments = 0 means RL_FEATURE_MAX_SEGMENTS; otherwise it is 1 .. RL_PATH_MAX_SEGMENTS_CAP.
 *   The films.  Any of the three plot units may be NULL; that film is not written.  Each film takes rl_plot_unit_plot_photons'
 *   splat: the four pixels and weights of x, y under the unit's width, height and aspect ratio, each colour component times each
 *   weight added with f32 atomics onto what the buffer holds.
 *     albedo: colour get_tristimulus(wavelength) * albedo, only if albedo != 0 -- exactly rl_plot_unit_plot_photons of the photon
 *       {x, y, albedo, wavelength}.
 *     normal: colour (normal.x, normal.y, normal.z), for EMITTER and DIFFUSE.
 *     aux: colour (1, depth, (float)segments), for every path.
 *   Consumers normalise: aux.x is the reconstruction weight, aux.y / aux.x the mean depth, normal / |normal| the mean normal.
 *   Given units must be three distinct handles, else RL_E_INVALID; they must be width x height and on the scene's device, else
 *   RL_E_STATE and nothing is written.  They are plot units so that rl_gather_unit_accumulate, rl_plot_unit_reduce / _add,
 *   _download and _clear work on guides unchanged.
 *   Records.  device_records may be NULL.  Otherwise it is device memory on the scene's device, 16-byte aligned, with room for
 *   n_paths records; pageable host memory is refused as in the other _device forms.  All 48 bytes of every record are written.
 *   Stats.  `stats` may be NULL and is a HOST pointer, written on return; all zero for n_paths == 0.  It is exact, additive over
 *   any split of a range ([a, b) plus [b, c) equals [a, c)), and independent of the fetch mode, the kernel variant and how the work
 *   is handed out.
 *   Determinism.  Records and stats are exact; the films differ only by the order of the atomics.
 *   Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: a NULL scene; an unknown
 *   fetch mode; width or height 0, or width * height > RL_MAX_PIXELS; max_segments > RL_PATH_MAX_SEGMENTS_CAP; path indices that
 *   reach 2^64 - 1; device_records not 16-byte aligned; two given units that are the same handle.
 *   Ordering is rl_plot_unit_render_direct's, for each given unit: the call ends a fused render begun into the unit, runs after
 *   everything queued into it, returns when the splats are in the buffers, and waits for an open launch to drain, as a query
 *   does.  Any n_paths is accepted: launches of at most 2^30 paths queued back to back, the counters read once.  No scratch
 *   memory that grows with n_paths. */
int rl_scene_render_features(const RlScene* scene, int primitive_fetch, uint32_t width, uint32_t height, uint64_t seed,
                             uint32_t stream, uint64_t first_path_index, uint64_t n_paths, uint32_t max_segments,
                             RlPlotUnit* albedo, RlPlotUnit* normal, RlPlotUnit* aux, RlFeatureSample* device_records,
                             RlFeatureStats* stats);

/* ---- denoising: the edge-avoiding a-trous filter over the guides (rl_denoise_unit_denoise) ---- */

#define RL_DENOISE_ITERATIONS 5     /* iterations = 0 */
#define RL_DENOISE_MAX_ITERATIONS 6
typedef struct RlDenoiseParams {
    uint32_t iterations;   /* 0 = RL_DENOISE_ITERATIONS (5); otherwise 1 .. RL_DENOISE_MAX_ITERATIONS */
    float sigma_colour;    /* each sigma: 0 = that term off; otherwise in [1e-3, 1e3] */
    float sigma_normal;
    float sigma_depth;
    float sigma_albedo;
    uint32_t reserved[3];  /* must be 0 */
} RlDenoiseParams;         /* 32 bytes */

/* rl_denoise_unit_denoise: the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 -- `iterations` passes of a 5x5
 * B3-spline kernel at dilation 1, 2, 4, ..., each tap weighted by an edge-stopping term built from the image's own luminance and
 * from the guides rl_scene_render_features makes -- from one gather unit into another, on the device.  The chain is: render the
 * noisy image into a gather unit; render the guides into plot units and accumulate each into a gather unit; one denoise call;
 * rl_tonemap_unit_tonemap of `dst`.
 *   The unit owns the call's scratch, sized at creation: a 32-byte guide record per pixel and two width x height XYZ buffers.
 *   rl_denoise_unit_create refuses a zero size and width * height > RL_MAX_PIXELS as the other units do.
 *   rl_denoise_params_default writes {5, 0.6, 0.3, 0.1, 0.2} and zero `reserved`.  params == NULL means those.
 *   Inputs.  `image` and `dst` are required.  albedo, normal and aux -- gather units that accumulated the three films of
 *   rl_scene_render_features -- may each be NULL: a NULL aux acts as (1, 0, 0) in every pixel, a NULL albedo or normal as zeros.
 *   The arithmetic.  All f32, in exactly this order, never contracted; rl_sqrtf and rl_expf are csrc/rl_math.h's, division is the
 *   correctly rounded one.  A, N, X: the tristimulus buffers of albedo, normal, aux.
 *     Guide record of pixel p, once per call:
 *       wgt = X.x;  live = wgt > 0;  z = live ? X.y / wgt : 0;  a = live ? (A.x / wgt, A.y / wgt, A.z / wgt) : 0;
 *       l2 = (N.x*N.x + N.y*N.y) + N.z*N.z;  len = rl_sqrtf(l2);  n = len > 0 ? (N.x / len, N.y / len, N.z / len) : 0.
 *     Constants, on the host: k(sigma) = sigma == 0 ? 0.0f : 1.0f / (sigma * sigma), giving kc, kn, kz, ka for colour, normal,
 *       depth, albedo.  Taps h = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *     Pass i = 0 .. iterations - 1: step s = 1 << i; kc_i = kc * (float)(1u << 2*i) (the colour sigma halves per pass; exact);
 *       input C_i, C_0 being the image's tristimulus buffer.  Per pixel p: if p is not live, C_{i+1}[p] = C_i[p].  Otherwise
 *       sum_w = 0, sum_c = (0, 0, 0); for dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = p + s * (dx, dy); q outside the image or
 *       not live is skipped; else
 *         m = fabsf(C_i[p].y) + fabsf(C_i[q].y);  r = m > 0 ? (C_i[p].y - C_i[q].y) / m : 0;  e_c = r*r;
 *         d = n_p - n_q;  e_n = (d.x*d.x + d.y*d.y) + d.z*d.z;
 *         mz = z_p > z_q ? z_p : z_q;  rz = mz > 0 ? (z_p - z_q) / mz : 0;  e_z = rz*rz;
 *         da = a_p - a_q;  e_a = (da.x*da.x + da.y*da.y) + da.z*da.z;
 *         x = ((e_c*kc_i + e_n*kn) + e_z*kz) + e_a*ka;  wt = (h[dy+2] * h[dx+2]) * rl_expf(-x);
 *         sum_w += wt;  sum_c.k += wt * C_i[q].k for k = x, y, z;
 *       then C_{i+1}[p] = sum_c / sum_w per component.  The centre tap has x = 0 and wt = 9/64, so sum_w > 0 for finite input.
 *     No special cases for non-finite values: whatever the arithmetic above yields is the answer.
 *   Result.  dst's tristimulus buffer holds C_iterations and its compensation buffer is all +0, so rl_tonemap_unit_tonemap,
 *   rl_gather_unit_save, _download and a later _accumulate work on it unchanged.  The inputs are left as they were.
 *   Determinism.  The result is exact: the same bits on every run, and the bits of the CPU restatement tests/_denoise_oracle.py.
 *   Arguments, checked in this order, each failure RL_E_INVALID with a message before any device work: a NULL unit, image or dst;
 *   iterations > RL_DENOISE_MAX_ITERATIONS; a sigma that is negative, NaN, or non-zero and outside [1e-3, 1e3]; non-zero
 *   `reserved`; two given gather units (dst included) that are the same handle.  Every given gather unit must be width x height and
 *   on the unit's device, else RL_E_STATE and nothing is written.
 *   Ordering.  The call waits on the device, through events, for everything queued on the streams of the gather units it reads,
 *   runs on dst's stream and returns when dst is complete, with a host synchronisation: it is a once-per-image operation.  One
 *   user per denoise unit at a time. */
int rl_denoise_params_default(RlDenoiseParams* out);
int rl_denoise_unit_create(int device, uint32_t width, uint32_t height, RlDenoiseUnit** out);
int rl_denoise_unit_destroy(RlDenoiseUnit* unit);
int rl_denoise_unit_denoise(RlDenoiseUnit* unit, RlGatherUnit* image, RlGatherUnit* albedo, RlGatherUnit* normal, RlGatherUnit* aux,
                            const RlDenoiseParams* params, RlGatherUnit* dst);

/* ---- variance-guided denoising: the same filter with the error unit's variance as its colour term ---- */

/* rl_denoise_unit_denoise_variance: the a-trous filter above with the relative colour term replaced by the squared luminance
 * difference over the sum of the two pixels' variances, the variance being the error unit's (rl_error_unit_*) and filtered along
 * with the image.  The plain filter does not know how noisy a pixel is and blurs a converged image as hard as a noisy one; this
 * one backs off as the image converges, which is what an image rendered to a target error (rl_app_run_to_error) needs.
 *   rl_denoise_variance_params_default writes {5, 3.0, 0.3, 0.1, 0.2} and zero `reserved`.  params == NULL means those.  The struct
 *   is RlDenoiseParams; here sigma_colour is in standard deviations of the luminance difference.
 *   Inputs.  As rl_denoise_unit_denoise, and `error`: an error unit with at least two observations.  `image` must be in the units
 *   of the error unit's S, which holds when the error unit observed every plot buffer the image gathered.  THE CALL DOES NOT CHECK
 *   THIS: an image in other units is filtered with a variance that does not belong to it.
 *   The unit's scratch grows by two width x height float planes at its first variance call; a unit that never makes one owns what
 *   rl_denoise_unit_denoise states.
 *   The arithmetic.  All f32 unless stated, in exactly this order, never contracted; division is correctly rounded; rl_expf is
 *   csrc/rl_math.h's.  The guide record, the constants kn, kz, ka, the taps h, the step s = 1 << i, the tap order (dy outer, dx
 *   inner) and the liveness rules are those of rl_denoise_unit_denoise.
 *     V_0 of pixel p, once per call, from the error unit's S, Q (f64), N, k:
 *       d = Q - (S * S) / (double)N;  d = d < 0 ? 0 : d (a NaN stays a NaN);  v = d * ((double)N / (double)(k - 1));  V_0 = (float)v.
 *       This is rl_error_unit_estimate's v: rl_sqrtf(V_0) has the bits of that call's `se`.
 *     Pass i = 0 .. iterations - 1: kv = k(sigma_colour), the same for every pass (the filtered variance shrinks instead of the
 *       sigma).  For a live p: sum_w = 0, sum_c = (0, 0, 0), sum_v = 0; for each tap q inside the image and live
 *         dl = C_i[p].y - C_i[q].y;  m = V_i[p] + V_i[q];  e_c = m > 0 ? (dl * dl) / m : 0
 *           (a pair without variance information has the term off; a NaN m too);
 *         e_n, e_z, e_a as in the plain filter;
 *         x = ((e_c*kv + e_n*kn) + e_z*kz) + e_a*ka;  wt = (h[dy+2] * h[dx+2]) * rl_expf(-x);
 *         sum_w += wt;  sum_c.k += wt * C_i[q].k;  sum_v += (wt * wt) * V_i[q];
 *       then C_{i+1}[p] = sum_c / sum_w per component and V_{i+1}[p] = sum_v / (sum_w * sum_w).
 *       For a p that is not live: C_{i+1}[p] = C_i[p] and V_{i+1}[p] = V_i[p].
 *     No special cases for non-finite values.
 *   Result.  dst holds C_iterations with a +0 compensation buffer, as after the plain call.  variance_out (host, width x height
 *   floats, may be NULL) receives V_iterations: under the model of independent pixels, the variance of the denoised luminance.  The
 *   inputs, the error unit included, are left as they were.
 *   Determinism.  The result is exact: the same bits on every run, and the bits of tests/_denoise_variance_oracle.py.
 *   Arguments, checked in this order before any device work: a NULL unit, image, dst or error (RL_E_INVALID); the plain call's
 *   checks of params and its rule that the given gather units are distinct, in its order (RL_E_INVALID); an error unit with fewer
 *   than two observations (RL_E_STATE); any given unit, the error unit included, of another size or device (RL_E_STATE).  In the
 *   refused cases nothing is written.
 *   Ordering.  As the plain call; the call also waits, through an event, for what is queued on the error unit's stream.  The copy
 *   to variance_out happens after the last pass and before the return. */
int rl_denoise_variance_params_default(RlDenoiseParams* out);
int rl_denoise_unit_denoise_variance(RlDenoiseUnit* unit, RlGatherUnit* image, RlGatherUnit* albedo, RlGatherUnit* normal, RlGatherUnit* aux,
                                     RlErrorUnit* error, const RlDenoiseParams* params, RlGatherUnit* dst,
                                     float* variance_out /* host, width x height, may be NULL */);

/* ---- spectral film: photons kept by wavelength, projected under any observer (rl_spectral_unit_*) ---- */

#define RL_SPECTRAL_MAX_NODES 401

/* A spectral unit is a film of `n_nodes` planes of width x height floats.  Every other film of the library multiplies a photon by
 * rl_tristimulus(wavelength) inside the splat and keeps three floats per pixel; this one splats the photon's intensity by wavelength
 * and leaves the observer to a projection, rl_spectral_unit_project, under a caller-supplied n_nodes x 3 matrix: CIE 1931
 * (rl_spectral_observer_cie1931), a camera's measured sensitivities, a single band, another white point -- without a re-trace.  The
 * projection writes a gather unit, so rl_tonemap_unit_tonemap, rl_gather_unit_save, _download and rl_denoise_unit_denoise work on
 * the result unchanged.  The chain is: rl_trace_unit_render (un-fused); rl_spectral_unit_plot; rl_spectral_unit_project; tonemap.
 *   The node model is the CIE table's own (81 nodes at 380 + 5 i nm, interpolated linearly, a linear fall-off beyond each end):
 *   at n_nodes = 81, projecting with the CIE table reproduces the XYZ film of the same photons up to rounding.
 *   The arithmetic.  All f32, in exactly this order, never contracted; division is the correctly rounded one.
 *     Constants, on the host: spacing = 400.0f / (float)(n_nodes - 1); node b sits at 380.0f + (float)b * spacing.
 *     Splat of one photon {x, y, probability, wavelength}.  Skipped if probability == 0; skipped if x or y is NaN or infinite
 *       (rl_plot_unit_plot_photons' rule); skipped if wavelength is NaN or infinite -- a DIFFERENCE from the XYZ film, which has no
 *       such rule and plots what rl_tristimulus makes of that wavelength.  Otherwise
 *         f = (wavelength - 380.0f) / spacing;  fl = floorf(f);  r = f - fl;
 *         lo = probability * (1.0f - r)  -> node (int)fl;      hi = probability * r  -> node (int)fl + 1.
 *       Whether a node is in the film is decided by comparing fl as a float (0 <= fl <= n_nodes - 1 for lo, -1 <= fl <= n_nodes - 2
 *       for hi) before any conversion to int, so no conversion of an out-of-range float is relied on.  A node outside
 *       0 .. n_nodes - 1 is dropped: the table's linear fall-off at 375-380 and 780-785 nm, and zero beyond.  Each kept value is
 *       multiplied by each of the four weights of the plot unit's splat (rl_splat_weights(width, height, aspect, x, y), aspect =
 *       (float)width / (float)height; the four pixels are clamped into the film) and each product is added with an f32 atomic to
 *       film[node * width * height + pixel], onto what is there: at most eight atomics per photon.  A negative probability
 *       subtracts; an infinite one is plotted as the arithmetic gives.
 *     Project, per pixel p and component k of 3: acc = 0.0f; for b = 0 .. n_nodes - 1 in order
 *       acc = acc + matrix[b * 3 + k] * film[b * n_pixels + p]; dst's tristimulus buffer gets acc.  No special cases for non-finite
 *       values.  dst's compensation buffer is all +0, as after rl_denoise_unit_denoise.  The film is left as it was.
 *   rl_spectral_unit_create.  Checked in this order before any device work, each failure RL_E_INVALID with a message: a NULL
 *   `out`; a zero width or height; n_nodes < 2 or > RL_SPECTRAL_MAX_NODES; width * height * n_nodes > RL_MAX_PIXELS (computed in
 *   64 bits).  The film is zeroed.  rl_spectral_unit_clear zeroes it again (queued on the unit; everything below is ordered after it).
 *   rl_spectral_unit_plot takes the photons of each given trace unit's last un-fused render, as rl_plot_unit_plot does; it is
 *   ordered after those renders on the device (a render that was begun is ended) and returns when the splats are in the film.  It
 *   is synchronous on purpose: it takes no part in what makes a trace unit's next render wait for a plot unit, so the same trace
 *   units may be plotted into a plot unit and a spectral unit, in either order.  A NULL unit, or NULL trace_units with
 *   n_trace_units > 0, is RL_E_INVALID; a NULL trace unit or one on another device is RL_E_STATE, as for rl_plot_unit_plot.
 *   rl_spectral_unit_plot_photons / _device.  Every rule of rl_plot_unit_plot_photons / _device holds: any n is accepted, the host
 *   form stages in chunks of 2^20 records, the _device form refuses pageable host memory (RL_E_INVALID), n = 0 does nothing, a
 *   NULL unit, or NULL photons with n > 0, is RL_E_INVALID before any device work; the splats are in the film on return.
 *   rl_spectral_unit_download / _upload move the whole film, n_nodes * width * height floats, planes in node order (node-major:
 *   part of the ABI), each plane rows of `width`.
 *   rl_spectral_unit_project.  Checked in this order: a NULL unit, matrix or dst is RL_E_INVALID; a dst of another size or device
 *   is RL_E_STATE, and nothing is written.  `matrix` is host memory, n_nodes x 3 floats, row b = what one unit of node b adds to the
 *   three components; it is read as given, non-finite entries included.  Ordering is the denoiser's: the call waits on the device
 *   for everything queued on dst's stream and on the film, runs on dst's stream and returns when dst is complete.
 *   rl_spectral_observer_cie1931(n_nodes, out) writes n_nodes x 3 floats, row b = rl_tristimulus of node b's wavelength from the
 *   library's table: at 81 nodes the table's rows exactly.  Host arithmetic only: callable without a GPU.  A NULL `out` or an
 *   n_nodes outside 2 .. RL_SPECTRAL_MAX_NODES is RL_E_INVALID.
 *   Determinism.  The film differs between runs only by the order of its atomics; a (node, pixel) that received at most two
 *   non-zero terms holds the same bits on every run.  The projection is exact given the film: the same bits on every run, and the
 *   bits of the CPU restatement tests/_spectral_oracle.py.
 *   One user per spectral unit at a time. */
int rl_spectral_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, RlSpectralUnit** out);
int rl_spectral_unit_destroy(RlSpectralUnit* unit);
int rl_spectral_unit_clear(RlSpectralUnit* unit);
int rl_spectral_unit_plot(RlSpectralUnit* unit, RlTraceUnit* const* trace_units, uint32_t n_trace_units);
int rl_spectral_unit_plot_photons(RlSpectralUnit* unit, const RlMappedPhoton* photons, uint64_t n);
int rl_spectral_unit_plot_photons_device(RlSpectralUnit* unit, const RlMappedPhoton* device_photons, uint64_t n);
int rl_spectral_unit_download(RlSpectralUnit* unit, float* out);
int rl_spectral_unit_upload(RlSpectralUnit* unit, const float* in);
int rl_spectral_unit_project(RlSpectralUnit* unit, const float* matrix, RlGatherUnit* dst);
int rl_spectral_observer_cie1931(uint32_t n_nodes, float* out);

/* ---- spectral glare: a wavelength-scaled point-spread convolution of the spectral film (rl_glare_unit_*) ---- */

#define RL_GLARE_MAX_TAPS 65

/* A glare unit holds one K x K gather table per spectral node (K = `taps`, odd, 1 .. RL_GLARE_MAX_TAPS; R = (K - 1) / 2) and
 * applies them to a spectral unit's film: bloom, veiling glare, the diffraction pattern of an aperture -- point-spread functions
 * whose size grows linearly with wavelength, which is what gives a glare halo its coloured fringe (red outside, blue inside) and
 * what a blur of an XYZ image cannot reproduce.  rl_glare_unit_apply convolves every plane with its node's table, projects the
 * result under a caller-supplied n_nodes x 3 matrix (as rl_spectral_unit_project takes it) in the same launch and writes a gather
 * unit, so rl_tonemap_unit_tonemap, rl_gather_unit_save, _download and the denoisers work on the result unchanged.  The convolved
 * cube never exists in memory.  The chain is: rl_spectral_unit_plot; rl_glare_unit_set_kernels; rl_glare_unit_apply; tonemap.
 *   The cap of 65 taps is part of the ABI: at that size a 64 x 16 output tile with its halo is 40 KB of on-chip memory, so more
 *   than one workgroup still fits on a compute unit.  Wider point-spread functions want another method and another contract.
 *   The arithmetic of apply.  All f32, in exactly this order, a separate multiply and add, never contracted.  For pixel (x, y) and
 *   component c of 3:
 *       acc_c = 0.0f
 *       for b = 0 .. n_nodes - 1:
 *           g = 0.0f
 *           for j = 0 .. K - 1:
 *               r = 0.0f
 *               for i = 0 .. K - 1:
 *                   (qx, qy) = (x + i - R, y + j - R)
 *                   if (qx, qy) is inside the film:  r = r + tables[b][j][i] * film[b][qy][qx]
 *               g = g + r
 *           acc_c = acc_c + matrix[b * 3 + c] * g
 *       dst.tristimulus[(y * width + x) * 3 + c] = acc_c
 *     A tap outside the film adds nothing -- no clamp, no mirror: light from outside the frame is unknown.  No special cases for
 *     non-finite values.  dst's compensation buffer is all +0, as after rl_spectral_unit_project.  The film and the tables are left
 *     as they were.  The two-level sum (row sums, then the sum of rows) keeps the rounding error at O(K) ulps instead of O(K^2).
 *     With K = 1 and every table entry 1.0f, apply writes the bits of rl_spectral_unit_project for any finite film.
 *   rl_glare_unit_create.  Checked in this order before any device work, each failure RL_E_INVALID with a message: a NULL `out`;
 *   a zero width or height; n_nodes outside 2 .. RL_SPECTRAL_MAX_NODES; taps even, zero or above RL_GLARE_MAX_TAPS;
 *   width * height * n_nodes > RL_MAX_PIXELS (computed in 64 bits).  A unit starts without tables.
 *   rl_glare_unit_set_kernels.  `tables` is host memory, n_nodes * taps * taps floats: table b, row j, entry i at
 *   (b * taps + j) * taps + i; entry (j, i) weighs the film at (x + i - R, y + j - R), a gather.  A NULL unit or NULL tables is
 *   RL_E_INVALID.  The tables are read as given, non-finite entries included, copied to the device and queued on the unit; they may
 *   be set again.
 *   rl_glare_unit_apply.  Checked in this order: a NULL unit, film, matrix or dst is RL_E_INVALID; a unit without tables is
 *   RL_E_STATE; a film of another width, height, n_nodes or device is RL_E_STATE; a dst of another size or device is RL_E_STATE.
 *   Nothing is written on failure.  `matrix` is host memory, n_nodes x 3 floats, read as given.  Ordering is the projection's: the
 *   call waits on the device for everything queued on dst's stream, on the film and on the unit's tables, runs on dst's stream
 *   and returns when dst is complete.
 *   rl_glare_psf_veil(taps, r0, out) writes a taps x taps table, a veiling-glare point-spread function: entry (j, i) with
 *   d2 = (i - R)^2 + (j - R)^2 is 1 / (q * sqrt(q)), q = 1 + d2 / (r0 * r0), computed in f64 in that order and rounded to f32.  The
 *   table is not normalised.  Checked in this order: a NULL `out`; taps not odd in 1 .. RL_GLARE_MAX_TAPS; an r0 that is not finite
 *   and greater than 0 (RL_E_INVALID).
 *   rl_glare_kernels_scaled(psf, psf_taps, lambda0, n_nodes, strength, taps, out) turns one base point-spread function -- psf_taps
 *   x psf_taps floats, row-major, centre at R_in = (psf_taps - 1) / 2, sampled at pixel pitch for wavelength lambda0 (nm) -- into
 *   the n_nodes gather tables of set_kernels.  All f64 with add, subtract, multiply, divide and floor only, in this order; node b:
 *   lambda = 380 + b * (400 / (n_nodes - 1)); s = lambda / lambda0; for entry (j, i): u = -(i - R) / s + R_in, v = -(j - R) / s +
 *   R_in (the point flip makes a gather table out of a scatter function: an impulse at q produces the function centred on q,
 *   unflipped); iu = floor(u), fu = u - iu, likewise for v; w = ((1 - fu) * p00 + fu * p10) * (1 - fv) + ((1 - fu) * p01 + fu * p11)
 *   * fv, where pab = psf[iv + b][iu + a] and 0 outside the base table.  S = the sum of w over the table in row-major order with
 *   one accumulator; t = strength * (w / S), the centre entry gets + (1 - strength); out = (float)t.  So every node's table sums to 1
 *   up to rounding: glare moves energy, it adds none.  For s > 1 the scaled function is cut at the table's edge BEFORE it is
 *   normalised: what a wider table would have spread further stays inside.  RL_E_INVALID before anything is written: a NULL psf
 *   or out; psf_taps not odd in 1 .. 257; a lambda0 that is not finite and greater than 0; n_nodes outside 2 ..
 *   RL_SPECTRAL_MAX_NODES; a strength outside [0, 1]; taps not odd in 1 .. RL_GLARE_MAX_TAPS; a psf entry that is not finite and
 *   >= 0; a node whose S is not > 0 (the function gives it nothing).
 *   Both helpers are host arithmetic only: callable without a GPU.
 *   Determinism.  apply is exact given the film, the tables and the matrix: the same bits on every run, and the bits of the CPU
 *   restatement tests/_glare_oracle.py; so are the two helpers.
 *   One user per glare unit at a time. */
int rl_glare_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, uint32_t taps, RlGlareUnit** out);
int rl_glare_unit_destroy(RlGlareUnit* unit);
int rl_glare_unit_set_kernels(RlGlareUnit* unit, const float* tables);
int rl_glare_unit_apply(RlGlareUnit* unit, RlSpectralUnit* film, const float* matrix, RlGatherUnit* dst);
int rl_glare_psf_veil(uint32_t taps, double r0, float* out);
int rl_glare_kernels_scaled(const float* psf, uint32_t psf_taps, double lambda0, uint32_t n_nodes, double strength, uint32_t taps,
                            float* out);

/* ---- relight film: photons kept by wavelength and by light, re-mixed without a re-trace (rl_relight_unit_*) ---- */

#define RL_RELIGHT_MAX_GROUPS 16
#define RL_RELIGHT_DROP 0xff

/* A relight unit is a film of n_groups * n_nodes planes of width x height floats: n_groups spectral cubes, one per group of
 * lights.  Plane q = g * n_nodes + b holds node b of group g (group-major, then node-major: part of the ABI of download and
 * upload).  The node model is the spectral film's: spacing = 400.0f / (float)(n_nodes - 1), node b at 380.0f + (float)b * spacing.
 *   Why it is exact.  render_ray multiplies the emission in as the last factor of a path's value (trace_unit.rs:99-101): geometry,
 *   bounces and roulette never see it, and RlPathResult::object names the emitter.  So another temperature or intensity of a black
 *   body changes the value of a finished path that ended on it by get_intensity'(wavelength) / get_intensity(wavelength)
 *   (material.rs:92-104) and nothing else.  Keep the photons by emitter, and a light is dimmed, warmed or shown alone by a gain per
 *   (group, node) applied in the mix: rl_relight_gains_black_body gives that ratio at the nodes.  What is not exact is the node
 *   model: the gain is interpolated linearly between nodes, as the observer is.
 *   rl_relight_unit_create.  Checked in this order before any device work, each failure RL_E_INVALID with a message: a NULL `out`;
 *   a zero width or height; n_nodes outside 2 .. RL_SPECTRAL_MAX_NODES; n_groups outside 1 .. RL_RELIGHT_MAX_GROUPS;
 *   width * height * n_nodes * n_groups > RL_MAX_PIXELS (computed in 64 bits).  The film is zeroed.  rl_relight_unit_clear zeroes
 *   it again (queued on the unit; everything below is ordered after it).
 *   rl_relight_unit_set_groups.  groups[o] is the group of object o of the scene's description, n_objects entries: each below
 *   n_groups, or RL_RELIGHT_DROP (paths that end on that object are left out).  Any other entry is RL_E_INVALID and the unit keeps
 *   the table it had; so is a NULL unit or table and n_objects == 0.  A unit starts without a table, and the calls that need one
 *   return RL_E_STATE until it has one.  The call returns when the table is on the device.
 *   The routed splat (rl_relight_unit_plot_results / _device) of sample i with result r = results[i].  All f32, in this order, never
 *   contracted.  Skipped if r.value == 0; if samples[i].x or .y is NaN or infinite; if samples[i].ray.wavelength is NaN or
 *   infinite; if r.object >= n_objects (RL_OBJECT_NONE is such a value); if groups[r.object] == RL_RELIGHT_DROP.  Otherwise it is
 *   rl_spectral_unit_plot_photons' splat of the photon {x, y, r.value, wavelength} -- the same f, fl, r, lo, hi, the same decisions
 *   on fl as a float, the same four weights, at most eight f32 atomics -- into the cube of group g = groups[r.object]: plane
 *   g * n_nodes + node.  No content of the buffers makes the kernel touch memory outside the film.  r.end and r.segments are not read.
 *   Checked in this order before any device work: a NULL unit, or NULL samples or results with n > 0 (RL_E_INVALID); a unit without
 *   a table (RL_E_STATE).  n = 0 then does nothing and launches nothing.  The host form stages in chunks of 2^20 records, the
 *   _device form takes device pointers on the unit's device and refuses pageable host memory (RL_E_INVALID), as
 *   rl_scene_render_rays_device does.  The splats are in the film on return.
 *   rl_relight_unit_render.  Paths first_path_index .. first_path_index + n_paths - 1 of RNG stream `stream` under `seed`, in chunks
 *   of at most 2^20 in scratch the unit owns (taken at the first such call): rl_scene_camera_rays_device's samples of those indices
 *   for the unit's width x height; their rays traced by the path kernel as rl_scene_render_rays_device traces them (the same
 *   launch, the same results bit for bit); the routed splat.  Checked in this order: a NULL unit, a NULL scene, an unknown fetch
 *   mode, max_segments > RL_PATH_MAX_SEGMENTS_CAP (RL_E_INVALID); a unit without a table (RL_E_STATE); path indices that reach
 *   2^64 - 1 (RL_E_INVALID); a table whose n_objects is not the scene's object count, or unit and scene on different devices
 *   (RL_E_STATE).  n_paths = 0 then does nothing.  The call orders against open launches as rl_scene_render_rays does and returns
 *   when the splats are in the film.
 *   rl_relight_unit_download / _upload move the whole film, n_groups * n_nodes * width * height floats, planes in the order above,
 *   each plane rows of `width`.
 *   rl_relight_unit_mix.  gains is host memory, n_groups x n_nodes floats (NULL: all 1); matrix is host memory, n_nodes x 3 floats,
 *   an observer as rl_spectral_unit_project takes it.  The host forms c[3 q + k] = gains[q] * matrix[3 b + k] for q = g * n_nodes + b,
 *   one f32 multiply (gains == NULL: matrix[3 b + k] itself).  Per pixel p and component k the device computes acc = 0.0f; for
 *   q = 0 .. n_groups * n_nodes - 1 in order acc = acc + c[3 q + k] * film[q * n_pixels + p], multiply and add separate, no special
 *   case for non-finite values.  dst's tristimulus buffer gets acc and its compensation buffer is all +0; the film is left as it
 *   was.  This is rl_spectral_unit_project's arithmetic on the composed matrix.  A NULL unit, matrix or dst is RL_E_INVALID; a dst
 *   of another size or device is RL_E_STATE, and nothing is written.  Ordering is rl_spectral_unit_project's.
 *   rl_relight_gains_black_body(n_nodes, kelvins_from, intensity_from, kelvins_to, intensity_to, out) writes n_nodes floats:
 *   out[b] = I_to(l_b) / I_from(l_b), l_b node b's wavelength, I(l) = (float)rl_boltzmann((double)l, (double)kelvins) *
 *   rl_black_body_normalisation(kelvins, intensity) -- the library's get_intensity -- and the divide in f32; a node whose I_from is 0
 *   gets gain 0 (that light deposited nothing there).  Host arithmetic only: callable without a GPU.  A NULL `out`, an n_nodes
 *   outside 2 .. RL_SPECTRAL_MAX_NODES, or a kelvins or intensity that is not finite and greater than 0 is RL_E_INVALID.
 *   Determinism.  The film differs between runs only by the order of its atomics, as the spectral film does; the mix is exact given
 *   the film: the same bits on every run, and the bits of the CPU restatement tests/_relight_oracle.py.
 *   One user per relight unit at a time. */
int rl_relight_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_nodes, uint32_t n_groups, RlRelightUnit** out);
int rl_relight_unit_destroy(RlRelightUnit* unit);
int rl_relight_unit_clear(RlRelightUnit* unit);
int rl_relight_unit_set_groups(RlRelightUnit* unit, const uint8_t* groups, uint32_t n_objects);
int rl_relight_unit_plot_results(RlRelightUnit* unit, const RlCameraSample* samples, const RlPathResult* results, uint64_t n);
int rl_relight_unit_plot_results_device(RlRelightUnit* unit, const RlCameraSample* device_samples, const RlPathResult* device_results,
                                        uint64_t n);
int rl_relight_unit_render(RlRelightUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed, uint32_t stream,
                           uint64_t first_path_index, uint64_t n_paths, uint32_t max_segments);
int rl_relight_unit_download(RlRelightUnit* unit, float* out);
int rl_relight_unit_upload(RlRelightUnit* unit, const float* in);
int rl_relight_unit_mix(RlRelightUnit* unit, const float* gains, const float* matrix, RlGatherUnit* dst);
int rl_relight_gains_black_body(uint32_t n_nodes, float kelvins_from, float intensity_from, float kelvins_to, float intensity_to,
                                float* out);

/* ---- noise estimate: the standard error of the accumulated luminance (rl_error_unit_*) ---- */

#define RL_ERROR_TILE 16

/* An error unit says how noisy an accumulated image is.  It is shown every plot buffer just before the buffer is gathered
 * (rl_error_unit_observe; the caller gathers afterwards) and keeps, per pixel, two f64 sums over these observations: observation j
 * is a plot buffer that holds the sum of what n_j independent paths splatted; y_j is the Y component of a pixel in it.
 *     S = sum_j y_j,   Q = sum_j y_j^2 / n_j,   N = sum_j n_j,   k = the number of observations.
 * d = Q - S^2 / N is the weighted sum of squared deviations of the batch means, on k - 1 degrees of freedom, and
 * sqrt(d N / (k - 1)) estimates the standard deviation of S itself, in the gather unit's own units; batches of unequal size are
 * handled exactly.  Luminance only.  The sums are f64 because d cancels: f32 sums lose 6e-4 of d at 7,000 paths per pixel per
 * observation and 6e-2 at 116,000.  The unit keeps its own S: a gather unit may hold samples the error unit never saw (a resumed
 * checkpoint, rl_gather_unit_load).
 *   The arithmetic.  f64 and f32 as stated, in exactly this order, never contracted; division and square root correctly rounded.
 *   rl_error_unit_observe(unit, plot, n_paths).  Reads the plot unit's Y plane and leaves the plot buffer exactly as it was.  Per
 *     pixel: yd = (double)y;  S = S + yd;  Q = Q + (yd * yd) / (double)n_paths.  On the host: k += 1; N += n_paths.  No special
 *     cases for a negative or non-finite y.  Checked in this order: a NULL unit or plot, or n_paths == 0, is RL_E_INVALID; N
 *     overflowing 64 bits is RL_E_INVALID; a plot unit of another size or device is RL_E_STATE, and nothing is written.
 *     Ordering is rl_gather_unit_accumulate's: a fused render begun into the plot unit is ended first; the kernel waits through an
 *     event for everything queued on the plot unit's stream and runs on the error unit's own stream; the plot unit's stream then
 *     waits for the kernel, so a later clear or gather cannot overtake the read.  The call does not synchronise the host.
 *   rl_error_unit_estimate(unit, stats, se, tiles).  Needs k >= 2, else RL_E_STATE (after: a NULL unit or stats is RL_E_INVALID).
 *     Per pixel: d = Q - (S * S) / (double)N;  d = d < 0 ? 0 : d (a NaN stays a NaN);  v = d * ((double)N / (double)(k - 1));
 *       se = rl_sqrtf((float)v);  ay = fabs(S).
 *     Per RL_ERROR_TILE x RL_ERROR_TILE tile (each tile starts at a multiple of 16): the 256 values of (double)se in tile raster
 *       order, +0.0 for positions outside the image; for stride = 128, 64, ..., 1: v[i] = v[i] + v[i + stride] for i < stride; v[0]
 *       is the tile's t_se.  The same tree over ay gives t_y.  The bits of that tree are the contract.
 *     On the host, from the tile pairs, sequentially in f64 in tile raster order: sum_se = sum t_se, sum_y = sum t_y (each from
 *       +0.0), relative_error = sum_se / sum_y as the arithmetic gives (a black image: NaN); m = sum_y / (double)n_tiles;
 *       rel = t_se / (t_y > m ? t_y : m); worst_tile_error starts as tile 0's rel and is replaced where a later rel > it (so
 *       worst_tile_x, _y name the first tile that holds it).  A tile at least as bright as the average reports its own relative
 *       error; a darker one is measured against the average brightness, which is what its noise costs after tonemapping.
 *     `se` may be NULL; otherwise width x height floats of host memory, in rows.  `tiles` may be NULL; otherwise
 *     tiles_y * tiles_x * 2 doubles of host memory, {t_se, t_y} per tile, tiles in raster order.  The call waits for the
 *     observations queued on the unit and returns with a host synchronisation: a once-per-tonemap operation.  The result is exact:
 *     the same bits on every run, and the bits of the CPU restatement tests/_error_oracle.py.
 *   rl_error_unit_download / _upload move S and Q as planar width x height doubles in rows (the host layout is part of the ABI),
 *     and k and N; any of download's outputs may be NULL; upload needs both planes (a NULL unit or plane is RL_E_INVALID).  They
 *     wait for what is queued on the unit.  State can be kept across runs by hand with them.
 *   rl_error_unit_create refuses a NULL `out`, a zero size and width * height > RL_MAX_PIXELS (RL_E_INVALID, in this order, before
 *     any device work).  The planes start as +0 and k = N = 0; rl_error_unit_clear restores that (queued on the unit).
 *   One user per error unit at a time. */
typedef struct RlErrorStats {
    uint64_t observations, paths;        /* k, N */
    uint32_t tiles_x, tiles_y;           /* ceil(width / 16), ceil(height / 16) */
    uint32_t worst_tile_x, worst_tile_y;
    double sum_y, sum_se;                /* over the image */
    double relative_error;               /* sum_se / sum_y */
    double worst_tile_error;
} RlErrorStats;

int rl_error_unit_create(int device, uint32_t width, uint32_t height, RlErrorUnit** out);
int rl_error_unit_destroy(RlErrorUnit* unit);
int rl_error_unit_clear(RlErrorUnit* unit);
int rl_error_unit_observe(RlErrorUnit* unit, RlPlotUnit* plot, uint64_t n_paths);
int rl_error_unit_estimate(RlErrorUnit* unit, RlErrorStats* stats, float* se, double* tiles);
int rl_error_unit_download(RlErrorUnit* unit, double* sum_y, double* sum_q, uint64_t* observations, uint64_t* paths);
int rl_error_unit_upload(RlErrorUnit* unit, const double* sum_y, const double* sum_q, uint64_t observations, uint64_t paths);

/* ---- robust film: M sub-films combined by a Gini-trimmed median of means (rl_robust_unit_*) ---- */

#define RL_ROBUST_MAX_BUCKETS 32
#define RL_ROBUST_NEXT 0xffffffffu

/* A robust unit removes outliers -- fireflies: rare paths whose contribution is hundreds of times a pixel's mean -- from an
 * accumulated image.  It keeps M = n_buckets independent sub-films ("buckets") instead of one: it is shown every plot buffer just
 * before the buffer is gathered (rl_robust_unit_observe, the error unit's protocol; the caller gathers afterwards) and adds it to
 * one bucket.  rl_robust_unit_resolve combines the buckets per pixel by a median of means whose trim follows the inequality of the
 * M bucket means, measured by their Gini coefficient (Buisine et al. 2021, "Firefly removal in Monte Carlo rendering with adaptive
 * Median of meaNs"): equal buckets are averaged, one bucket far above the others is dropped together with the lowest one.  The
 * result goes to a gather unit, as the denoiser's and the spectral projection's do.
 *   State.  On the device M x 3 planes of width x height doubles in rows, all +0 at first: plane j * 3 + c holds component c (X, Y,
 *     Z) of bucket j's sum S[j][c].  sums[(j * 3 + c) * n_pixels + p] is the host layout of download and upload and part of the
 *     ABI.  On the host n[j], the paths of bucket j (u64), and k, the number of observations.  24 M bytes per pixel.
 *   The arithmetic.  f64 as stated, in exactly this order, never contracted; the division correctly rounded.
 *   rl_robust_unit_observe(unit, plot, n_paths, bucket).  j = bucket, or k mod M for RL_ROBUST_NEXT.  Per pixel and component:
 *     S[j][c] = S[j][c] + (double)p[c]; the plot buffer is only read and left exactly as it was.  On the host: n[j] += n_paths;
 *     k += 1.  No special cases for negative or non-finite values.  Checked in this order: a NULL unit or plot, or n_paths == 0, is
 *     RL_E_INVALID; bucket >= M and != RL_ROBUST_NEXT is RL_E_INVALID; n[j] or the total N overflowing 64 bits is RL_E_INVALID; a
 *     plot unit of another size or device is RL_E_STATE, and nothing is written.  Ordering is rl_error_unit_observe's: a fused
 *     render begun into the plot unit is ended first; the kernel waits through an event for everything queued on the plot unit's
 *     stream and runs on the robust unit's own stream; the plot unit's stream then waits for the kernel, so a later clear or gather
 *     cannot overtake the read.  The call does not synchronise the host.  The caller owes independence: each observation is a plot
 *     buffer of paths that no other bucket's observations contain.
 *   rl_robust_unit_resolve(unit, params, dst, stats, trim).  Checked in this order: a NULL unit, params or dst is RL_E_INVALID;
 *     params->gain NaN or negative is RL_E_INVALID (+infinity is legal); any n[j] == 0 is RL_E_STATE (every bucket needs an
 *     observation); a dst of another size or device is RL_E_STATE, and nothing is written.  With N = sum_j n[j], per pixel:
 *       1. m[j][c] = S[j][c] / (double)n[j].
 *       2. The key of bucket j is m[j][1], its Y.
 *       3. The buckets are ranked by (key, j) ascending: rank(j) = the number of i with key[i] < key[j], or key[i] == key[j] and
 *          i < j.  (r) is the bucket of rank r.
 *       4. If any key is not finite or is < 0 the pixel is untrimmable: c = 0, it counts in untrimmable_pixels, the ranks are not
 *          used and the sums of 6 run in bucket order j = 0 .. M - 1.
 *       5. Otherwise T = sum_r key(r) and W = sum_r (double)(2 r - M + 1) * key(r), each summed sequentially from +0.0 for
 *          r = 0 .. M - 1 (the integer arithmetic first, then the conversion).  If !(T > 0): c = 0, counted in untrimmable_pixels
 *          too.  Else G = W / ((double)M * T) -- the Gini coefficient of the keys --, v = ((gain * G) * (double)M) * 0.5 and
 *          cmax = min(max_trim, (M - 1) / 2) in integer division; c = 0 if !(v >= 0), c = cmax if v >= (double)cmax, otherwise
 *          c = (uint32_t)floor(v).
 *       6. Per component, A = sum of m(r)[c] for r = c .. M - c - 1, sequentially from +0.0 in rank order.  The ranks of Y order
 *          all three components: a pixel keeps whole buckets, so its colour stays that of real samples.
 *       7. dst's tristimulus gets (float)((A / (double)(M - 2 c)) * (double)N); dst's compensation gets +0, as after
 *          rl_spectral_unit_project.  dst's previous contents are replaced.
 *     So gain = 0, max_trim = 0 or M equal means give the plain pooled mean of the bucket means times N -- for equal n[j] the sum a
 *     gather unit would hold, up to rounding --, and gain = +infinity with any inequality gives the median bucket for odd M and the
 *     two middle buckets for even M.  Where c > 0 the film is no longer unbiased: a skewed pixel distribution is pulled towards
 *     its median.
 *     `trim` may be NULL; otherwise width x height bytes of host memory, c per pixel in rows.  `stats` may be NULL; its counts are
 *     exact (a host reduction of the trim bytes): the same on every run.  Ordering is rl_spectral_unit_project's: the call waits on
 *     the device for what is queued on dst's stream and on the unit, runs on dst's stream and returns with dst complete.
 *     Everything it produces is exact: the same bits on every run, and the bits of the CPU restatement tests/_robust_oracle.py.
 *   rl_robust_unit_estimate(unit, params, stats, se, tiles, trim).  How noisy the film is that rl_robust_unit_resolve writes with
 *     the same params: the standard error of its Y, per pixel and per tile, in rl_error_unit_estimate's output format, so that the
 *     tile map, a target-error stopping rule and rl_adaptive_unit_plan take it as they take that call's.  The M buckets are M
 *     estimates of the pixel; the standard error of their trimmed mean is the winsorized sum of squares over K (K - 1), K the
 *     number of kept buckets (Tukey and McLaughlin 1963), so a firefly that the resolve trims stops inflating the estimate.
 *     Luminance only, from the Y planes alone.  Checked in this order: a NULL unit, params or stats is RL_E_INVALID; params->gain
 *     NaN or negative is RL_E_INVALID (+infinity is legal); any n[j] == 0 is RL_E_STATE; nothing is written and nothing launched.
 *     All arithmetic is f64 in exactly this order, never contracted, the division correctly rounded; one f64 -> f32 conversion and
 *     one rl_sqrtf.  With N = sum_j n[j] and k observations, per pixel:
 *       1. key[j] = S[j][1] / (double)n[j].  The ranks, the untrimmable rule, T, W, G and v are the resolve's steps 2 to 5, word for
 *          word, but for the cap: cmax = min(max_trim, (M - 2) / 2) in integer division, so that at least two buckets are kept --
 *          for odd M at full trim one less than the resolve's cap; M = 3 never trims.
 *       2. With c the trim and K = M - 2 c: lo = key(c), hi = key(M - c - 1), and A = sum of key(r) for r = c .. M - c - 1,
 *          sequentially from +0.0 in rank order.  An untrimmable pixel has c = 0 and bucket order, as in the resolve.
 *       3. B = (double)c * lo + A;  B = B + (double)c * hi;  mw = B / (double)M: the winsorized mean.
 *       4. D from +0.0: for r = c .. M - c - 1 in order e = key(r) - mw; D = D + e * e.  Then el = lo - mw;
 *          D = D + (double)c * (el * el);  eh = hi - mw;  D = D + (double)c * (eh * eh).
 *       5. var = D / (double)(K * (K - 1)), the integer product first.
 *       6. f = (A / (double)K) * (double)N -- the Y the resolve writes, before its conversion, wherever its c is this c --;
 *          v = (var * (double)N) * (double)N;  se = rl_sqrtf((float)v);  ay = fabs(f).  No special cases: a NaN stays a NaN, an
 *          overflow becomes +infinity.
 *       7. The RL_ERROR_TILE tiles are rl_error_unit_estimate's tree over (double)se and over ay, bit for bit (strides 128 .. 1,
 *          +0.0 outside the image), and the host part is that call's: sum_se, sum_y, relative_error, the worst tile.
 *          stats->observations = k and stats->paths = N.
 *       8. trim[p] = c, with bit 7 set for an untrimmable pixel.
 *     The estimate treats the bucket means as equally weighted draws, as the resolve does: with unequal n[j] it is an
 *     approximation.  For gain 0, equal n[j] and one observation per bucket, v equals rl_error_unit_estimate's d N / (k - 1)
 *     algebraically.  The trim is chosen from the same keys whose spread is then measured: the estimate is calibrated for a fixed c
 *     (tests/test_robust_error.py), and by how much a Gini-chosen c biases it is not measured.
 *     `se` may be NULL; otherwise width x height floats of host memory, in rows.  `tiles` may be NULL; otherwise
 *     tiles_y * tiles_x * 2 doubles, {t_se, t_y} per tile in raster order.  `trim` may be NULL; otherwise width x height bytes.
 *     Ordering is rl_error_unit_estimate's: the call runs on the unit's stream behind what is queued on the unit and returns with a
 *     host synchronisation; the unit's state is only read.  The result is exact: the same bits on every run, and the bits of the CPU
 *     restatement tests/_robust_error_oracle.py.
 *   rl_robust_unit_download / _upload move the planes in the host layout above, the M values n[j] and k; any of download's outputs
 *     may be NULL; upload needs `sums` and `bucket_paths` (a NULL unit or either is RL_E_INVALID), takes any contents of the planes,
 *     NaN included, and refuses an `observations` below the number of non-zero bucket_paths entries and a total N that overflows
 *     64 bits (RL_E_INVALID, before any device work).  They wait for what is queued on the unit.
 *   rl_robust_unit_create refuses a NULL `out`, a zero size, width * height > RL_MAX_PIXELS and n_buckets < 3 or
 *     > RL_ROBUST_MAX_BUCKETS (RL_E_INVALID, in this order, before any device work; the handle is left NULL).
 *     rl_robust_unit_clear restores the initial state (queued on the unit).
 *   rl_robust_params_default: gain 1.0, max_trim 0xffffffff (no limit besides (M - 1) / 2), reserved 0.
 *   One user per robust unit at a time. */
typedef struct RlRobustParams {
    double gain;       /* scales the trim: c = floor(gain * G * M / 2), at most cmax */
    uint32_t max_trim; /* an upper limit of c */
    uint32_t reserved; /* 0 */
} RlRobustParams;
typedef struct RlRobustStats {
    uint64_t observations, paths;    /* k, N */
    uint32_t buckets, largest_trim;  /* M, the largest c */
    uint64_t trimmed_pixels;         /* pixels with c > 0 */
    uint64_t trimmed_buckets;        /* the sum of 2 c over the pixels */
    uint64_t untrimmable_pixels;
} RlRobustStats;

int rl_robust_params_default(RlRobustParams* out);
int rl_robust_unit_create(int device, uint32_t width, uint32_t height, uint32_t n_buckets, RlRobustUnit** out);
int rl_robust_unit_destroy(RlRobustUnit* unit);
int rl_robust_unit_clear(RlRobustUnit* unit);
int rl_robust_unit_observe(RlRobustUnit* unit, RlPlotUnit* plot, uint64_t n_paths, uint32_t bucket);
int rl_robust_unit_resolve(RlRobustUnit* unit, const RlRobustParams* params, RlGatherUnit* dst, RlRobustStats* stats, uint8_t* trim);
int rl_robust_unit_estimate(RlRobustUnit* unit, const RlRobustParams* params, RlErrorStats* stats, float* se, double* tiles, uint8_t* trim);
int rl_robust_unit_download(RlRobustUnit* unit, double* sums, uint64_t* bucket_paths, uint64_t* observations);
int rl_robust_unit_upload(RlRobustUnit* unit, const double* sums, const uint64_t* bucket_paths, uint64_t observations);

/* ---- adaptive sampling: camera samples drawn tile by tile from an importance map (rl_adaptive_unit_*) ---- */

/* An adaptive unit holds a plan for one batch of n_paths camera paths over a width x height film: how many of them start in each
 * RL_ERROR_TILE x RL_ERROR_TILE tile (the error unit's tiles, raster order, tiles_x = ceil(width / 16)), and the weight their
 * splats carry so that the film's expectation is the uniform sampler's.  The importance is the caller's: a tile's t_se of
 * rl_error_unit_estimate is the intended one.
 *   Cells.  In continuous pixel coordinates a photon sits at px = (x * 0.5 + 0.5) * (width - 1) (plot_unit.rs:60-61).  The cell of
 *     tile column i is [max(0, 16 i - 0.5), min(width - 1, 16 i + 15.5)], rows the same way with the height: the cells tile
 *     [0, width - 1] x [0, height - 1] exactly, a partial last tile is a cell like any other (for width = 16 i + 1 the last cell
 *     is 0.5 wide).  The area a_t of a cell is exact in f64; the areas sum to A = (width - 1)(height - 1).
 *   rl_adaptive_unit_plan(unit, importance, uniform_share, n_paths, stats).  importance: tiles_y * tiles_x doubles of host memory
 *     in raster order, or NULL for the uniform plan.  The rule, in f64 in exactly this order, never contracted, the divide correctly
 *     rounded:
 *       g_t = importance[t] if it is finite and > 0, else 0;  G = the sequential sum of g_t in raster order from +0.0.
 *       A G that is infinite is RL_E_INVALID.  NULL, or G == 0: q_t = a_t / A.  Otherwise, with u = uniform_share:
 *         q_t = u * (a_t / A) + (1 - u) * (g_t / G).
 *       e_t = (double)n_paths * q_t;  c_t = floor(e_t);  r_t = e_t - floor(e_t).
 *       The n_paths - sum c_t paths left over go one each to the tiles with the largest r_t, ties to the lower tile index.
 *       w_t = (float)(((double)n_paths * a_t) / (A * (double)c_t)).
 *     So sum c_t == n_paths exactly and |c_t - n_paths q_t| < 1.  Every tile must have c_t >= 1 -- a tile nobody samples is a
 *     biased image: if one would get 0 the call is RL_E_INVALID and the unit keeps its previous plan.  w_t is the unbiasedness
 *     condition: c_t w_t / a_t = n_paths / A for every tile, so any weighted splat has the uniform sampler's expectation, whichever
 *     pixels its four taps land on, a neighbouring tile's included.  The bits of c_t and w_t are the contract
 *     (tests/_adaptive_oracle.py restates the rule in numpy).
 *     Checked in this order, each RL_E_INVALID before any device work: a NULL unit; uniform_share not in (0, 1] (a NaN too);
 *     n_paths == 0 or > 2^32 - 1; then the rule's own refusals.  `stats` may be NULL.  The call uploads the exclusive prefix sums
 *     off[t] of the counts (32 bits), the cells and the weights, and returns when they are on the device.
 *   rl_adaptive_unit_download_plan(unit, counts, weights) reads the plan back from the device: tiles_y * tiles_x uint32_t and
 *     floats of host memory, either may be NULL.  A unit starts with no plan; calls that need one return RL_E_STATE.
 *   rl_adaptive_unit_samples(unit, scene, seed, stream, first_path_index, first_sample, n, out).  out[i] is sample
 *     j = first_sample + i of the plan, which is path first_path_index + j of RNG stream `stream` under `seed`; its tile is the t
 *     with off[t] <= j < off[t + 1].  It draws what rl_scene_camera_rays draws for that path from blocks 0 and 1, word for word: the
 *     wavelength from w[0], the camera time from w[3], the lens from block 1.  Only the screen position differs, f32 in exactly
 *     this order, never contracted, the divide correctly rounded:
 *       u = get_unit(w[1]);  px = x_lo + (x_hi - x_lo) * u;  x = (px / ((float)width - 1) - 0.5f) * 2.0f;
 *       v = get_unit(w[2]);  py = y_lo + (y_hi - y_lo) * v;  y = ((py / ((float)height - 1) - 0.5f) * 2.0f) / aspect_ratio;
 *     with the cell's bounds rounded to f32 and aspect_ratio = (float)width / (float)height.  From there the ray is
 *     rl_scene_camera_rays' arithmetic.  out[i] holds the ray, x, y, reserved0 = t and reserved1 = the bits of w_t; the film calls
 *     that take camera samples ignore both reserved fields.
 *     Checked in this order: a NULL unit, a NULL scene, NULL `out` with n > 0 (RL_E_INVALID); no plan (RL_E_STATE);
 *     first_sample + n > n_paths, path indices that reach 2^64 - 1 (RL_E_INVALID); unit and scene on different devices
 *     (RL_E_STATE).  n = 0 does nothing.  Host and _device forms as rl_scene_camera_rays*; the _device form wants device_out
 *     16-byte aligned (RL_E_INVALID).
 *   rl_plot_unit_render_adaptive(plot, unit, scene, primitive_fetch, seed, stream, first_path_index, max_segments) renders the
 *     whole plan into `plot`, in chunks of at most 2^20 samples in scratch the adaptive unit owns (taken at the first such call):
 *     the samples; their rays traced as rl_scene_render_rays_device traces them (the same launch of the same kernel, so the
 *     results are that call's bit for bit); and for every path with value != 0 and a finite position
 *     get_tristimulus(wavelength) * (value * w_t) -- one f32 multiply of value and weight -- added to the four pixels of
 *     plot_pixel(x, y) by rl_plot_unit_plot_photons' arithmetic.  The buffer then holds an unbiased estimate of what n_paths
 *     uniform paths would sum to, so rl_error_unit_observe(error, plot, n_paths) and rl_gather_unit_accumulate take it as they take
 *     any batch.  Batches under different plans are independent but not identically distributed: the batch-deviation estimate of
 *     the error unit stays valid on the conservative side (the spread between plans adds to the spread it measures).
 *     Checked in this order, each RL_E_INVALID before any device work: NULL plot unit, NULL adaptive unit, NULL scene, unknown
 *     fetch mode, max_segments > RL_PATH_MAX_SEGMENTS_CAP; then no plan (RL_E_STATE); path indices that reach 2^64 - 1
 *     (RL_E_INVALID); a film of another size than the plot unit's, or the three handles not on one device (RL_E_STATE).
 *     Ordering is rl_plot_unit_render_samples_device's: a fused render begun into `plot` ends first, the call runs after everything
 *     queued into the plot unit, orders against open launches as rl_scene_render_rays does, and returns when the splats are in the
 *     buffer.
 *   rl_adaptive_unit_create refuses a NULL `out`, a width or height below 2 (plot_pixel maps x onto [0, width - 1]: a 1-wide film
 *     has no area) and width * height > RL_MAX_PIXELS (RL_E_INVALID, in this order, before any device work).
 *   One user per adaptive unit at a time. */
typedef struct RlAdaptiveStats {
    uint64_t n_paths;
    uint32_t tiles_x, tiles_y;        /* ceil(width / 16), ceil(height / 16) */
    uint32_t min_count, max_count;    /* over the tiles */
    float min_weight, max_weight;
    double importance_sum;            /* G; 0 for the uniform plan */
} RlAdaptiveStats;

int rl_adaptive_unit_create(int device, uint32_t width, uint32_t height, RlAdaptiveUnit** out);
int rl_adaptive_unit_destroy(RlAdaptiveUnit* unit);
int rl_adaptive_unit_plan(RlAdaptiveUnit* unit, const double* importance, double uniform_share, uint64_t n_paths,
                          RlAdaptiveStats* stats);
int rl_adaptive_unit_download_plan(RlAdaptiveUnit* unit, uint32_t* counts, float* weights);
int rl_adaptive_unit_samples(RlAdaptiveUnit* unit, const RlScene* scene, uint64_t seed, uint32_t stream, uint64_t first_path_index,
                             uint64_t first_sample, uint32_t n, RlCameraSample* out);
int rl_adaptive_unit_samples_device(RlAdaptiveUnit* unit, const RlScene* scene, uint64_t seed, uint32_t stream,
                                    uint64_t first_path_index, uint64_t first_sample, uint32_t n, RlCameraSample* device_out);
int rl_plot_unit_render_adaptive(RlPlotUnit* plot, RlAdaptiveUnit* unit, const RlScene* scene, int primitive_fetch, uint64_t seed,
                                 uint32_t stream, uint64_t first_path_index, uint32_t max_segments);

/* ---- GatherUnit (gather_unit.rs:24-92) ----------------------------------------------------- */

/* GatherUnit::new(width, height) WITHOUT the implicit read() of ./buffer.raw
 * (gather_unit.rs:42-43): resuming is explicit through rl_gather_unit_load. */
int rl_gather_unit_create(int device, uint32_t width, uint32_t height, RlGatherUnit** out);
int rl_gather_unit_destroy(RlGatherUnit* unit);
/* GatherUnit::accumulate(&plot.tristimulus_buffer) followed by plot.clear()
 * (app.rs:143-148, gather_unit.rs:49-64): Kahan-compensated, never re-associated. */
int rl_gather_unit_accumulate(RlGatherUnit* unit, RlPlotUnit* plot);
/* GatherUnit::save / read (gather_unit.rs:68-92): headerless tristimulus then compensation
 * buffers, 12 native-endian bytes per pixel each.  A short file leaves the tail untouched
 * (read.rs:20-32). */
int rl_gather_unit_save(RlGatherUnit* unit, const char* path);
int rl_gather_unit_load(RlGatherUnit* unit, const char* path);
int rl_gather_unit_download(RlGatherUnit* unit, RlVector3* tristimulus, RlVector3* compensation);
/* Blocks until every accumulate / tonemap queued on this gather unit is done (they run on its own stream). */
int rl_gather_unit_sync(RlGatherUnit* unit);

/* ---- the GatherUnit-time exchange between GPUs (no reference counterpart: the reference is one process on
 * one CPU) ---------------------------------------------------------------------------------------
 * Samples shard: every GPU renders the full frame with its own RNG stream into its own plot units, and the only
 * exchange is the element-wise f32 sum of the tristimulus buffers (3*W*H floats) onto rank 0 when a plot unit
 * is gathered -- one ncclReduce over xGMI -- followed by rank 0's Kahan accumulation (gather_unit.rs:49-64).
 * RCCL is loaded at run time (dlopen) by the first rl_comm_* call; RL_E_NO_DEVICE if it is absent. */
#define RL_COMM_ID_BYTES 128
/* One rank per process (torchrun / MPI style launchers): rank 0 obtains an id, hands the 128 bytes to the other
 * ranks over any channel, and every rank joins with its own device. */
int rl_comm_unique_id(uint8_t id[RL_COMM_ID_BYTES]);
int rl_comm_init_rank(const uint8_t id[RL_COMM_ID_BYTES], int world, int rank, int device, RlComm** out);
/* One process driving n distinct GPUs: out[i] is rank i on devices[i]. */
int rl_comm_init_all(const int* devices, int n, RlComm** out);
int rl_comm_destroy(RlComm* comm);
int rl_comm_rank(const RlComm* comm, int* rank, int* world);
/* What the exchange really runs on, for a measurement that has to explain itself: the rank, the size RCCL reports for the
 * communicator (ncclCommCount), the RCCL version (ncclGetVersion, e.g. 22707) and the path of the library that was
 * loaded.  Any output may be NULL. */
int rl_comm_info(const RlComm* comm, int* rank, int* world, int* rccl_version, char* library_path, uint32_t path_cap);
/* ncclGroupStart / ncclGroupEnd: a single host thread that issues the collective for several ranks brackets
 * the calls with these (one thread or process per rank needs neither). */
int rl_comm_group_start(void);
int rl_comm_group_end(void);
/* The exchange: sums this plot unit's tristimulus buffer with those of the other ranks into rank `root`'s
 * buffer, in place (ncclReduce, f32, sum).  Collective: every rank calls it with its own plot unit of the same
 * size.  Queued on the plot unit's stream, i.e. after every plot / fused render into the buffer. */
int rl_plot_unit_reduce(RlPlotUnit* unit, RlComm* comm, int root);
/* Device time of this unit's exchanges so far: every rl_plot_unit_reduce is bracketed by events on the plot unit's
 * stream.  Waits for the ones still in flight.  Cumulative since creation. */
int rl_plot_unit_exchange_stats(RlPlotUnit* unit, uint64_t* exchanges, double* device_ms);
/* dst += src for two plot units on the SAME device (two RNG streams rendered by one GPU); src is left as it is. */
int rl_plot_unit_add(RlPlotUnit* dst, RlPlotUnit* src);
/* Task::Gather on G GPUs in one call per rank: rl_plot_unit_reduce(plot, comm, 0), then on rank 0
 * rl_gather_unit_accumulate(gather, plot) and on the other ranks rl_plot_unit_clear(plot) (gather may be NULL
 * there).  For one thread or process per rank; a single thread driving several ranks uses the three calls
 * itself with the reduces inside rl_comm_group_start/end. */
int rl_gather_unit_allreduce(RlGatherUnit* gather, RlPlotUnit* plot, RlComm* comm);

/* ---- TonemapUnit (tonemap_unit.rs:21-100, srgb.rs:20-41) ------------------------------------ */

int rl_tonemap_unit_create(int device, uint32_t width, uint32_t height, RlTonemapUnit** out);
int rl_tonemap_unit_destroy(RlTonemapUnit* unit);
/* TonemapUnit::tonemap(&gather.tristimulus_buffer) (tonemap_unit.rs:73-100). */
int rl_tonemap_unit_tonemap(RlTonemapUnit* unit, RlGatherUnit* gather);
/* rgb_buffer (tonemap_unit.rs:30): width*height*3 bytes RGB8. */
int rl_tonemap_unit_rgb(RlTonemapUnit* unit, uint8_t* out);
/* The clamped sRGB value before `* 255 as u8` (tonemap_unit.rs:88-98), width*height*3 floats, and
 * the exposure estimate of find_exposure (tonemap_unit.rs:55-69).  Either pointer may be NULL. */
int rl_tonemap_unit_srgb_float(RlTonemapUnit* unit, float* out, float* max_intensity);

/* ---- Task / TaskScheduler (task_scheduler.rs:26-182) --------------------------------------- */

enum RlTaskKind { RL_TASK_SLEEP = 0, RL_TASK_TRACE = 1, RL_TASK_PLOT = 2, RL_TASK_GATHER = 3, RL_TASK_TONEMAP = 4 };

/* Capacity of RlTask::units: 3 * concurrency trace units must fit, so at most 85 worker threads (the reference
 * uses num_cpus::get(), app.rs:55; a GPU is saturated by 8-16 workers).  rl_scheduler_create and
 * rl_app_run return RL_E_INVALID with a message naming the limit beyond it. */
#define RL_TASK_MAX_UNITS 256

/* enum Task by value (task_scheduler.rs:26-41), units named by their ids (trace_unit.rs:59,
 * plot_unit.rs:37).  unit = the trace/plot unit of Trace/Plot; units[] = the trace units of a Plot
 * or the plot units of a Gather. */
typedef struct RlTask {
    uint32_t kind; /* enum RlTaskKind */
    uint32_t unit;
    uint32_t n_units;
    uint32_t units[RL_TASK_MAX_UNITS];
} RlTask;

/* TaskScheduler::new(concurrency, width, height) (task_scheduler.rs:91-125) over unit ids only:
 * 3*concurrency trace units, max(1, concurrency/2) plot units.  tonemap_interval_ms replaces the
 * hard-coded 30 s (task_scheduler.rs:44-46). */
int rl_scheduler_create(uint32_t concurrency, int64_t tonemap_interval_ms, RlScheduler** out);
int rl_scheduler_destroy(RlScheduler* s);
/* TaskScheduler::get_new_task(completed) (task_scheduler.rs:127-182).  now_ms is the caller's
 * monotonic clock (the reference calls time::get_time() inside). */
int rl_scheduler_get_new_task(RlScheduler* s, const RlTask* completed, int64_t now_ms, RlTask* next);
/* Mean and standard deviation of batches/sec over the last <= 512 tonemap intervals
 * (task_scheduler.rs:308-325). */
int rl_scheduler_performance(RlScheduler* s, float* mean, float* stddev);

/* ---- App (app.rs:48-164) ----------------------------------------------------------------------- */

typedef struct RlAppConfig {
    uint32_t width, height;      /* main.rs:47-48 (1280 x 720 there) */
    int device;                  /* GPU that takes the place of the CPU worker pool */
    uint32_t concurrency;        /* scheduler depth = worker threads unless `threads` says otherwise; the reference uses num_cpus::get() (app.rs:55) */
    uint32_t photons_per_batch;  /* 0 -> 1024*512 (trace_unit.rs:67) */
    uint64_t seed;
    uint32_t stream;             /* RNG stream (multi-GPU: the rank) */
    int builtin_scene;           /* enum RlBuiltinScene */
    int builtin_param;
    uint64_t max_batches;        /* stop after this many trace tasks (the reference never stops, main.rs:57) */
    int64_t tonemap_interval_ms; /* 30000 in the reference (task_scheduler.rs:44-46) */
    int fused;                   /* 0: Trace fills mapped_photons, Plot splats them (reference structure);
                                    1: Trace renders straight into the plot unit it will be plotted by */
    const char* output_ppm;      /* image written after every tonemap: "*.png" -> PNG (the reference's output.png,
                                    main.rs:61), anything else -> binary PPM (P6); NULL = none */
    const char* checkpoint;      /* GatherUnit::save target, written at every tonemap and at the end; NULL = none */
    int resume;                  /* non-zero: rl_gather_unit_load(checkpoint) before rendering (gather_unit.rs:42-43) */
    int verbose;                 /* print the reference's progress lines (task_scheduler.rs:242-325) */
    uint32_t sleep_us;           /* how long Task::Sleep waits before the worker asks again.  The reference sleeps
                                    100 ms (app.rs:129) because its tasks take seconds; a task here takes about a
                                    millisecond, so 0 selects 200 us.  100000 restores the reference's value. */
    uint64_t first_batch;        /* index of the first batch this run renders; batch b is the path indices
                                    [b * photons_per_batch, (b + 1) * photons_per_batch) of every rank's RNG stream.
                                    With `resume` the larger of this and the index stored beside the checkpoint
                                    ("<checkpoint>.next", written with every save) is used, so a resumed run adds new
                                    samples instead of repeating the old ones.  RlAppStats::next_batch continues a run
                                    by hand. */
    uint32_t n_devices;          /* 0 or 1: render on `device`.  G > 1: one process drives G ranks; every scheduler
                                    unit is one unit per rank, rank r uses RNG stream `stream + r`, and Task::Gather
                                    sums the ranks' plot buffers onto rank 0 first (rl_plot_unit_reduce over xGMI for
                                    distinct GPUs, rl_plot_unit_add for ranks that share one) */
    int blocking_trace;          /* 0 (default): a task BEGINS its render (rl_trace_unit_render_begin, un-fused in the Trace task;
                                    rl_trace_unit_render_fused_begin, fused in the Plot task) and the worker moves on; the task
                                    that uses the result next -- Plot resp. Gather -- ends it.  Non-zero: the task waits for its
                                    own paths, like a reference worker that traces them itself (slower with few workers: the
                                    device only ever has `concurrency` batches to work on) */
    const int* devices;          /* n_devices device indices, rank 0 first (gather, tonemap and output live there);
                                    NULL = device, device + 1, ...  A device may be listed more than once. */
    uint32_t threads;            /* host worker threads; 0 = `concurrency`, as in the reference (app.rs:55,66: one thread per unit
                                    of scheduler depth).  The scheduler's pools are sized by `concurrency` (3 x trace units,
                                    concurrency / 2 plot units, task_scheduler.rs:95-96) -- how many batches the DEVICE can have in
                                    flight; a task here only begins or enqueues device work, so a host with few cores per GPU
                                    sets e.g. concurrency = 16, threads = 2: the pool stays deep, two threads issue it */
} RlAppConfig;

typedef struct RlAppStats {
    uint64_t batches, paths, segments;
    uint64_t tasks[5];           /* executed tasks by RlTaskKind */
    double seconds;
    double kernel_ms;            /* device time in trace kernels */
    float batches_per_sec_mean, batches_per_sec_stddev; /* task_scheduler.rs:308-325 */
    uint32_t tonemaps;
    uint64_t next_batch;         /* first_batch of a run that continues this one */
} RlAppStats;

/* App::new + the worker loops (app.rs:54-111) until max_batches trace tasks are done, gathered and
 * tonemapped once more.  The batches cover the path indices [first_batch * photons_per_batch,
 * (first_batch + max_batches) * photons_per_batch) of every rank's RNG stream exactly once (un-fused: trace task number k, in scheduler order, renders batch k; fused: each plot task renders the
 * batches of its trace units as one launch over the next contiguous range), so the final image does not
 * depend on which worker or unit ran which task.  rgb_out (may be NULL) receives the last RGB8 image. */
int rl_app_run(const RlAppConfig* config, RlAppStats* stats, uint8_t* rgb_out);

/* ---- render until a target error (rl_app_run_to_error) ---- */

typedef struct RlErrorTarget {
    double relative_error;     /* stop when the estimate is <= this; 0 never stops a noisy render */
    double worst_tile_error;   /* 0 = not part of the rule; otherwise the worst tile must be <= this too */
    uint32_t min_observations; /* 0 = 16 */
    uint32_t reserved;         /* must be 0 */
} RlErrorTarget;

typedef struct RlAppErrorStats {
    RlErrorStats at_stop;      /* the estimate that met the target; zeros if none did */
    RlErrorStats at_end;       /* after the last gather (zeros if the run made fewer than two observations) */
    uint32_t reached, estimates;
} RlAppErrorStats;

/* rl_app_run with a stopping rule.  With a NULL target it is rl_app_run (error_stats, if given, is zeroed).  With a target the App
 * owns an error unit on rank 0's device.  It counts, per plot unit, the paths plotted or fused into it since its last gather, over
 * all ranks; the Gather task calls rl_error_unit_observe with that count just before its rl_gather_unit_accumulate, after the
 * ranks' buffers have been summed onto rank 0, and skips a buffer whose count is zero.  Every Tonemap task runs the estimate before
 * tonemapping (once k >= 2); when k >= min_observations and relative_error <= target->relative_error (and, with a non-zero
 * target->worst_tile_error, worst_tile_error <= it: a NaN meets neither) the hand-out of trace tasks ends exactly as at an exhausted
 * max_batches, which stays the upper limit.  The run then gathers what is in flight, estimates once more (at_end) and tonemaps.
 * `estimates` counts the estimates made, at_end's included.  Tonemap tasks come every tonemap_interval_ms, so that is how often
 * the rule is looked at.  16 observations by default: the relative standard deviation of a variance estimate on k - 1 degrees of
 * freedom is sqrt(2 / (k - 1)), 0.37 at 16, so about 0.18 on one pixel's se, and the sums average that over hundreds of pixels.
 *   Checked before any device work, after rl_app_run's own checks: a negative or NaN relative_error or worst_tile_error, or a
 * non-zero reserved, is RL_E_INVALID.
 *   With `resume` the estimate covers this run's samples only, so it overstates the error of the resumed image: conservative.  The
 * error state is not kept beside the checkpoint.
 *   rl_app_error_tiles: the {t_se, t_y} pairs of at_end of the calling thread's last rl_app_run_to_error, tiles in raster order.
 * *n_tiles (may be NULL) is always set to their number (0 if that run made no final estimate); `tiles` receives 2 * n doubles when
 * capacity >= n, else RL_E_INVALID -- the capacity protocol of rl_scene_emitters.
 *   rl_app_error_state: the error unit's state at the end of the calling thread's last rl_app_run_to_error -- the planes S and Q,
 * width x height doubles in rows, the observations k and the paths N -- which otherwise dies with the run.  The same protocol:
 * *n_pixels, *observations and *paths (each may be NULL) are always set, to zeros after a run without a target or one that made no
 * observation; sum_y and sum_q each receive n doubles when capacity_pixels >= n, else RL_E_INVALID.  The planes are downloaded
 * once per run, after the final estimate and after stats->seconds is taken.  Uploaded into an error unit of the caller's
 * (rl_error_unit_upload) they give at_end's estimate again, and rl_denoise_unit_denoise_variance the variance of the run's image. */
int rl_app_run_to_error(const RlAppConfig* config, const RlErrorTarget* target, RlAppStats* stats, RlAppErrorStats* error_stats,
                        uint8_t* rgb_out);
int rl_app_error_tiles(double* tiles, uint32_t capacity, uint32_t* n_tiles);
int rl_app_error_state(double* sum_y, double* sum_q, uint64_t capacity_pixels, uint64_t* n_pixels, uint64_t* observations,
                       uint64_t* paths);

/* ---- the App with wavelength importance sampling (rl_app_run_sampled) ---- */

typedef struct RlWavelengthSampling {
    const double* importance; /* n_nodes values from 380 to 780 nm (NULL: uniform), as rl_wavelength_table_create takes them */
    uint32_t n_nodes;
    uint32_t reserved;        /* must be 0 */
    double uniform_share;
} RlWavelengthSampling;

/* rl_app_run_to_error whose trace units draw their wavelengths by importance: the App creates one table per rank, on the rank's
 * device, sets it on every trace unit of the rank (rl_trace_unit_set_wavelengths) and destroys it with them.  With a NULL
 * `sampling` it is rl_app_run_to_error; `target` may be NULL as there.  RlAppConfig keeps its layout.  The sampling's arguments are
 * checked as rl_wavelength_table_create checks them, after rl_app_run_to_error's own checks and before any device work; a non-zero
 * reserved is RL_E_INVALID too.  rl_app_error_tiles and rl_app_error_state serve this call as they serve rl_app_run_to_error. */
int rl_app_run_sampled(const RlAppConfig* config, const RlErrorTarget* target, const RlWavelengthSampling* sampling, RlAppStats* stats,
                       RlAppErrorStats* error_stats, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif /* ROBIGO_LUCULENTA_H */
