// ffi.rs -- Rust declarations of every entry point of include/robigo_luculenta.h
// (tests/test_abi.py parses both files and compares every function's arity, argument and return types through a
// C -> Rust type map, and every #[repr(C)] struct's field names, order, types and size with the header and with
// the ctypes mirror, so a u32 swapped for a u64 fails the test).
// Documentation artefact: this image has no rustc, so the file is compiled only where cargo exists;
// INTEGRATION.md explains how the reference's units wrap these handles.
#![allow(dead_code)]
use std::os::raw::{c_char, c_double, c_float, c_int};

#[repr(C)] #[derive(Copy, Clone)] pub struct RlVector3 { pub x: f32, pub y: f32, pub z: f32 }          // vector3.rs:20-25
#[repr(C)] #[derive(Copy, Clone)] pub struct RlMappedPhoton { pub x: f32, pub y: f32, pub probability: f32, pub wavelength: f32 } // trace_unit.rs:23-37
#[repr(C)] #[derive(Copy, Clone)] pub struct RlObjectDesc {
    pub surface_kind: u32, pub material_kind: u32, pub v0: RlVector3, pub v1: RlVector3,
    pub f0: f32, pub f1: f32, pub f2: f32, pub f3: f32, pub m0: f32, pub m1: f32, pub m2: f32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct RlCameraDesc {
    pub phi0: f32, pub phi1: f32, pub alpha0: f32, pub alpha1: f32, pub dist0: f32, pub dist1: f32,
    pub fov_over_pi: f32, pub focal_factor: f32, pub depth_of_field: f32, pub chromatic_abberation: f32,
}
#[repr(C)] pub struct RlSceneDesc { pub n_objects: u32, pub objects: *const RlObjectDesc, pub camera: RlCameraDesc }
// Scene::intersect as a batched query (rl_scene_intersect*): ray.rs:19-33 without wavelength and probability, intersection.rs:20-32
#[repr(C)] #[derive(Copy, Clone)] pub struct RlRay { pub origin: RlVector3, pub t_max: f32, pub direction: RlVector3, pub reserved: u32 } // 32 bytes
#[repr(C)] #[derive(Copy, Clone)] pub struct RlIntersection { pub position: RlVector3, pub normal: RlVector3, pub tangent: RlVector3, pub distance: f32 } // 40 bytes
#[repr(C)] #[derive(Copy, Clone)] pub struct RlRayHit { pub isect: RlIntersection, pub object: u32, pub reserved: u32 } // 48 bytes
pub const RL_OBJECT_NONE: u32 = 0xffff_ffff;
// TraceUnit::render_ray on caller-supplied rays (rl_scene_camera_rays*, rl_scene_render_rays*)
#[repr(C)] #[derive(Copy, Clone)] pub struct RlSpectralRay { pub origin: RlVector3, pub wavelength: f32, pub direction: RlVector3, pub reserved: u32 } // 32 bytes
#[repr(C)] #[derive(Copy, Clone)] pub struct RlCameraSample { pub ray: RlSpectralRay, pub x: f32, pub y: f32, pub reserved0: u32, pub reserved1: u32 } // 48 bytes
#[repr(C)] #[derive(Copy, Clone)] pub struct RlPathResult { pub value: f32, pub segments: u32, pub object: u32, pub end: u32 } // 16 bytes
pub const RL_PATH_END_VOID: u32 = 0;
pub const RL_PATH_END_EMITTER: u32 = 1;
pub const RL_PATH_END_ROULETTE: u32 = 2;
pub const RL_PATH_END_LIMIT: u32 = 3;
pub const RL_PATH_END_INVALID: u32 = 4;
pub const RL_PATH_MAX_SEGMENTS: u32 = 4096;
pub const RL_PATH_MAX_SEGMENTS_CAP: u32 = 65536;
pub const RL_FEATURE_VOID: u32 = 0;
pub const RL_FEATURE_EMITTER: u32 = 1;
pub const RL_FEATURE_DIFFUSE: u32 = 2;
pub const RL_FEATURE_LIMIT: u32 = 3;
pub const RL_FEATURE_MAX_SEGMENTS: u32 = 64;
// one turn of render_ray's loop at a time on states the caller holds (rl_scene_begin_paths*, rl_scene_step_paths*)
#[repr(C)] #[derive(Copy, Clone)] pub struct RlPathState {
    pub origin: RlVector3, pub wavelength: f32, pub direction: RlVector3, pub intensity: f32, pub continue_chance: f32,
    pub segments: u32, pub end: u32, pub value: f32, pub path_index: u64, pub object: u32, pub reserved: u32,
} // 64 bytes
pub const RL_PATH_LIVE: u32 = 0xffff_ffff;
pub const RL_STEP_NO_ROULETTE: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct RlLightSample {      // rl_scene_light_paths: one direct-light sample per path vertex
    pub direction: RlVector3, pub distance: f32, pub value: f32, pub weight: f32, pub emitter: u32,
    pub status: u32,    // 0 skipped, 1 backfacing, 2 occluded, 3 visible
} // 32 bytes
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlDirectStats {      // rl_plot_unit_render_direct: what one call did, exact counts
    pub paths: u64, pub segments: u64, pub light_samples: u64, pub shadow_rays: u64, pub visible: u64,
    pub endings_kept: u64, pub endings_dropped: u64,
} // 56 bytes
#[repr(C)] #[derive(Copy, Clone)] pub struct RlFeatureSample {             // rl_scene_render_features: the guide record of one path
    pub x: f32, pub y: f32, pub wavelength: f32, pub albedo: f32, pub normal: RlVector3, pub depth: f32,
    pub object: u32, pub segments: u32,
    pub kind: u32,      // RL_FEATURE_*
    pub reserved: u32,
} // 48 bytes
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlFeatureStats {     // rl_scene_render_features: what one call did, exact counts
    pub paths: u64, pub segments: u64, pub kinds: [u64; 4],
} // 48 bytes
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlDenoiseParams {    // rl_denoise_unit_denoise: 0 iterations = 5, a sigma of 0 = that term off
    pub iterations: u32, pub sigma_colour: f32, pub sigma_normal: f32, pub sigma_depth: f32, pub sigma_albedo: f32,
    pub reserved: [u32; 3],
} // 32 bytes
pub const RL_DENOISE_ITERATIONS: u32 = 5;
pub const RL_DENOISE_MAX_ITERATIONS: u32 = 6;
pub const RL_SPECTRAL_MAX_NODES: u32 = 401;
pub const RL_GLARE_MAX_TAPS: u32 = 65;
pub const RL_ERROR_TILE: u32 = 16;
pub const RL_RELIGHT_MAX_GROUPS: u32 = 16;
pub const RL_RELIGHT_DROP: u8 = 0xff;
pub const RL_ROBUST_NEXT: u32 = 0xffff_ffff;

pub const RL_MAX_PIXELS: usize = 2147483647;
pub const RL_TASK_MAX_UNITS: usize = 256;
pub const RL_COMM_ID_BYTES: usize = 128;
pub const RL_ROBUST_MAX_BUCKETS: usize = 32;
#[repr(C)] #[derive(Copy, Clone)] pub struct RlTask {            // enum Task by value, task_scheduler.rs:26-41
    pub kind: u32,      // 0 Sleep, 1 Trace, 2 Plot, 3 Gather, 4 Tonemap
    pub unit: u32, pub n_units: u32, pub units: [u32; RL_TASK_MAX_UNITS],
}
#[repr(C)] pub struct RlAppConfig {
    pub width: u32, pub height: u32, pub device: c_int, pub concurrency: u32, pub photons_per_batch: u32,
    pub seed: u64, pub stream: u32, pub builtin_scene: c_int, pub builtin_param: c_int, pub max_batches: u64,
    pub tonemap_interval_ms: i64, pub fused: c_int, pub output_ppm: *const c_char, pub checkpoint: *const c_char,
    pub resume: c_int, pub verbose: c_int, pub sleep_us: u32, pub first_batch: u64, pub n_devices: u32, pub blocking_trace: c_int, pub devices: *const c_int, pub threads: u32,
}
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlAppStats {
    pub batches: u64, pub paths: u64, pub segments: u64, pub tasks: [u64; 5], pub seconds: c_double, pub kernel_ms: c_double,
    pub batches_per_sec_mean: c_float, pub batches_per_sec_stddev: c_float, pub tonemaps: u32, pub next_batch: u64,
}

#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlErrorStats {
    pub observations: u64, pub paths: u64, pub tiles_x: u32, pub tiles_y: u32, pub worst_tile_x: u32, pub worst_tile_y: u32,
    pub sum_y: f64, pub sum_se: f64, pub relative_error: f64, pub worst_tile_error: f64,
}
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlRobustParams { pub gain: f64, pub max_trim: u32, pub reserved: u32 } // 16 bytes
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlRobustStats {
    pub observations: u64, pub paths: u64, pub buckets: u32, pub largest_trim: u32,
    pub trimmed_pixels: u64, pub trimmed_buckets: u64, pub untrimmable_pixels: u64,
}
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlErrorTarget {
    pub relative_error: f64, pub worst_tile_error: f64, pub min_observations: u32, pub reserved: u32,
}
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlAdaptiveStats {
    pub n_paths: u64, pub tiles_x: u32, pub tiles_y: u32, pub min_count: u32, pub max_count: u32,
    pub min_weight: f32, pub max_weight: f32, pub importance_sum: f64,
}
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct RlAppErrorStats {
    pub at_stop: RlErrorStats, pub at_end: RlErrorStats, pub reached: u32, pub estimates: u32,
}

pub enum RlScene {} pub enum RlTraceUnit {} pub enum RlPlotUnit {} pub enum RlGatherUnit {} pub enum RlTonemapUnit {}
pub enum RlScheduler {} pub enum RlComm {} pub enum RlDenoiseUnit {} pub enum RlSpectralUnit {} pub enum RlErrorUnit {}
pub enum RlAdaptiveUnit {}
pub enum RlRobustUnit {}
pub enum RlRelightUnit {} pub enum RlGlareUnit {}
pub enum RlWavelengthTable {}
#[repr(C)] #[derive(Copy, Clone)] pub struct RlWavelengthSampling {
    pub importance: *const f64, pub n_nodes: u32, pub reserved: u32, pub uniform_share: f64,
}
pub const RL_WAVELENGTH_BINS: usize = 256;

extern "C" {
    pub fn rl_last_error() -> *const c_char;
    pub fn rl_device_count() -> c_int;
    pub fn rl_device_pci_bus_id(device: c_int, out: *mut c_char, cap: u32) -> c_int;
    pub fn rl_version() -> *const c_char;
    pub fn rl_build_id() -> *const c_char;
    pub fn rl_scene_builtin_desc(which: c_int, param: c_int, objects: *mut RlObjectDesc, cap: u32,
                                 n_objects: *mut u32, camera: *mut RlCameraDesc) -> c_int;
    pub fn rl_scene_desc_save(path: *const c_char, desc: *const RlSceneDesc) -> c_int;
    pub fn rl_scene_desc_load(path: *const c_char, objects: *mut RlObjectDesc, cap: u32, n_objects: *mut u32,
                              camera: *mut RlCameraDesc) -> c_int;
    pub fn rl_scene_create(desc: *const RlSceneDesc, device: c_int, out: *mut *mut RlScene) -> c_int;
    pub fn rl_scene_destroy(scene: *mut RlScene) -> c_int;
    pub fn rl_scene_intersect(scene: *const RlScene, primitive_fetch: c_int, rays: *const RlRay, n_rays: u32, hits: *mut RlRayHit) -> c_int;
    pub fn rl_scene_intersect_device(scene: *const RlScene, primitive_fetch: c_int, device_rays: *const RlRay, n_rays: u32,
                                     device_hits: *mut RlRayHit) -> c_int;
    // the any-hit form: one byte per ray, 1 where rl_scene_intersect would report an object
    pub fn rl_scene_occluded(scene: *const RlScene, primitive_fetch: c_int, rays: *const RlRay, n_rays: u32, occluded: *mut u8) -> c_int;
    pub fn rl_scene_occluded_device(scene: *const RlScene, primitive_fetch: c_int, device_rays: *const RlRay, n_rays: u32,
                                    device_occluded: *mut u8) -> c_int;
    pub fn rl_scene_camera_rays(scene: *const RlScene, width: u32, height: u32, seed: u64, stream: u32, first_path_index: u64, n: u32,
                                samples: *mut RlCameraSample) -> c_int;
    pub fn rl_scene_camera_rays_device(scene: *const RlScene, width: u32, height: u32, seed: u64, stream: u32, first_path_index: u64,
                                       n: u32, device_samples: *mut RlCameraSample) -> c_int;
    pub fn rl_scene_render_rays(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, first_path_index: u64,
                                max_segments: u32, rays: *const RlSpectralRay, n_rays: u32, results: *mut RlPathResult) -> c_int;
    pub fn rl_scene_render_rays_device(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, first_path_index: u64,
                                       max_segments: u32, device_rays: *const RlSpectralRay, n_rays: u32,
                                       device_results: *mut RlPathResult) -> c_int;
    pub fn rl_scene_begin_paths(scene: *const RlScene, first_path_index: u64, rays: *const RlSpectralRay, n: u32,
                                states: *mut RlPathState) -> c_int;
    pub fn rl_scene_begin_paths_device(scene: *const RlScene, first_path_index: u64, device_rays: *const RlSpectralRay, n: u32,
                                       device_states: *mut RlPathState) -> c_int;
    pub fn rl_scene_step_paths(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, flags: u32,
                               states: *mut RlPathState, n: u32, hits: *mut RlRayHit) -> c_int;
    pub fn rl_scene_step_paths_device(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, flags: u32,
                                      device_states: *mut RlPathState, n: u32, device_hits: *mut RlRayHit) -> c_int;
    pub fn rl_scene_step_path_list(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, flags: u32,
                                   states: *mut RlPathState, n_states: u32, list: *const u32, n_list: u32, hits: *mut RlRayHit,
                                   live_list: *mut u32, n_live: *mut u32) -> c_int;
    pub fn rl_scene_step_path_list_device(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, flags: u32,
                                          device_states: *mut RlPathState, n_states: u32, device_list: *const u32, n_list: u32,
                                          device_hits: *mut RlRayHit, device_live_list: *mut u32, n_live: *mut u32) -> c_int;
    pub fn rl_scene_emitters(scene: *const RlScene, objects: *mut u32, cap: u32, n_emitters: *mut u32) -> c_int;
    pub fn rl_scene_light_paths(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, states: *const RlPathState,
                                n_states: u32, list: *const u32, n_list: u32, hits: *const RlRayHit, samples: *mut RlLightSample) -> c_int;
    pub fn rl_scene_light_paths_device(scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                       device_states: *const RlPathState, n_states: u32, device_list: *const u32, n_list: u32,
                                       device_hits: *const RlRayHit, device_samples: *mut RlLightSample) -> c_int;

    pub fn rl_trace_unit_create(device: c_int, id: u32, w: u32, h: u32, n_photons: u32, out: *mut *mut RlTraceUnit) -> c_int;
    pub fn rl_trace_unit_destroy(u: *mut RlTraceUnit) -> c_int;
    pub fn rl_trace_unit_set_fetch(u: *mut RlTraceUnit, primitive_fetch: c_int) -> c_int;   // 0 LDS, 1 global
    pub fn rl_wavelength_table_create(device: c_int, importance: *const f64, n_nodes: u32, uniform_share: f64,
                                      out: *mut *mut RlWavelengthTable) -> c_int;
    pub fn rl_wavelength_table_destroy(table: *mut RlWavelengthTable) -> c_int;
    pub fn rl_wavelength_table_download(table: *mut RlWavelengthTable, quantiles: *mut f32, weights: *mut f32) -> c_int;   // 257, 256
    pub fn rl_wavelength_importance_cie1931(out: *mut f64) -> c_int;   // 81
    pub fn rl_trace_unit_set_wavelengths(u: *mut RlTraceUnit, table: *const RlWavelengthTable) -> c_int;   // null: the uniform draw
    pub fn rl_trace_unit_render(u: *mut RlTraceUnit, scene: *const RlScene, seed: u64, stream: u32, first_path: u64) -> c_int;
    pub fn rl_trace_unit_render_begin(u: *mut RlTraceUnit, scene: *const RlScene, seed: u64, stream: u32, first_path: u64) -> c_int;
    pub fn rl_trace_unit_render_end(u: *mut RlTraceUnit) -> c_int;
    pub fn rl_trace_unit_render_async(u: *mut RlTraceUnit, scene: *const RlScene, seed: u64, stream: u32, first_path: u64) -> c_int;
    pub fn rl_trace_unit_render_fused(u: *mut RlTraceUnit, scene: *const RlScene, plot: *mut RlPlotUnit,
                                      seed: u64, stream: u32, first_path: u64, n_paths: u64) -> c_int;
    pub fn rl_trace_unit_render_fused_sync(u: *mut RlTraceUnit, scene: *const RlScene, plot: *mut RlPlotUnit,
                                           seed: u64, stream: u32, first_path: u64, n_paths: u64) -> c_int;
    pub fn rl_trace_unit_render_fused_begin(u: *mut RlTraceUnit, scene: *const RlScene, plot: *mut RlPlotUnit,
                                            seed: u64, stream: u32, first_path: u64, n_paths: u64) -> c_int;
    pub fn rl_trace_unit_sync(u: *mut RlTraceUnit) -> c_int;
    pub fn rl_trace_unit_photons(u: *mut RlTraceUnit, out: *mut RlMappedPhoton) -> c_int;
    pub fn rl_trace_unit_stats(u: *mut RlTraceUnit, paths: *mut u64, segments: *mut u64, kernel_ms: *mut c_double) -> c_int;

    pub fn rl_plot_unit_create(device: c_int, id: u32, w: u32, h: u32, external_xyz: *mut f32, out: *mut *mut RlPlotUnit) -> c_int;
    pub fn rl_plot_unit_destroy(u: *mut RlPlotUnit) -> c_int;
    pub fn rl_plot_unit_plot(u: *mut RlPlotUnit, trace_units: *const *mut RlTraceUnit, n: u32) -> c_int;
    pub fn rl_plot_unit_clear(u: *mut RlPlotUnit) -> c_int;
    pub fn rl_plot_unit_sync(u: *mut RlPlotUnit) -> c_int;
    pub fn rl_plot_unit_device_buffer(u: *mut RlPlotUnit, device_xyz: *mut *mut f32) -> c_int;
    pub fn rl_plot_unit_download(u: *mut RlPlotUnit, out: *mut RlVector3) -> c_int;
    pub fn rl_plot_unit_upload(u: *mut RlPlotUnit, input: *const RlVector3) -> c_int;
    // PlotUnit::plot for photons the caller holds, and render_ray for the caller's camera samples with the splat (a film).
    pub fn rl_plot_unit_plot_photons(u: *mut RlPlotUnit, photons: *const RlMappedPhoton, n: u64) -> c_int;
    pub fn rl_plot_unit_plot_photons_device(u: *mut RlPlotUnit, device_photons: *const RlMappedPhoton, n: u64) -> c_int;
    pub fn rl_plot_unit_render_samples(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                       first_path_index: u64, max_segments: u32, samples: *const RlCameraSample, n: u32,
                                       results: *mut RlPathResult) -> c_int;
    pub fn rl_plot_unit_render_samples_device(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                              first_path_index: u64, max_segments: u32, device_samples: *const RlCameraSample, n: u32,
                                              device_results: *mut RlPathResult) -> c_int;
    pub fn rl_plot_unit_light_paths(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                    states: *const RlPathState, n_states: u32, list: *const u32, n_list: u32, hits: *const RlRayHit,
                                    camera: *const RlCameraSample, sampled: *mut u8, samples: *mut RlLightSample) -> c_int;
    pub fn rl_plot_unit_light_paths_device(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                           device_states: *const RlPathState, n_states: u32, device_list: *const u32, n_list: u32,
                                           device_hits: *const RlRayHit, device_camera: *const RlCameraSample, device_sampled: *mut u8,
                                           device_samples: *mut RlLightSample) -> c_int;
    pub fn rl_plot_unit_render_samples_direct(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                              first_path_index: u64, max_segments: u32, samples: *const RlCameraSample, n: u32,
                                              results: *mut RlPathResult) -> c_int;
    pub fn rl_plot_unit_render_samples_direct_device(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64,
                                                     stream: u32, first_path_index: u64, max_segments: u32,
                                                     device_samples: *const RlCameraSample, n: u32, device_results: *mut RlPathResult) -> c_int;
    pub fn rl_plot_unit_render_direct(u: *mut RlPlotUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32,
                                      first_path_index: u64, n_paths: u64, max_segments: u32, device_results: *mut RlPathResult,
                                      stats: *mut RlDirectStats) -> c_int;
    pub fn rl_scene_render_features(scene: *const RlScene, primitive_fetch: c_int, width: u32, height: u32, seed: u64, stream: u32,
                                    first_path_index: u64, n_paths: u64, max_segments: u32, albedo: *mut RlPlotUnit,
                                    normal: *mut RlPlotUnit, aux: *mut RlPlotUnit, device_records: *mut RlFeatureSample,
                                    stats: *mut RlFeatureStats) -> c_int;

    // The edge-avoiding a-trous filter over the guides of rl_scene_render_features, gather unit to gather unit.
    pub fn rl_denoise_params_default(out: *mut RlDenoiseParams) -> c_int;
    pub fn rl_denoise_unit_create(device: c_int, width: u32, height: u32, out: *mut *mut RlDenoiseUnit) -> c_int;
    pub fn rl_denoise_unit_destroy(unit: *mut RlDenoiseUnit) -> c_int;
    pub fn rl_denoise_unit_denoise(unit: *mut RlDenoiseUnit, image: *mut RlGatherUnit, albedo: *mut RlGatherUnit, normal: *mut RlGatherUnit,
                                   aux: *mut RlGatherUnit, params: *const RlDenoiseParams, dst: *mut RlGatherUnit) -> c_int;
    // The same filter with the error unit's variance as its colour term; sigma_colour in standard deviations, default 3.0.
    // variance_out: host, width x height floats, may be null.
    pub fn rl_denoise_variance_params_default(out: *mut RlDenoiseParams) -> c_int;
    pub fn rl_denoise_unit_denoise_variance(unit: *mut RlDenoiseUnit, image: *mut RlGatherUnit, albedo: *mut RlGatherUnit, normal: *mut RlGatherUnit,
                                            aux: *mut RlGatherUnit, error: *mut RlErrorUnit, params: *const RlDenoiseParams, dst: *mut RlGatherUnit,
                                            variance_out: *mut f32) -> c_int;

    // The spectral film: photons kept by wavelength in n_nodes planes, projected into a gather unit under an n_nodes x 3 matrix.
    pub fn rl_spectral_unit_create(device: c_int, width: u32, height: u32, n_nodes: u32, out: *mut *mut RlSpectralUnit) -> c_int;
    pub fn rl_spectral_unit_destroy(unit: *mut RlSpectralUnit) -> c_int;
    pub fn rl_spectral_unit_clear(unit: *mut RlSpectralUnit) -> c_int;
    pub fn rl_spectral_unit_plot(unit: *mut RlSpectralUnit, trace_units: *const *mut RlTraceUnit, n_trace_units: u32) -> c_int;
    pub fn rl_spectral_unit_plot_photons(unit: *mut RlSpectralUnit, photons: *const RlMappedPhoton, n: u64) -> c_int;
    pub fn rl_spectral_unit_plot_photons_device(unit: *mut RlSpectralUnit, device_photons: *const RlMappedPhoton, n: u64) -> c_int;
    pub fn rl_spectral_unit_download(unit: *mut RlSpectralUnit, out: *mut f32) -> c_int;
    pub fn rl_spectral_unit_upload(unit: *mut RlSpectralUnit, input: *const f32) -> c_int;
    pub fn rl_spectral_unit_project(unit: *mut RlSpectralUnit, matrix: *const f32, dst: *mut RlGatherUnit) -> c_int;
    pub fn rl_spectral_observer_cie1931(n_nodes: u32, out: *mut f32) -> c_int;
    // Spectral glare: one taps x taps gather table per node applied to a spectral unit's film and projected in the same launch.
    pub fn rl_glare_unit_create(device: c_int, width: u32, height: u32, n_nodes: u32, taps: u32, out: *mut *mut RlGlareUnit) -> c_int;
    pub fn rl_glare_unit_destroy(unit: *mut RlGlareUnit) -> c_int;
    pub fn rl_glare_unit_set_kernels(unit: *mut RlGlareUnit, tables: *const f32) -> c_int;
    pub fn rl_glare_unit_apply(unit: *mut RlGlareUnit, film: *mut RlSpectralUnit, matrix: *const f32, dst: *mut RlGatherUnit) -> c_int;
    pub fn rl_glare_psf_veil(taps: u32, r0: f64, out: *mut f32) -> c_int;
    pub fn rl_glare_kernels_scaled(psf: *const f32, psf_taps: u32, lambda0: f64, n_nodes: u32, strength: f64, taps: u32, out: *mut f32) -> c_int;
    pub fn rl_relight_unit_create(device: c_int, width: u32, height: u32, n_nodes: u32, n_groups: u32, out: *mut *mut RlRelightUnit) -> c_int;
    pub fn rl_relight_unit_destroy(unit: *mut RlRelightUnit) -> c_int;
    pub fn rl_relight_unit_clear(unit: *mut RlRelightUnit) -> c_int;
    pub fn rl_relight_unit_set_groups(unit: *mut RlRelightUnit, groups: *const u8, n_objects: u32) -> c_int;
    pub fn rl_relight_unit_plot_results(unit: *mut RlRelightUnit, samples: *const RlCameraSample, results: *const RlPathResult, n: u64) -> c_int;
    pub fn rl_relight_unit_plot_results_device(unit: *mut RlRelightUnit, device_samples: *const RlCameraSample, device_results: *const RlPathResult, n: u64) -> c_int;
    pub fn rl_relight_unit_render(unit: *mut RlRelightUnit, scene: *const RlScene, primitive_fetch: c_int, seed: u64, stream: u32, first_path_index: u64, n_paths: u64, max_segments: u32) -> c_int;
    pub fn rl_relight_unit_download(unit: *mut RlRelightUnit, out: *mut f32) -> c_int;
    pub fn rl_relight_unit_upload(unit: *mut RlRelightUnit, input: *const f32) -> c_int;
    pub fn rl_relight_unit_mix(unit: *mut RlRelightUnit, gains: *const f32, matrix: *const f32, dst: *mut RlGatherUnit) -> c_int;
    pub fn rl_relight_gains_black_body(n_nodes: u32, kelvins_from: f32, intensity_from: f32, kelvins_to: f32, intensity_to: f32, out: *mut f32) -> c_int;

    // The noise estimate: f64 sums of Y and Y^2 / n over the plot buffers shown to the unit; the standard error per pixel and tile.
    pub fn rl_error_unit_create(device: c_int, width: u32, height: u32, out: *mut *mut RlErrorUnit) -> c_int;
    pub fn rl_error_unit_destroy(unit: *mut RlErrorUnit) -> c_int;
    pub fn rl_error_unit_clear(unit: *mut RlErrorUnit) -> c_int;
    pub fn rl_error_unit_observe(unit: *mut RlErrorUnit, plot: *mut RlPlotUnit, n_paths: u64) -> c_int;
    pub fn rl_error_unit_estimate(unit: *mut RlErrorUnit, stats: *mut RlErrorStats, se: *mut f32, tiles: *mut f64) -> c_int;
    pub fn rl_error_unit_download(unit: *mut RlErrorUnit, sum_y: *mut f64, sum_q: *mut f64, observations: *mut u64, paths: *mut u64) -> c_int;
    pub fn rl_error_unit_upload(unit: *mut RlErrorUnit, sum_y: *const f64, sum_q: *const f64, observations: u64, paths: u64) -> c_int;
    pub fn rl_robust_params_default(out: *mut RlRobustParams) -> c_int;
    pub fn rl_robust_unit_create(device: c_int, width: u32, height: u32, n_buckets: u32, out: *mut *mut RlRobustUnit) -> c_int;
    pub fn rl_robust_unit_destroy(unit: *mut RlRobustUnit) -> c_int;
    pub fn rl_robust_unit_clear(unit: *mut RlRobustUnit) -> c_int;
    pub fn rl_robust_unit_observe(unit: *mut RlRobustUnit, plot: *mut RlPlotUnit, n_paths: u64, bucket: u32) -> c_int;
    pub fn rl_robust_unit_resolve(unit: *mut RlRobustUnit, params: *const RlRobustParams, dst: *mut RlGatherUnit, stats: *mut RlRobustStats,
                                  trim: *mut u8) -> c_int;
    pub fn rl_robust_unit_estimate(unit: *mut RlRobustUnit, params: *const RlRobustParams, stats: *mut RlErrorStats, se: *mut f32,
                                   tiles: *mut f64, trim: *mut u8) -> c_int;
    pub fn rl_robust_unit_download(unit: *mut RlRobustUnit, sums: *mut f64, bucket_paths: *mut u64, observations: *mut u64) -> c_int;
    pub fn rl_robust_unit_upload(unit: *mut RlRobustUnit, sums: *const f64, bucket_paths: *const u64, observations: u64) -> c_int;
    pub fn rl_adaptive_unit_create(device: c_int, width: u32, height: u32, out: *mut *mut RlAdaptiveUnit) -> c_int;
    pub fn rl_adaptive_unit_destroy(unit: *mut RlAdaptiveUnit) -> c_int;
    pub fn rl_adaptive_unit_plan(unit: *mut RlAdaptiveUnit, importance: *const f64, uniform_share: f64, n_paths: u64,
                                 stats: *mut RlAdaptiveStats) -> c_int;
    pub fn rl_adaptive_unit_download_plan(unit: *mut RlAdaptiveUnit, counts: *mut u32, weights: *mut f32) -> c_int;
    pub fn rl_adaptive_unit_samples(unit: *mut RlAdaptiveUnit, scene: *const RlScene, seed: u64, stream: u32, first_path_index: u64,
                                    first_sample: u64, n: u32, out: *mut RlCameraSample) -> c_int;
    pub fn rl_adaptive_unit_samples_device(unit: *mut RlAdaptiveUnit, scene: *const RlScene, seed: u64, stream: u32, first_path_index: u64,
                                           first_sample: u64, n: u32, device_out: *mut RlCameraSample) -> c_int;
    pub fn rl_plot_unit_render_adaptive(plot: *mut RlPlotUnit, unit: *mut RlAdaptiveUnit, scene: *const RlScene, primitive_fetch: c_int,
                                        seed: u64, stream: u32, first_path_index: u64, max_segments: u32) -> c_int;

    pub fn rl_gather_unit_create(device: c_int, w: u32, h: u32, out: *mut *mut RlGatherUnit) -> c_int;
    pub fn rl_gather_unit_destroy(u: *mut RlGatherUnit) -> c_int;
    pub fn rl_gather_unit_accumulate(u: *mut RlGatherUnit, plot: *mut RlPlotUnit) -> c_int;
    pub fn rl_gather_unit_save(u: *mut RlGatherUnit, path: *const c_char) -> c_int;
    pub fn rl_gather_unit_load(u: *mut RlGatherUnit, path: *const c_char) -> c_int;
    pub fn rl_gather_unit_download(u: *mut RlGatherUnit, tristimulus: *mut RlVector3, compensation: *mut RlVector3) -> c_int;
    pub fn rl_gather_unit_sync(u: *mut RlGatherUnit) -> c_int;

    // The GatherUnit-time exchange between GPUs (RCCL over xGMI, bound at run time).
    pub fn rl_comm_unique_id(id: *mut u8) -> c_int;                                  // RL_COMM_ID_BYTES bytes
    pub fn rl_comm_init_rank(id: *const u8, world: c_int, rank: c_int, device: c_int, out: *mut *mut RlComm) -> c_int;
    pub fn rl_comm_init_all(devices: *const c_int, n: c_int, out: *mut *mut RlComm) -> c_int;
    pub fn rl_comm_destroy(comm: *mut RlComm) -> c_int;
    pub fn rl_comm_rank(comm: *const RlComm, rank: *mut c_int, world: *mut c_int) -> c_int;
    pub fn rl_comm_info(comm: *const RlComm, rank: *mut c_int, world: *mut c_int, rccl_version: *mut c_int, library_path: *mut c_char, path_cap: u32) -> c_int;
    pub fn rl_comm_group_start() -> c_int;
    pub fn rl_comm_group_end() -> c_int;
    pub fn rl_plot_unit_reduce(u: *mut RlPlotUnit, comm: *mut RlComm, root: c_int) -> c_int;
    pub fn rl_plot_unit_exchange_stats(u: *mut RlPlotUnit, exchanges: *mut u64, device_ms: *mut f64) -> c_int;
    pub fn rl_plot_unit_add(dst: *mut RlPlotUnit, src: *mut RlPlotUnit) -> c_int;
    pub fn rl_gather_unit_allreduce(gather: *mut RlGatherUnit, plot: *mut RlPlotUnit, comm: *mut RlComm) -> c_int;

    pub fn rl_tonemap_unit_create(device: c_int, w: u32, h: u32, out: *mut *mut RlTonemapUnit) -> c_int;
    pub fn rl_tonemap_unit_destroy(u: *mut RlTonemapUnit) -> c_int;
    pub fn rl_tonemap_unit_tonemap(u: *mut RlTonemapUnit, gather: *mut RlGatherUnit) -> c_int;
    pub fn rl_tonemap_unit_rgb(u: *mut RlTonemapUnit, out: *mut u8) -> c_int;
    pub fn rl_tonemap_unit_srgb_float(u: *mut RlTonemapUnit, out: *mut f32, max_intensity: *mut f32) -> c_int;

    // TaskScheduler over unit ids (task_scheduler.rs:91-182, 308-325) and the whole App (app.rs:48-164), for
    // hosts that do not keep the reference's own scheduler.
    pub fn rl_scheduler_create(concurrency: u32, tonemap_interval_ms: i64, out: *mut *mut RlScheduler) -> c_int;
    pub fn rl_scheduler_destroy(s: *mut RlScheduler) -> c_int;
    pub fn rl_scheduler_get_new_task(s: *mut RlScheduler, completed: *const RlTask, now_ms: i64, next: *mut RlTask) -> c_int;
    pub fn rl_scheduler_performance(s: *mut RlScheduler, mean: *mut f32, stddev: *mut f32) -> c_int;
    pub fn rl_app_run(config: *const RlAppConfig, stats: *mut RlAppStats, rgb_out: *mut u8) -> c_int;
    // rl_app_run with a stopping rule: render until the estimated relative error is below a target (NULL target: rl_app_run).
    pub fn rl_app_run_to_error(config: *const RlAppConfig, target: *const RlErrorTarget, stats: *mut RlAppStats,
                               error_stats: *mut RlAppErrorStats, rgb_out: *mut u8) -> c_int;
    pub fn rl_app_run_sampled(config: *const RlAppConfig, target: *const RlErrorTarget, sampling: *const RlWavelengthSampling,
                              stats: *mut RlAppStats, error_stats: *mut RlAppErrorStats, rgb_out: *mut u8) -> c_int;
    pub fn rl_app_error_tiles(tiles: *mut f64, capacity: u32, n_tiles: *mut u32) -> c_int;
    pub fn rl_app_error_state(sum_y: *mut f64, sum_q: *mut f64, capacity_pixels: u64, n_pixels: *mut u64, observations: *mut u64,
                              paths: *mut u64) -> c_int;

}

pub fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(rl_last_error()) }.to_string_lossy().into_owned();
        panic!("robigo_luculenta: {} ({})", msg, rc);   // the reference panics on every error (app.rs:107,163)
    }
}
