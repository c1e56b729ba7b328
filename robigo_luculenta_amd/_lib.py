"""Loads librobigo_luculenta.so (the C ABI of include/robigo_luculenta.h) with ctypes.

There is no Python or CPU implementation of the hot path behind this module: if the HIP library is
missing the import fails, and if no GPU is visible every compute call raises RlError."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# RL_LIBRARY: a diagnostic build of the same library (e.g. `make -C csrc stats`); never a different implementation.
LIB_PATH = os.environ.get("RL_LIBRARY") or os.path.join(HERE, "librobigo_luculenta.so")

RL_TASK_MAX_UNITS = 256
RL_COMM_ID_BYTES = 128


class RlError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("robigo_luculenta error %d: %s" % (code, message))
        self.code = code


class RlVector3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class RlMappedPhoton(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("probability", C.c_float), ("wavelength", C.c_float)]


class RlObjectDesc(C.Structure):
    _fields_ = [("surface_kind", C.c_uint32), ("material_kind", C.c_uint32), ("v0", RlVector3), ("v1", RlVector3),
                ("f0", C.c_float), ("f1", C.c_float), ("f2", C.c_float), ("f3", C.c_float),
                ("m0", C.c_float), ("m1", C.c_float), ("m2", C.c_float)]


class RlCameraDesc(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("phi0", "phi1", "alpha0", "alpha1", "dist0", "dist1", "fov_over_pi",
                                          "focal_factor", "depth_of_field", "chromatic_abberation")]


class RlSceneDesc(C.Structure):
    _fields_ = [("n_objects", C.c_uint32), ("objects", C.c_void_p), ("camera", RlCameraDesc)]


class RlRay(C.Structure):
    _fields_ = [("origin", RlVector3), ("t_max", C.c_float), ("direction", RlVector3), ("reserved", C.c_uint32)]


class RlIntersection(C.Structure):
    _fields_ = [("position", RlVector3), ("normal", RlVector3), ("tangent", RlVector3), ("distance", C.c_float)]


class RlRayHit(C.Structure):
    _fields_ = [("isect", RlIntersection), ("object", C.c_uint32), ("reserved", C.c_uint32)]


RL_OBJECT_NONE = 0xffffffff


class RlSpectralRay(C.Structure):
    _fields_ = [("origin", RlVector3), ("wavelength", C.c_float), ("direction", RlVector3), ("reserved", C.c_uint32)]


class RlCameraSample(C.Structure):
    _fields_ = [("ray", RlSpectralRay), ("x", C.c_float), ("y", C.c_float), ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]


class RlPathResult(C.Structure):
    _fields_ = [("value", C.c_float), ("segments", C.c_uint32), ("object", C.c_uint32), ("end", C.c_uint32)]


RL_PATH_END_VOID, RL_PATH_END_EMITTER, RL_PATH_END_ROULETTE, RL_PATH_END_LIMIT, RL_PATH_END_INVALID = range(5)
RL_PATH_MAX_SEGMENTS = 4096
RL_PATH_MAX_SEGMENTS_CAP = 65536
RL_PATH_LIVE = 0xffffffff
RL_STEP_NO_ROULETTE = 1


class RlPathState(C.Structure):
    _fields_ = [("origin", RlVector3), ("wavelength", C.c_float), ("direction", RlVector3), ("intensity", C.c_float),
                ("continue_chance", C.c_float), ("segments", C.c_uint32), ("end", C.c_uint32), ("value", C.c_float),
                ("path_index", C.c_uint64), ("object", C.c_uint32), ("reserved", C.c_uint32)]


RL_LIGHT_SKIPPED, RL_LIGHT_BACKFACING, RL_LIGHT_OCCLUDED, RL_LIGHT_VISIBLE = range(4)


class RlLightSample(C.Structure):
    _fields_ = [("direction", RlVector3), ("distance", C.c_float), ("value", C.c_float), ("weight", C.c_float),
                ("emitter", C.c_uint32), ("status", C.c_uint32)]


class RlDirectStats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("light_samples", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("visible", C.c_uint64), ("endings_kept", C.c_uint64), ("endings_dropped", C.c_uint64)]


RL_FEATURE_VOID, RL_FEATURE_EMITTER, RL_FEATURE_DIFFUSE, RL_FEATURE_LIMIT = range(4)
RL_FEATURE_MAX_SEGMENTS = 64


class RlFeatureSample(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("wavelength", C.c_float), ("albedo", C.c_float), ("normal", RlVector3),
                ("depth", C.c_float), ("object", C.c_uint32), ("segments", C.c_uint32), ("kind", C.c_uint32), ("reserved", C.c_uint32)]


class RlFeatureStats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("kinds", C.c_uint64 * 4)]


RL_DENOISE_ITERATIONS = 5
RL_DENOISE_MAX_ITERATIONS = 6


class RlDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_colour", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float), ("reserved", C.c_uint32 * 3)]


RL_SPECTRAL_MAX_NODES = 401
RL_GLARE_MAX_TAPS = 65
RL_RELIGHT_MAX_GROUPS = 16
RL_RELIGHT_DROP = 0xFF
RL_ERROR_TILE = 16


RL_ROBUST_MAX_BUCKETS = 32
RL_ROBUST_NEXT = 0xFFFFFFFF


class RlRobustParams(C.Structure):
    _fields_ = [("gain", C.c_double), ("max_trim", C.c_uint32), ("reserved", C.c_uint32)]


class RlRobustStats(C.Structure):
    _fields_ = [("observations", C.c_uint64), ("paths", C.c_uint64), ("buckets", C.c_uint32), ("largest_trim", C.c_uint32),
                ("trimmed_pixels", C.c_uint64), ("trimmed_buckets", C.c_uint64), ("untrimmable_pixels", C.c_uint64)]


class RlErrorStats(C.Structure):
    _fields_ = [("observations", C.c_uint64), ("paths", C.c_uint64), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32),
                ("worst_tile_x", C.c_uint32), ("worst_tile_y", C.c_uint32), ("sum_y", C.c_double), ("sum_se", C.c_double),
                ("relative_error", C.c_double), ("worst_tile_error", C.c_double)]


class RlAdaptiveStats(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32), ("min_count", C.c_uint32),
                ("max_count", C.c_uint32), ("min_weight", C.c_float), ("max_weight", C.c_float), ("importance_sum", C.c_double)]


class RlErrorTarget(C.Structure):
    _fields_ = [("relative_error", C.c_double), ("worst_tile_error", C.c_double), ("min_observations", C.c_uint32),
                ("reserved", C.c_uint32)]


class RlWavelengthSampling(C.Structure):
    _fields_ = [("importance", C.c_void_p), ("n_nodes", C.c_uint32), ("reserved", C.c_uint32), ("uniform_share", C.c_double)]


class RlAppErrorStats(C.Structure):
    _fields_ = [("at_stop", RlErrorStats), ("at_end", RlErrorStats), ("reached", C.c_uint32), ("estimates", C.c_uint32)]


class RlTask(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("unit", C.c_uint32), ("n_units", C.c_uint32),
                ("units", C.c_uint32 * RL_TASK_MAX_UNITS)]


class RlAppConfig(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("device", C.c_int), ("concurrency", C.c_uint32),
                ("photons_per_batch", C.c_uint32), ("seed", C.c_uint64), ("stream", C.c_uint32),
                ("builtin_scene", C.c_int), ("builtin_param", C.c_int), ("max_batches", C.c_uint64),
                ("tonemap_interval_ms", C.c_int64), ("fused", C.c_int), ("output_ppm", C.c_char_p),
                ("checkpoint", C.c_char_p), ("resume", C.c_int), ("verbose", C.c_int), ("sleep_us", C.c_uint32),
                ("first_batch", C.c_uint64), ("n_devices", C.c_uint32), ("blocking_trace", C.c_int), ("devices", C.POINTER(C.c_int)), ("threads", C.c_uint32)]


class RlAppStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("paths", C.c_uint64), ("segments", C.c_uint64), ("tasks", C.c_uint64 * 5),
                ("seconds", C.c_double), ("kernel_ms", C.c_double), ("batches_per_sec_mean", C.c_float),
                ("batches_per_sec_stddev", C.c_float), ("tonemaps", C.c_uint32), ("next_batch", C.c_uint64)]


# name -> (restype, argtypes); every symbol include/robigo_luculenta.h declares.
_vp, _u8p = C.c_void_p, C.c_void_p
_i, _u32, _u64, _i64, _f = C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_float
_pp = C.POINTER(C.c_void_p)
SIGNATURES = {
    "rl_last_error": (C.c_char_p, []),
    "rl_device_count": (_i, []),
    "rl_device_pci_bus_id": (_i, [_i, C.c_char_p, _u32]),
    "rl_version": (C.c_char_p, []),
    "rl_build_id": (C.c_char_p, []),
    "rl_scene_builtin_desc": (_i, [_i, _i, _vp, _u32, C.POINTER(_u32), C.POINTER(RlCameraDesc)]),
    "rl_scene_desc_save": (_i, [C.c_char_p, C.POINTER(RlSceneDesc)]),
    "rl_scene_desc_load": (_i, [C.c_char_p, _vp, _u32, C.POINTER(_u32), C.POINTER(RlCameraDesc)]),
    "rl_scene_create": (_i, [C.POINTER(RlSceneDesc), _i, _pp]),
    "rl_scene_destroy": (_i, [_vp]),
    "rl_scene_intersect": (_i, [_vp, _i, _vp, _u32, _vp]),
    "rl_scene_intersect_device": (_i, [_vp, _i, _vp, _u32, _vp]),
    "rl_scene_occluded": (_i, [_vp, _i, _vp, _u32, _vp]),
    "rl_scene_occluded_device": (_i, [_vp, _i, _vp, _u32, _vp]),
    "rl_scene_camera_rays": (_i, [_vp, _u32, _u32, _u64, _u32, _u64, _u32, _vp]),
    "rl_scene_camera_rays_device": (_i, [_vp, _u32, _u32, _u64, _u32, _u64, _u32, _vp]),
    "rl_scene_render_rays": (_i, [_vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_scene_render_rays_device": (_i, [_vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_scene_begin_paths": (_i, [_vp, _u64, _vp, _u32, _vp]),
    "rl_scene_begin_paths_device": (_i, [_vp, _u64, _vp, _u32, _vp]),
    "rl_scene_step_paths": (_i, [_vp, _i, _u64, _u32, _u32, _vp, _u32, _vp]),
    "rl_scene_step_paths_device": (_i, [_vp, _i, _u64, _u32, _u32, _vp, _u32, _vp]),
    "rl_scene_step_path_list": (_i, [_vp, _i, _u64, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "rl_scene_step_path_list_device": (_i, [_vp, _i, _u64, _u32, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "rl_scene_emitters": (_i, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "rl_scene_light_paths": (_i, [_vp, _i, _u64, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "rl_scene_light_paths_device": (_i, [_vp, _i, _u64, _u32, _vp, _u32, _vp, _u32, _vp, _vp]),
    "rl_trace_unit_create": (_i, [_i, _u32, _u32, _u32, _u32, _pp]),
    "rl_trace_unit_destroy": (_i, [_vp]),
    "rl_trace_unit_set_fetch": (_i, [_vp, _i]),
    "rl_trace_unit_set_wavelengths": (_i, [_vp, _vp]),
    "rl_wavelength_table_create": (_i, [_i, _vp, _u32, C.c_double, _pp]),
    "rl_wavelength_table_destroy": (_i, [_vp]),
    "rl_wavelength_table_download": (_i, [_vp, _vp, _vp]),
    "rl_wavelength_importance_cie1931": (_i, [_vp]),
    "rl_trace_unit_render": (_i, [_vp, _vp, _u64, _u32, _u64]),
    "rl_trace_unit_render_begin": (_i, [_vp, _vp, _u64, _u32, _u64]),
    "rl_trace_unit_render_end": (_i, [_vp]),
    "rl_trace_unit_render_async": (_i, [_vp, _vp, _u64, _u32, _u64]),
    "rl_trace_unit_render_fused": (_i, [_vp, _vp, _vp, _u64, _u32, _u64, _u64]),
    "rl_trace_unit_render_fused_sync": (_i, [_vp, _vp, _vp, _u64, _u32, _u64, _u64]),
    "rl_trace_unit_render_fused_begin": (_i, [_vp, _vp, _vp, _u64, _u32, _u64, _u64]),
    "rl_trace_unit_sync": (_i, [_vp]),
    "rl_trace_unit_photons": (_i, [_vp, _vp]),
    "rl_trace_unit_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rl_plot_unit_create": (_i, [_i, _u32, _u32, _u32, _vp, _pp]),
    "rl_plot_unit_destroy": (_i, [_vp]),
    "rl_plot_unit_plot": (_i, [_vp, _pp, _u32]),
    "rl_plot_unit_clear": (_i, [_vp]),
    "rl_plot_unit_sync": (_i, [_vp]),
    "rl_plot_unit_reduce": (_i, [_vp, _vp, _i]),
    "rl_plot_unit_exchange_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(C.c_double)]),
    "rl_plot_unit_add": (_i, [_vp, _vp]),
    "rl_gather_unit_allreduce": (_i, [_vp, _vp, _vp]),
    "rl_comm_unique_id": (_i, [_vp]),
    "rl_comm_init_rank": (_i, [_vp, _i, _i, _i, _pp]),
    "rl_comm_init_all": (_i, [C.POINTER(_i), _i, _pp]),
    "rl_comm_destroy": (_i, [_vp]),
    "rl_comm_rank": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "rl_comm_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.c_char_p, _u32]),
    "rl_comm_group_start": (_i, []),
    "rl_comm_group_end": (_i, []),
    "rl_plot_unit_device_buffer": (_i, [_vp, _pp]),
    "rl_plot_unit_download": (_i, [_vp, _vp]),
    "rl_plot_unit_upload": (_i, [_vp, _vp]),
    "rl_plot_unit_plot_photons": (_i, [_vp, _vp, _u64]),
    "rl_plot_unit_plot_photons_device": (_i, [_vp, _vp, _u64]),
    "rl_plot_unit_render_samples": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_plot_unit_render_samples_device": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_plot_unit_light_paths": (_i, [_vp, _vp, _i, _u64, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "rl_plot_unit_light_paths_device": (_i, [_vp, _vp, _i, _u64, _u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "rl_plot_unit_render_samples_direct": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_plot_unit_render_samples_direct_device": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u32, _vp, _u32, _vp]),
    "rl_plot_unit_render_direct": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u64, _u32, _vp, C.POINTER(RlDirectStats)]),
    "rl_scene_render_features": (_i, [_vp, _i, _u32, _u32, _u64, _u32, _u64, _u64, _u32, _vp, _vp, _vp, _vp, C.POINTER(RlFeatureStats)]),
    "rl_denoise_params_default": (_i, [C.POINTER(RlDenoiseParams)]),
    "rl_denoise_unit_create": (_i, [_i, _u32, _u32, _pp]),
    "rl_denoise_unit_destroy": (_i, [_vp]),
    "rl_denoise_unit_denoise": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(RlDenoiseParams), _vp]),
    "rl_denoise_variance_params_default": (_i, [C.POINTER(RlDenoiseParams)]),
    "rl_denoise_unit_denoise_variance": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RlDenoiseParams), _vp, _vp]),
    "rl_spectral_unit_create": (_i, [_i, _u32, _u32, _u32, _pp]),
    "rl_spectral_unit_destroy": (_i, [_vp]),
    "rl_spectral_unit_clear": (_i, [_vp]),
    "rl_spectral_unit_plot": (_i, [_vp, _pp, _u32]),
    "rl_spectral_unit_plot_photons": (_i, [_vp, _vp, _u64]),
    "rl_spectral_unit_plot_photons_device": (_i, [_vp, _vp, _u64]),
    "rl_spectral_unit_download": (_i, [_vp, _vp]),
    "rl_spectral_unit_upload": (_i, [_vp, _vp]),
    "rl_spectral_unit_project": (_i, [_vp, _vp, _vp]),
    "rl_spectral_observer_cie1931": (_i, [_u32, _vp]),
    "rl_glare_unit_create": (_i, [_i, _u32, _u32, _u32, _u32, _pp]),
    "rl_glare_unit_destroy": (_i, [_vp]),
    "rl_glare_unit_set_kernels": (_i, [_vp, _vp]),
    "rl_glare_unit_apply": (_i, [_vp, _vp, _vp, _vp]),
    "rl_glare_psf_veil": (_i, [_u32, C.c_double, _vp]),
    "rl_glare_kernels_scaled": (_i, [_vp, _u32, C.c_double, _u32, C.c_double, _u32, _vp]),
    "rl_relight_unit_create": (_i, [_i, _u32, _u32, _u32, _u32, _pp]),
    "rl_relight_unit_destroy": (_i, [_vp]),
    "rl_relight_unit_clear": (_i, [_vp]),
    "rl_relight_unit_set_groups": (_i, [_vp, _u8p, _u32]),
    "rl_relight_unit_plot_results": (_i, [_vp, _vp, _vp, _u64]),
    "rl_relight_unit_plot_results_device": (_i, [_vp, _vp, _vp, _u64]),
    "rl_relight_unit_render": (_i, [_vp, _vp, _i, _u64, _u32, _u64, _u64, _u32]),
    "rl_relight_unit_download": (_i, [_vp, _vp]),
    "rl_relight_unit_upload": (_i, [_vp, _vp]),
    "rl_relight_unit_mix": (_i, [_vp, _vp, _vp, _vp]),
    "rl_relight_gains_black_body": (_i, [_u32, _f, _f, _f, _f, _vp]),
    "rl_error_unit_create": (_i, [_i, _u32, _u32, _pp]),
    "rl_error_unit_destroy": (_i, [_vp]),
    "rl_error_unit_clear": (_i, [_vp]),
    "rl_error_unit_observe": (_i, [_vp, _vp, _u64]),
    "rl_error_unit_estimate": (_i, [_vp, C.POINTER(RlErrorStats), _vp, _vp]),
    "rl_error_unit_download": (_i, [_vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "rl_error_unit_upload": (_i, [_vp, _vp, _vp, _u64, _u64]),
    "rl_robust_params_default": (_i, [C.POINTER(RlRobustParams)]),
    "rl_robust_unit_create": (_i, [_i, _u32, _u32, _u32, _pp]),
    "rl_robust_unit_destroy": (_i, [_vp]),
    "rl_robust_unit_clear": (_i, [_vp]),
    "rl_robust_unit_observe": (_i, [_vp, _vp, _u64, _u32]),
    "rl_robust_unit_resolve": (_i, [_vp, C.POINTER(RlRobustParams), _vp, C.POINTER(RlRobustStats), _vp]),
    "rl_robust_unit_estimate": (_i, [_vp, C.POINTER(RlRobustParams), C.POINTER(RlErrorStats), _vp, _vp, _vp]),
    "rl_robust_unit_download": (_i, [_vp, _vp, _vp, C.POINTER(_u64)]),
    "rl_robust_unit_upload": (_i, [_vp, _vp, _vp, _u64]),
    "rl_adaptive_unit_create": (_i, [_i, _u32, _u32, _pp]),
    "rl_adaptive_unit_destroy": (_i, [_vp]),
    "rl_adaptive_unit_plan": (_i, [_vp, _vp, C.c_double, _u64, C.POINTER(RlAdaptiveStats)]),
    "rl_adaptive_unit_download_plan": (_i, [_vp, _vp, _vp]),
    "rl_adaptive_unit_samples": (_i, [_vp, _vp, _u64, _u32, _u64, _u64, _u32, _vp]),
    "rl_adaptive_unit_samples_device": (_i, [_vp, _vp, _u64, _u32, _u64, _u64, _u32, _vp]),
    "rl_plot_unit_render_adaptive": (_i, [_vp, _vp, _vp, _i, _u64, _u32, _u64, _u32]),
    "rl_gather_unit_sync": (_i, [_vp]),
    "rl_gather_unit_create": (_i, [_i, _u32, _u32, _pp]),
    "rl_gather_unit_destroy": (_i, [_vp]),
    "rl_gather_unit_accumulate": (_i, [_vp, _vp]),
    "rl_gather_unit_save": (_i, [_vp, C.c_char_p]),
    "rl_gather_unit_load": (_i, [_vp, C.c_char_p]),
    "rl_gather_unit_download": (_i, [_vp, _vp, _vp]),
    "rl_tonemap_unit_create": (_i, [_i, _u32, _u32, _pp]),
    "rl_tonemap_unit_destroy": (_i, [_vp]),
    "rl_tonemap_unit_tonemap": (_i, [_vp, _vp]),
    "rl_tonemap_unit_rgb": (_i, [_vp, _vp]),
    "rl_tonemap_unit_srgb_float": (_i, [_vp, _vp, C.POINTER(_f)]),
    "rl_scheduler_create": (_i, [_u32, _i64, _pp]),
    "rl_scheduler_destroy": (_i, [_vp]),
    "rl_scheduler_get_new_task": (_i, [_vp, C.POINTER(RlTask), _i64, C.POINTER(RlTask)]),
    "rl_scheduler_performance": (_i, [_vp, C.POINTER(_f), C.POINTER(_f)]),
    "rl_app_run": (_i, [C.POINTER(RlAppConfig), C.POINTER(RlAppStats), _vp]),
    "rl_app_run_to_error": (_i, [C.POINTER(RlAppConfig), C.POINTER(RlErrorTarget), C.POINTER(RlAppStats), C.POINTER(RlAppErrorStats), _vp]),
    "rl_app_run_sampled": (_i, [C.POINTER(RlAppConfig), C.POINTER(RlErrorTarget), C.POINTER(RlWavelengthSampling), C.POINTER(RlAppStats),
                                C.POINTER(RlAppErrorStats), _vp]),
    "rl_app_error_tiles": (_i, [_vp, _u32, C.POINTER(_u32)]),
    "rl_app_error_state": (_i, [_vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
}
# include/robigo_luculenta_debug.h: diagnostics, not part of the drop-in boundary
DEBUG_SIGNATURES = {
    "rl_debug_math_probe": (_i, [_i, _i, _vp, _vp, _u32]),
    "rl_debug_math_sweep": (_i, [_i, _i, _u32, _u32, _i, _vp, _vp]),
    "rl_debug_app_rank_plan": (_i, [_i, _vp, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "rl_debug_batch_histogram": (_i, [_i, _vp]),
    "rl_debug_variant_launches": (_i, [_vp]),
    "rl_debug_wavelength_variant_launches": (_i, [_vp]),
    "rl_debug_query_launches": (_i, [_vp]),
    "rl_debug_occlusion_launches": (_i, [_vp]),
    "rl_debug_path_launches": (_i, [_vp]),
    "rl_debug_film_launches": (_i, [_vp]),
    "rl_debug_step_launches": (_i, [_vp]),
    "rl_debug_path_list_launches": (_i, [_vp]),
    "rl_debug_light_launches": (_i, [_vp]),
    "rl_debug_light_film_launches": (_i, [_vp]),
    "rl_debug_direct_launches": (_i, [_vp]),
    "rl_debug_feature_launches": (_i, [_vp]),
    "rl_debug_denoise_launches": (_i, [_vp]),
    "rl_debug_denoise_pass_ms": (_i, [_vp, _vp]),
    "rl_debug_denoise_variance_launches": (_i, [_vp]),
    "rl_debug_denoise_variance_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rl_debug_spectral_launches": (_i, [_vp]),
    "rl_debug_spectral_ms": (_i, [_vp, _vp]),
    "rl_debug_glare_launches": (_i, [_vp]),
    "rl_debug_glare_ms": (_i, [_vp, _vp]),
    "rl_debug_relight_launches": (_i, [_vp]),
    "rl_debug_relight_ms": (_i, [_vp, _vp]),
    "rl_debug_error_launches": (_i, [_vp]),
    "rl_debug_error_ms": (_i, [_vp, _vp]),
    "rl_debug_robust_launches": (_i, [_vp]),
    "rl_debug_robust_ms": (_i, [_vp, _vp]),
    "rl_debug_robust_estimate_launches": (_i, [C.POINTER(_u64)]),
    "rl_debug_robust_estimate_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "rl_debug_adaptive_launches": (_i, [_vp]),
    "rl_debug_adaptive_ms": (_i, [_vp, _vp]),
    "rl_debug_gather_accumulate_ms": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "rl_debug_live_resources": (_i, [_vp]),
    "rl_debug_scene_emitters": (_i, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "rl_debug_light_sample": (_i, [_vp, _u32, _u64, _u32, _vp, _vp, _u32, _vp, _vp]),
    "rl_debug_prism_probe": (_i, [_vp, _u32, _vp, _u32, _vp]),
    "rl_debug_prism_count": (_i, [_vp, C.POINTER(_u32)]),
}

if not os.path.exists(LIB_PATH):
    # Nothing is built at import time and there is no CPU implementation to fall back to.
    raise ImportError("robigo_luculenta_amd: %s is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C robigo_luculenta_amd/csrc` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)

lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


def check(rc):
    if rc != 0:
        raise RlError(rc, lib.rl_last_error().decode("utf-8", "replace"))
