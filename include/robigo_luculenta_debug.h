/* robigo_luculenta_debug.h -- diagnostics of librobigo_luculenta.so.  NOT part of the drop-in boundary
 * (include/robigo_luculenta.h): nothing here replaces a reference interface, a host never needs it, and the
 * Rust binding (bindings/rust/ffi.rs) does not declare it.  Used by tests/, tools/ and the profiling scripts. */
#ifndef ROBIGO_LUCULENTA_DEBUG_H
#define ROBIGO_LUCULENTA_DEBUG_H
#include "robigo_luculenta.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Evaluates the shared numerics header (csrc/rl_math.h) on the GPU so a test can check that the hipcc and
 * g++ builds agree bit-for-bit.  fn: 0 sin, 1 cos, 2 tan, 3 exp, 4 ln, 5 acos, 6 SF10 index of refraction
 * (material.rs:203-213), 7 sqrt, 8 x[i] / x[i+1 mod n], 9 x^(1/2.4) (srgb.rs:24), 10 the Russian-roulette
 * decision (trace_unit.rs:122-125) for the triples (x[i], x[m+i], x[2m+i]) = (rand, continue_chance,
 * intensity), i < m = n / 3, result 1 or 0 in y[i], 11 vector3.rs:56-67 normalise of the triples (x[i], x[m+i], x[2m+i])
 * into (y[i], y[m+i], y[2m+i]). */
int rl_debug_math_probe(int device, int fn, const float* x, float* y, uint32_t n);
/* The short square root / reciprocal / division by 200 of csrc/rl_math.h and rl_core.h (fn 16, 17, 18 of rl_debug_math_probe)
 * against the compiler's correctly rounded expansions, ON THE DEVICE, for every float whose bits lie in [lo_bits, hi_bits) -- and
 * its negative when both_signs != 0.  counts[0] = arguments whose results differ, counts[1] = arguments compared, *example = the
 * bits of one argument that differs.  Seconds for the whole normal range: the exhaustive checks of the -m gpu suite. */
int rl_debug_math_sweep(int device, int fn, uint32_t lo_bits, uint32_t hi_bits, int both_signs, uint64_t* counts, uint32_t* example);
/* The rank bookkeeping of rl_app_run for RlAppConfig{device, devices, n_devices} -- which device each rank renders on (its RNG
 * stream is config.stream + rank), the first rank on the same device (ranks sharing a GPU are added onto it), the rank's place in
 * the RCCL communicator (one per DISTINCT device in order of first appearance, so rank 0 is the root; -1: none) and the
 * communicator's size (0: a run on one device needs none).  Host arithmetic only: callable without a GPU.  Arrays of
 * max(n_devices, 1) entries. */
int rl_debug_app_rank_plan(int device, const int* devices, uint32_t n_devices, int* rank_device, int* leader, int* comm_rank,
                           uint32_t* n_communicator_ranks);
/* Blocking render calls share launches (see rl_trace_unit_render).  out[k], k = 1..256: launches on `device` that
 * carried k calls since the library was loaded (257 counters, out[0] unused).  Waits for running ones to end. */
int rl_debug_batch_histogram(int device, uint64_t* out);
/* out[v], v = 0..23: launches of instantiation v of the trace kernel since the library was loaded.  v < 16: v = 8 * (the whole
 * scene staged in LDS) + 4 * (trace fused with the splat) + 2 * (open launch: a blocking render call) + 1 * (prisms carry a
 * second bound); v = 16 + the low three bits: the variants that stage the scene's tables only (a scene too large for LDS).
 * The parity matrix (tests/test_gpu_parity.py) asserts with it that the variant it means to test is the one that ran. */
int rl_debug_variant_launches(uint64_t* out);
/* The same for the instantiations that draw the wavelength from a table (a unit after rl_trace_unit_set_wavelengths), indexed as
 * rl_debug_variant_launches is; that one does not count them. */
int rl_debug_wavelength_variant_launches(uint64_t out[24]);
/* out[v], v = 0..5: launches of instantiation v of the query kernel (rl_scene_intersect*) since the library was loaded;
 * v = 2 * stage + (prisms carry a second bound), stage 0: nothing staged in LDS, 1: the scene's tables, 2: the whole scene. */
int rl_debug_query_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the occlusion kernel (rl_scene_occluded*) since the library was loaded, indexed
 * as rl_debug_query_launches is. */
int rl_debug_occlusion_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the path kernel (rl_scene_render_rays*) since the library was loaded, indexed
 * as rl_debug_query_launches is. */
int rl_debug_path_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the film path kernel (rl_plot_unit_render_samples*) since the library was
 * loaded, indexed as rl_debug_query_launches is. */
int rl_debug_film_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the step kernel (rl_scene_step_paths*) since the library was loaded, indexed
 * as rl_debug_query_launches is. */
int rl_debug_step_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the list-step kernel (rl_scene_step_path_list*) since the library was loaded,
 * indexed as rl_debug_query_launches is. */
int rl_debug_path_list_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the light kernel (rl_scene_light_paths*) since the library was loaded, indexed
 * as rl_debug_query_launches is. */
int rl_debug_light_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the light kernel with a film (rl_plot_unit_light_paths*,
 * rl_plot_unit_render_samples_direct*) since the library was loaded, indexed as rl_debug_query_launches is. */
int rl_debug_light_film_launches(uint64_t* out);
/* out[v], v = 0..5: launches of instantiation v of the direct path kernel (rl_plot_unit_render_direct) since the library was
 * loaded, indexed as rl_debug_query_launches is. */
int rl_debug_direct_launches(uint64_t out[6]);
/* out[v], v = 0..5: launches of instantiation v of the feature path kernel (rl_scene_render_features) since the library was
 * loaded, indexed as rl_debug_query_launches is. */
int rl_debug_feature_launches(uint64_t out[6]);
/* out[0]: launches of rl_denoise_guides_kernel, out[1]: launches of rl_denoise_pass_kernel (rl_denoise_unit_denoise: one and
 * `iterations` per call) since the library was loaded. */
int rl_debug_denoise_launches(uint64_t out[2]);
/* Device time of the unit's last completed rl_denoise_unit_denoise call, from events on dst's stream, in milliseconds: out[0] the
 * guide launch, out[1 + i] pass i; 0 for passes the call did not make (all 0 before the first call).  tools/denoise_bench.py. */
int rl_debug_denoise_pass_ms(RlDenoiseUnit* unit, float out[1 + RL_DENOISE_MAX_ITERATIONS]);
/* out[0]: launches of the V_0 kernel (rl_variance_denoise_kernel), out[1]: launches of the variance form of the pass kernel
 * (rl_variance_denoise_pass_kernel) since the library was loaded: rl_denoise_unit_denoise_variance adds (1, iterations).  Its guide
 * launch counts in rl_debug_denoise_launches' out[0]; its passes do not count in out[1] there. */
int rl_debug_denoise_variance_launches(uint64_t out[2]);
/* Device time of the V_0 launch of the unit's last completed rl_denoise_unit_denoise_variance call, in milliseconds (0 before the
 * first); that call's guide launch and passes are read with rl_debug_denoise_pass_ms.  tools/denoise_variance_bench.py. */
int rl_debug_denoise_variance_ms(RlDenoiseUnit* unit, float* ms);
/* out[0]: launches of rl_spectral_photons_kernel (one per trace unit of rl_spectral_unit_plot, one per chunk of
 * rl_spectral_unit_plot_photons, one per rl_spectral_unit_plot_photons_device), out[1]: launches of rl_spectral_project_kernel (one
 * per rl_spectral_unit_project) since the library was loaded. */
int rl_debug_spectral_launches(uint64_t out[2]);
/* Device time in milliseconds, from events around the launch: out[0] the last splat launch of the unit's last completed splat call
 * (rl_spectral_unit_plot, _plot_photons, _plot_photons_device), out[1] the projection launch of its last completed
 * rl_spectral_unit_project; 0 before the first.  tools/spectral_bench.py. */
int rl_debug_spectral_ms(RlSpectralUnit* unit, float out[2]);
/* Launches of rl_glare_kernel (one per rl_glare_unit_apply, either form of the kernel) since the library was loaded. */
int rl_debug_glare_launches(uint64_t* out);
/* Device time in milliseconds, from events around the launch, of the unit's last completed rl_glare_unit_apply; 0 before the
 * first.  tools/glare_bench.py. */
int rl_debug_glare_ms(RlGlareUnit* unit, float* ms);
/* out[0]: launches of rl_relight_splat_kernel (one per chunk of rl_relight_unit_plot_results and of rl_relight_unit_render, one per
 * rl_relight_unit_plot_results_device), out[1]: path kernel launches made by rl_relight_unit_render (one per chunk; counted in
 * rl_debug_path_launches too), out[2]: launches of the mix (rl_spectral_project_kernel on the composed matrix, one per
 * rl_relight_unit_mix; not counted in rl_debug_spectral_launches), since the library was loaded. */
int rl_debug_relight_launches(uint64_t out[3]);
/* Device time in milliseconds, from events around the launch: out[0] the last splat launch of the unit's last completed splat or
 * render call, out[1] the path launch of the last chunk of its last completed rl_relight_unit_render, out[2] the mix launch of
 * its last completed rl_relight_unit_mix; 0 before the first.  tools/relight_bench.py. */
int rl_debug_relight_ms(RlRelightUnit* unit, float out[3]);
/* out[0]: launches of rl_error_observe_kernel (one per rl_error_unit_observe), out[1]: launches of rl_error_estimate_kernel (one per
 * rl_error_unit_estimate) since the library was loaded. */
int rl_debug_error_launches(uint64_t out[2]);
/* Device time in milliseconds, from events around the launch: out[0] the unit's last observe launch, out[1] its last estimate
 * launch; 0 before the first.  Waits for the launch.  tools/error_bench.py. */
int rl_debug_error_ms(RlErrorUnit* unit, float out[2]);
/* out[0]: launches of rl_robust_observe_kernel (one per rl_robust_unit_observe), out[1]: launches of rl_robust_resolve_kernel (one per
 * rl_robust_unit_resolve) since the library was loaded. */
int rl_debug_robust_launches(uint64_t out[2]);
/* Device time in milliseconds, from events around the launch: out[0] the unit's last observe launch, out[1] the resolve launch of
 * its last completed rl_robust_unit_resolve; 0 before the first.  Waits for the launch.  tools/robust_bench.py. */
int rl_debug_robust_ms(RlRobustUnit* unit, float out[2]);
/* Launches of rl_robust_estimate_kernel (one per rl_robust_unit_estimate) since the library was loaded.  A counter of its own:
 * rl_debug_robust_launches keeps its two elements. */
int rl_debug_robust_estimate_launches(uint64_t* out);
/* Device time in milliseconds, from events around the launch, of the unit's last estimate launch; 0 before the first.  Waits for
 * the launch.  tools/robust_error_bench.py. */
int rl_debug_robust_estimate_ms(RlRobustUnit* unit, float* out);
/* out[0]: launches of rl_adaptive_samples_kernel (one per chunk of rl_adaptive_unit_samples* and of rl_plot_unit_render_adaptive),
 * out[1]: path kernel launches made by rl_plot_unit_render_adaptive (counted in rl_debug_path_launches too), out[2]: launches of
 * rl_adaptive_splat_kernel, since the library was loaded. */
int rl_debug_adaptive_launches(uint64_t out[3]);
/* Device time in milliseconds, from events around the launches of the last chunk of the unit's last completed
 * rl_plot_unit_render_adaptive: out[0] the sample kernel, out[1] the path kernel, out[2] the splat kernel; 0 before the first. */
int rl_debug_adaptive_ms(RlAdaptiveUnit* unit, float out[3]);
/* rl_gather_unit_accumulate(unit, plot) between two events on the gather unit's stream, with both units' streams drained before
 * and the gather unit's after: *ms is the device time of that call's rl_gather_kernel launch, the yardstick tools/error_bench.py
 * holds the observe kernel to.  The accumulation happens as usual. */
int rl_debug_gather_accumulate_ms(RlGatherUnit* unit, RlPlotUnit* plot, float* ms);
/* What the live handles of this process hold on their devices, all devices together: out[0] device allocations, out[1] streams,
 * out[2] plain (untimed) events, out[3] timed event pairs, spare and unread ones included.  Counted where a handle acquires and
 * releases them, so a *_destroy that frees exactly what its *_create took -- and whatever the handle's calls added -- returns all
 * four to their earlier values.  Scenes and the trace, plot, gather, tonemap, denoise, spectral and error units are counted; the
 * per-device open-launch slots and query contexts, which live as long as the process, and communicators are not. */
int rl_debug_live_resources(uint64_t out[4]);
/* rl_scene_emitters for a description instead of a scene: the sampleable emitters' object indices in scan order, by the function
 * rl_scene_create builds a scene's table with.  Host arithmetic only: callable without a GPU.  The same capacity protocol. */
int rl_debug_scene_emitters(const RlObjectDesc* objects, uint32_t n_objects, uint32_t* out, uint32_t cap, uint32_t* n_emitters);
/* The HOST compile of the sampling function behind rl_scene_light_paths (csrc/rl_core.h: rl_light_sample, the function the
 * kernel calls) for n (state, hit) pairs and the emitter table of a description, under (seed, stream); no device.  samples[i] is
 * what the call writes for states[i], hits[i] when the shadow ray is not blocked: RL_LIGHT_VISIBLE with its value wherever a ray
 * is cast.  rays (may be NULL) receives that ray -- the RlRay rl_scene_occluded decides -- and an all-zero record where none is
 * cast. */
int rl_debug_light_sample(const RlObjectDesc* objects, uint32_t n_objects, uint64_t seed, uint32_t stream, const RlPathState* states,
                          const RlRayHit* hits, uint32_t n, RlLightSample* samples, RlRay* rays);
/* The prism shortcut (csrc/rl_core.h: rl_hex_prism_fast) against the Compound tree it stands in for
 * (geometry.rs:380-407), both evaluated ON THE GPU -- with the hardware's v_rcp_f32 -- for n rays against prism
 * `prism` (0-based, in the scene's flattened order) of `scene`.  rays: n x {origin.xyz, direction.xyz}.
 * out: n x {status (0 miss, 1 hit, 2 undecided), t bits and half-space of the shortcut, t bits (or 0xffffffff for
 * "no hit") and half-space of the tree} as 5 uint32 each. */
int rl_debug_prism_probe(const RlScene* scene, uint32_t prism, const float* rays, uint32_t n, uint32_t* out);
/* Number of prism records of the scene's flattened form (padding prisms of the cull groups included). */
int rl_debug_prism_count(const RlScene* scene, uint32_t* n_prisms);

#ifdef __cplusplus
}
#endif
#endif /* ROBIGO_LUCULENTA_DEBUG_H */
