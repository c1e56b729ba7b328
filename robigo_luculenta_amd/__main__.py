"""`python -m robigo_luculenta_amd` -- the reference's main.rs (main.rs:45-67) on one MI355X: renders the
built-in scene with the App worker pool and writes output.ppm (+ buffer.raw) when the batch budget is done.
With --direct the image is rendered with direct light (PlotUnit.render_direct), batch by batch over the unit API.
With --features PREFIX the denoising guides of the same paths (Scene.render_features) are written beside the image.
With --denoise PATH as well the image is filtered over those guides on the device (DenoiseUnit.denoise) and tonemapped to PATH.
With --denoise-variance as well the filter's colour term is the noise estimate's variance (DenoiseUnit.denoise_variance): it backs off
as the image converges, which the plain filter does not.
With --spectral PATH the same paths are rendered once more into a spectral film (SpectralUnit) and the cube is saved as PATH (.npy).
With --glare PATH the same paths are rendered into a spectral film as for --spectral, a wavelength-scaled point-spread function
(--glare-psf FILE.npy, or the veil of --glare-r0) is applied to it under the CIE observer (GlareUnit.apply) and the tonemapped image written to PATH.
With --relight PATH the same paths are rendered once more into a relight film (RelightUnit), one cube per light, saved as PATH (.npy);
with --light G:KELVINS[:INTENSITY] as well light G is re-balanced in the mix and the relit image written beside the cubes, without a re-trace.
With --target-error E the run ends once the estimated relative error of the image (rl_app_run_to_error) is at most E; --batches stays
the cap.  With --error-map PATH the per-tile relative error of the last estimate is written as a grey image.
With --adaptive as well the batches are rendered over the unit API by render_adaptive_to_error: from --min-observations on, every batch's
camera samples are drawn tile by tile from the running error map (AdaptiveUnit), --uniform-share of them spread by area.
With --robust PATH every batch also goes into one of the --robust-buckets sub-films of a RobustUnit (with --direct inside its batch
loop, otherwise batch by batch over the unit API), and their Gini-trimmed median of means, fireflies removed, is tonemapped to PATH.
With --robust-target-error E as well that loop ends once the robust film's own noise estimate (RobustUnit.estimate) is at most E, with
--robust-adaptive the batches are render_robust_to_error's, drawn from that estimate's tile map, and --robust-error-map PATH writes it."""
import argparse
import os
import struct
import tempfile
import time
import zlib

from . import SCENE_DEMO, SCENE_GLASS_STRESS, app_run, app_run_to_error

TARGET_TONEMAP_INTERVAL_MS = 250   # with --target-error the stopping rule is looked at at every tonemap: four times a second


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m robigo_luculenta_amd")
    ap.add_argument("--width", type=int, default=1280)    # main.rs:47
    ap.add_argument("--height", type=int, default=720)    # main.rs:48
    ap.add_argument("--batches", type=int, default=32, help="trace tasks to run (the reference runs forever)")
    ap.add_argument("--photons-per-batch", type=int, default=64 * 1024 * 512,
                    help="paths per trace task; the reference's 524288 (trace_unit.rs:67) keeps an MI355X busy for "
                         "0.2 ms only, so the default is 64 of those")
    ap.add_argument("--concurrency", type=int, default=None, help="default 2")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--scene", choices=["demo", "glass"], default="demo")
    ap.add_argument("--unfused", action="store_true", help="keep the reference's separate Trace and Plot work")
    ap.add_argument("--output", default="output.png", help="*.png or *.ppm")  # main.rs:61
    ap.add_argument("--checkpoint", default=None, help="buffer.raw to write (and to resume from with --resume)")
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--direct", action="store_true",
                    help="render with direct light: one PlotUnit.render_direct call per batch, not the App worker pool")
    ap.add_argument("--max-segments", type=int, default=None,
                    help="with --direct or --features: segments per path (default: the library's)")
    ap.add_argument("--features", metavar="PREFIX", default=None,
                    help="after the image, write the denoising guides of the same paths: PREFIX.npz (albedo_xyz, normal, aux: raw sums), "
                         "PREFIX-normal.png and PREFIX-depth.png")
    ap.add_argument("--denoise", metavar="PATH", default=None,
                    help="with --features: filter the image over the guides (DenoiseUnit.denoise, the library's defaults) and write it, "
                         "tonemapped, to PATH (*.png or *.ppm)")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="with --denoise: the variance-guided filter (DenoiseUnit.denoise_variance, the library's defaults).  With --direct "
                         "every batch is observed by an error unit; otherwise the run must estimate (--target-error or --error-map). "
                         "Needs two batches at least")
    ap.add_argument("--spectral", metavar="PATH", default=None,
                    help="after the image, render the same paths un-fused into a spectral film (SpectralUnit.plot) and save the cube, "
                         "float32 (nodes, height, width), to PATH with numpy.save (*.npy)")
    ap.add_argument("--spectral-nodes", metavar="K", type=int, default=81,
                    help="with --spectral: nodes from 380 to 780 nm (default 81, the CIE table's own)")
    ap.add_argument("--glare", metavar="PATH", default=None,
                    help="after the image, render the same paths un-fused into a spectral film of --spectral-nodes nodes, apply a "
                         "wavelength-scaled point-spread function under the CIE observer (GlareUnit.apply) and write the tonemapped "
                         "image to PATH (*.png or *.ppm)")
    ap.add_argument("--glare-psf", metavar="FILE.npy", default=None,
                    help="with --glare: the base point-spread function, a square float array of odd side (at most 257) sampled at "
                         "pixel pitch for --glare-lambda0 (default: the veil of --glare-r0)")
    ap.add_argument("--glare-r0", metavar="PX", type=float, default=None,
                    help="with --glare: the veil 1 / (1 + d^2 / PX^2)^1.5 as the base function (default 2)")
    ap.add_argument("--glare-strength", metavar="A", type=float, default=None,
                    help="with --glare: the share of a pixel's light that the function spreads, 0 .. 1 (default 0.3)")
    ap.add_argument("--glare-taps", metavar="K", type=int, default=None,
                    help="with --glare: the side of the per-node tables, odd, 1 .. 65 (default 33)")
    ap.add_argument("--glare-lambda0", metavar="NM", type=float, default=None,
                    help="with --glare: the wavelength the base function is sampled for (default 550)")
    ap.add_argument("--relight", metavar="PATH", default=None,
                    help="after the image, render the same paths into a relight film (RelightUnit.render): one cube of --spectral-nodes "
                         "nodes per black body of the scene (relight_groups; at most 16), saved as float32 (groups, nodes, height, width) "
                         "to PATH with numpy.save (*.npy)")
    ap.add_argument("--light", metavar="G:KELVINS[:INTENSITY]", action="append", default=None,
                    help="with --relight, repeatable: give the light of group G another temperature (and intensity; default: the scene's) "
                         "and write the mix under the CIE observer, tonemapped, to PATH with its suffix replaced by .png")
    ap.add_argument("--target-error", metavar="E", type=float, default=None,
                    help="end the run once the estimated relative error of the image, sum of the pixels' standard errors over the sum "
                         "of their luminance, is at most E (looked at every %d ms); --batches stays the cap" % TARGET_TONEMAP_INTERVAL_MS)
    ap.add_argument("--min-observations", metavar="K", type=int, default=None,
                    help="with --target-error: gathered plot buffers the estimate must rest on before it may end the run (default 16)")
    ap.add_argument("--error-map", metavar="PATH", default=None,
                    help="write the per-tile relative error of the last estimate as a grey image, the worst 16 x 16 tile white, to "
                         "PATH (*.png or *.ppm); without --target-error the run estimates once at the end")
    ap.add_argument("--adaptive", action="store_true",
                    help="with --target-error: draw each batch's camera samples tile by tile from the running error map "
                         "(render_adaptive_to_error over the unit API, not the App worker pool)")
    ap.add_argument("--uniform-share", metavar="F", type=float, default=None,
                    help="with --adaptive: the share of a batch's paths spread by area, 0 < F <= 1 (default 0.25)")
    ap.add_argument("--wavelength-importance", choices=["cie"], default=None,
                    help="draw each path's wavelength by importance instead of uniformly from 380-780 nm, and weight it accordingly: "
                         "'cie' follows the sum of the CIE 1931 observer's three curves (the App modes and --spectral's re-render)")
    ap.add_argument("--wavelength-uniform-share", metavar="F", type=float, default=None,
                    help="with --wavelength-importance: the share of the density that stays uniform, 0 < F <= 1 (default 0.1)")
    ap.add_argument("--robust", metavar="PATH", default=None,
                    help="keep the batches in the buckets of a robust film (RobustUnit) as well and write its image, fireflies removed by "
                         "a Gini-trimmed median of means, to PATH (*.png or *.ppm); --output is what it is without this option")
    ap.add_argument("--robust-buckets", metavar="M", type=int, default=None,
                    help="with --robust: the number of buckets, 3 .. 32 (default 15); the batches go to them in turn")
    ap.add_argument("--robust-gain", metavar="G", type=float, default=None,
                    help="with --robust: scales the number of buckets trimmed at each end, G >= 0 (default 1; 0 trims nothing)")
    ap.add_argument("--robust-target-error", metavar="E", type=float, default=None,
                    help="with --robust: end the run once the estimated relative error of the robust film (RobustUnit.estimate, which a "
                         "trimmed firefly does not inflate) is at most E, looked at after every batch once each bucket has one; "
                         "--batches stays the cap")
    ap.add_argument("--robust-adaptive", action="store_true",
                    help="with --robust-target-error: draw each batch's camera samples tile by tile from the robust estimate's error map "
                         "(render_robust_to_error)")
    ap.add_argument("--robust-error-map", metavar="PATH", default=None,
                    help="with --robust: write the per-tile relative error of the last robust estimate as a grey image, the worst "
                         "16 x 16 tile white, to PATH (*.png or *.ppm); without --robust-target-error the run estimates once at the end")
    a = ap.parse_args(argv)
    for given, flag in ((a.robust_buckets is not None, "--robust-buckets"), (a.robust_gain is not None, "--robust-gain"),
                        (a.robust_target_error is not None, "--robust-target-error"), (a.robust_adaptive, "--robust-adaptive"),
                        (a.robust_error_map is not None, "--robust-error-map")):
        if given and a.robust is None:
            ap.error("%s needs --robust PATH" % flag)
    if a.robust_adaptive and a.robust_target_error is None:
        ap.error("--robust-adaptive needs --robust-target-error: the samples follow the estimate the target is held to")
    if a.robust_target_error is not None and not a.robust_target_error >= 0:
        ap.error("--robust-target-error must be a number >= 0")
    for given, flag in ((a.robust_target_error is not None, "--robust-target-error"), (a.robust_adaptive, "--robust-adaptive"),
                        (a.robust_error_map is not None, "--robust-error-map")):
        if given and a.direct:
            ap.error("%s cannot be combined with --direct: the robust estimate drives the camera-path batch loop" % flag)
    if a.robust_adaptive and not 0 < a.photons_per_batch < 1 << 32:
        ap.error("--robust-adaptive needs --photons-per-batch in 1 .. 2^32 - 1: a plan's size")
    if a.robust is not None:
        for given, flag in ((a.adaptive, "--adaptive"), (a.resume, "--resume"), (a.unfused, "--unfused"),
                            (a.concurrency is not None, "--concurrency"), (a.spectral is not None, "--spectral")):
            if given:
                ap.error("%s cannot be combined with --robust: the robust mode renders batch by batch over the unit API, every batch "
                         "into one bucket" % flag)
        if a.robust_buckets is None:
            a.robust_buckets = 15
        if not 3 <= a.robust_buckets <= 32:
            ap.error("--robust-buckets must be in 3 .. 32")
        if a.batches < a.robust_buckets:
            ap.error("--robust needs --batches of at least --robust-buckets (default 15): every bucket needs a batch")
        if a.robust_gain is None:
            a.robust_gain = 1.0
        if not a.robust_gain >= 0:
            ap.error("--robust-gain must be a number >= 0")
        for given, flag in ((a.target_error is not None, "--target-error"), (a.error_map is not None, "--error-map"),
                            (a.wavelength_importance is not None, "--wavelength-importance")):
            if given:
                ap.error("%s cannot be combined with --robust: that is the App worker pool's, and the robust mode renders over the "
                         "unit API" % flag)
    if a.wavelength_uniform_share is not None and a.wavelength_importance is None:
        ap.error("--wavelength-uniform-share needs --wavelength-importance")
    if a.wavelength_uniform_share is not None and not 0 < a.wavelength_uniform_share <= 1:
        ap.error("--wavelength-uniform-share must be a number in (0, 1]")
    if a.wavelength_importance is not None:
        for given, flag in ((a.direct, "--direct"), (a.adaptive, "--adaptive")):
            if given:
                ap.error("--wavelength-importance cannot be combined with %s: that renderer draws its own wavelengths" % flag)
        if a.wavelength_uniform_share is None:
            a.wavelength_uniform_share = 0.1
    if a.adaptive and a.target_error is None:
        ap.error("--adaptive needs --target-error: the samples follow the estimate the target is held to")
    if a.uniform_share is not None and not a.adaptive:
        ap.error("--uniform-share needs --adaptive")
    if a.uniform_share is not None and not 0 < a.uniform_share <= 1:
        ap.error("--uniform-share must be a number in (0, 1]")
    if a.adaptive:
        for given, flag in ((a.resume, "--resume"), (a.unfused, "--unfused"), (a.denoise_variance, "--denoise-variance"),
                            (a.concurrency is not None, "--concurrency"), (a.spectral is not None, "--spectral")):
            if given:
                ap.error("%s cannot be combined with --adaptive: the adaptive mode renders batch by batch over the unit API" % flag)
        if (a.min_observations or 16) > a.batches:
            ap.error("--adaptive needs --batches of at least --min-observations (default 16): the plans follow an estimate that rests on "
                     "that many batches")
        if not 0 < a.photons_per_batch < 1 << 32:
            ap.error("--adaptive needs --photons-per-batch in 1 .. 2^32 - 1: a plan's size")
    if a.target_error is not None and not a.target_error >= 0:
        ap.error("--target-error must be a number >= 0")
    if a.min_observations is not None and a.target_error is None:
        ap.error("--min-observations needs --target-error")
    if a.min_observations is not None and a.min_observations < 2:
        ap.error("--min-observations must be at least 2: the estimate needs two observations")
    for flag, given in (("--target-error", a.target_error is not None), ("--error-map", a.error_map is not None)):
        if given and a.direct:
            ap.error("%s cannot be combined with --direct: the estimate is made by the App worker pool" % flag)
    if a.spectral is not None and a.direct:
        ap.error("--spectral cannot be combined with --direct: the direct renderer writes no photons")
    for given, flag in ((a.glare_psf is not None, "--glare-psf"), (a.glare_r0 is not None, "--glare-r0"),
                        (a.glare_strength is not None, "--glare-strength"), (a.glare_taps is not None, "--glare-taps"),
                        (a.glare_lambda0 is not None, "--glare-lambda0")):
        if given and a.glare is None:
            ap.error("%s needs --glare PATH" % flag)
    if a.glare is not None:
        if a.direct:
            ap.error("--glare cannot be combined with --direct: the direct renderer writes no photons")
        if a.glare_psf is not None and a.glare_r0 is not None:
            ap.error("--glare-psf and --glare-r0 both name the base function: give one")
        a.glare_r0 = 2.0 if a.glare_r0 is None else a.glare_r0
        a.glare_strength = 0.3 if a.glare_strength is None else a.glare_strength
        a.glare_taps = 33 if a.glare_taps is None else a.glare_taps
        a.glare_lambda0 = 550.0 if a.glare_lambda0 is None else a.glare_lambda0
        if not 0 < a.glare_r0 < float("inf") or not 0 < a.glare_lambda0 < float("inf"):
            ap.error("--glare-r0 and --glare-lambda0 must be finite and greater than 0")
        if not 0 <= a.glare_strength <= 1:
            ap.error("--glare-strength must be in 0 .. 1")
        if not (1 <= a.glare_taps <= 65 and a.glare_taps % 2 == 1):
            ap.error("--glare-taps must be odd and in 1 .. 65")
    if a.light is not None and a.relight is None:
        ap.error("--light needs --relight PATH")
    if a.relight is not None:
        for given, flag in ((a.direct, "--direct"), (a.adaptive, "--adaptive"), (a.robust is not None, "--robust"),
                            (a.wavelength_importance is not None, "--wavelength-importance")):
            if given:
                ap.error("--relight cannot be combined with %s: the relight film re-renders the camera paths of the plain image" % flag)
        lights = []
        for text in a.light or []:
            parts = text.split(":")
            try:
                group, kelvins = int(parts[0]), float(parts[1])
                intensity = float(parts[2]) if len(parts) == 3 else None
                if len(parts) not in (2, 3) or group < 0 or not 0 < kelvins < float("inf") or (intensity is not None and not 0 < intensity < float("inf")):
                    raise ValueError(text)
            except (ValueError, IndexError):
                ap.error("--light takes G:KELVINS[:INTENSITY], G >= 0 and the numbers finite and greater than 0, not %r" % text)
            lights.append((group, kelvins, intensity))
        a.light = lights
    if a.denoise is not None and a.features is None:
        ap.error("--denoise needs --features: the filter is guided by the albedo, normal and depth films")
    if a.denoise_variance:
        if a.denoise is None:
            ap.error("--denoise-variance needs --denoise PATH: it chooses the filter that writes PATH")
        if not a.direct and a.target_error is None and a.error_map is None:
            ap.error("--denoise-variance needs --direct, --target-error or --error-map: the variance comes from a run that estimates its error")
        if a.resume:
            ap.error("--denoise-variance cannot be combined with --resume: the estimate covers this run's samples only, the image all of them")
        if a.batches < 2:
            ap.error("--denoise-variance needs at least two batches: the variance rests on two observations")
    if a.direct:
        for given, flag in ((a.unfused, "--unfused"), (a.concurrency is not None, "--concurrency"), (a.resume, "--resume")):
            if given:
                ap.error("%s cannot be combined with --direct: the direct mode makes one render_direct call per batch" % flag)
    elif a.max_segments is not None and a.features is None:
        ap.error("--max-segments needs --direct or --features")
    if a.concurrency is None:
        a.concurrency = 2
    return a


def write_image(path, rgb, width, height):
    """(height * width, 3) uint8 as binary PPM, or as PNG for a name that ends in .png."""
    data = rgb.tobytes()
    if path.lower().endswith(".png"):
        def chunk(kind, body):
            return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
        rows = b"".join(b"\x00" + data[y * width * 3:(y + 1) * width * 3] for y in range(height))
        blob = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))
    else:
        blob = b"P6\n%d %d\n255\n" % (width, height) + data
    with open(path, "wb") as f:
        f.write(blob)


def render_direct(a):
    """--direct: batch b is paths [b * photons_per_batch, (b + 1) * photons_per_batch) of stream 0, one render_direct call into a
    plot unit and one GatherUnit.accumulate each; one tonemap at the end.  With --denoise-variance an ErrorUnit observes each batch's
    plot buffer before it is gathered.  Returns (rgb, totals, the gather unit, the error unit or None)."""
    from . import ErrorUnit, GatherUnit, PlotUnit, RobustUnit, Scene, TonemapUnit
    scene = Scene.builtin(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, device=a.device)
    plot = PlotUnit(0, a.width, a.height, device=a.device)
    gather = GatherUnit(a.width, a.height, device=a.device)
    error = ErrorUnit(a.width, a.height, device=a.device) if a.denoise_variance else None
    robust = RobustUnit(a.width, a.height, a.robust_buckets, device=a.device) if a.robust is not None else None
    total = {}
    t0 = time.perf_counter()
    for b in range(a.batches):
        stats = plot.render_direct(scene, a.seed, 0, b * a.photons_per_batch, a.photons_per_batch, max_segments=a.max_segments or 0)
        if error is not None:
            error.observe(plot, a.photons_per_batch)
        if robust is not None:
            robust.observe(plot, a.photons_per_batch)
        gather.accumulate(plot)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
        if not a.quiet:
            print("batch %d: %s" % (b, ", ".join("%s %d" % kv for kv in stats.items())))
    tonemap = TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(gather)
    rgb = tonemap.rgb_buffer
    seconds = time.perf_counter() - t0
    write_image(a.output, rgb, a.width, a.height)
    if a.checkpoint:
        gather.save(a.checkpoint)
    print("direct light: %s" % ", ".join("%s %d" % kv for kv in total.items()))
    print("%d batches, %.1f Mpaths, %.1f Mrays and %.1f M shadow rays in %.2f s; wrote %s"
          % (a.batches, total.get("paths", 0) / 1e6, total.get("segments", 0) / 1e6, total.get("shadow_rays", 0) / 1e6, seconds, a.output))
    if robust is not None:
        resolve_robust(a, robust)
    return rgb, total, gather, error


def resolve_robust(a, robust):
    """--robust PATH: the robust unit that observed every batch resolved into a gather unit of its own, tonemapped as the image was,
    written to PATH; prints the stats line.  Returns (rgb, stats)."""
    from . import GatherUnit, TonemapUnit
    film = GatherUnit(a.width, a.height, device=a.device)
    stats = robust.resolve(film, gain=a.robust_gain)
    tonemap = TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(film)
    rgb = tonemap.rgb_buffer
    write_image(a.robust, rgb, a.width, a.height)
    print("robust film: %d buckets, gain %g, %d observations of %d paths; %d pixels trimmed (%d buckets, at most %d at each end), "
          "%d untrimmable; wrote %s"
          % (stats["buckets"], a.robust_gain, stats["observations"], stats["paths"], stats["trimmed_pixels"], stats["trimmed_buckets"],
             stats["largest_trim"], stats["untrimmable_pixels"], a.robust))
    return rgb, stats


def render_robust(a):
    """--robust without --direct: batch b is paths [b * photons_per_batch, (b + 1) * photons_per_batch) of stream 0, one fused
    synchronous render into a plot unit, shown to the robust unit and then gathered; one tonemap at the end, then the robust film.
    With --robust-target-error E the run ends once RobustUnit.estimate's relative_error -- the noise of the robust film, which a
    trimmed firefly does not inflate -- is at most E, looked at after every batch from the M-th on; the batches are the same fused
    renders, so --output is what --batches of that many gives without the option.  With --robust-adaptive as well the batches are
    render_robust_to_error's: every batch's camera samples follow the estimate's tile map.  With --robust-error-map PATH the last
    estimate's per-tile relative error is written as a grey image (without a target: one estimate at the end).
    Returns (rgb, the gather unit, the robust film's stats)."""
    from . import AdaptiveUnit, GatherUnit, PlotUnit, RobustUnit, Scene, TonemapUnit, TraceUnit, render_robust_to_error
    scene = Scene.builtin(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, device=a.device)
    plot = PlotUnit(0, a.width, a.height, device=a.device)
    gather = GatherUnit(a.width, a.height, device=a.device)
    robust = RobustUnit(a.width, a.height, a.robust_buckets, device=a.device)
    made, estimate, tiles = a.batches, None, None
    t0 = time.perf_counter()
    if a.robust_adaptive:
        adaptive = AdaptiveUnit(a.width, a.height, device=a.device)
        made, estimate, tiles = render_robust_to_error(scene, plot, gather, robust, adaptive, a.photons_per_batch, a.batches,
                                                       a.robust_target_error, gain=a.robust_gain, seed=a.seed)
    else:
        trace = TraceUnit(0, a.width, a.height, n_photons=64, device=a.device)
        for b in range(a.batches):
            trace.render_fused_sync(scene, plot, a.photons_per_batch, seed=a.seed, stream=0, first_path_index=b * a.photons_per_batch)
            robust.observe(plot, a.photons_per_batch)
            gather.accumulate(plot)
            if a.robust_target_error is not None and b + 1 >= a.robust_buckets:
                estimate, _, tiles = robust.estimate(a.robust_gain, se=False)
                if estimate["relative_error"] <= a.robust_target_error:
                    made = b + 1
                    break
        if estimate is None and a.robust_error_map is not None:
            estimate, _, tiles = robust.estimate(a.robust_gain, se=False)
    tonemap = TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(gather)
    rgb = tonemap.rgb_buffer
    seconds = time.perf_counter() - t0
    write_image(a.output, rgb, a.width, a.height)
    if a.checkpoint:
        gather.save(a.checkpoint)
    print("%d batches, %.1f Mpaths in %.2f s; wrote %s" % (made, made * a.photons_per_batch / 1e6, seconds, a.output))
    if estimate is not None:
        target = "no target"
        if a.robust_target_error is not None:
            target = "target %g %s" % (a.robust_target_error, "reached" if estimate["relative_error"] <= a.robust_target_error else "not reached")
        print("robust estimate: %d of %d batches, relative_error %.6g, %s" % (made, a.batches, estimate["relative_error"], target))
        if a.robust_error_map is not None:
            write_error_map(a, a.robust_error_map, tiles)
    return rgb, gather, resolve_robust(a, robust)[1]


def render_features(a):
    """--features PREFIX: batch b is paths [b * photons_per_batch, (b + 1) * photons_per_batch) of stream 0, one render_features
    call into three plot units and one GatherUnit.accumulate for each; PREFIX.npz holds the raw sums as float32 (h, w, 3) arrays,
    PREFIX-normal.png the mean normal and PREFIX-depth.png the mean depth over its maximum.  Returns the films, the totals and the three
    gather units (albedo, normal, aux), which --denoise goes on to use."""
    import numpy as np
    from . import GatherUnit, PlotUnit, Scene
    scene = Scene.builtin(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, device=a.device)
    names = ("albedo_xyz", "normal", "aux")
    plots = [PlotUnit(k, a.width, a.height, device=a.device) for k in range(3)]
    gathers = [GatherUnit(a.width, a.height, device=a.device) for _ in range(3)]
    total = {"paths": 0, "segments": 0, "kinds": [0, 0, 0, 0]}
    for b in range(a.batches):
        stats = scene.render_features(a.width, a.height, a.seed, 0, b * a.photons_per_batch, a.photons_per_batch,
                                      max_segments=a.max_segments or 0, albedo=plots[0], normal=plots[1], aux=plots[2])
        for gather, plot in zip(gathers, plots):
            gather.accumulate(plot)
        total["paths"] += stats["paths"]
        total["segments"] += stats["segments"]
        total["kinds"] = [x + y for x, y in zip(total["kinds"], stats["kinds"])]
    films = {name: gather.tristimulus_buffer.reshape(a.height, a.width, 3) for name, gather in zip(names, gathers)}
    np.savez(a.features + ".npz", **films)
    normal, aux = films["normal"].astype(np.float64), films["aux"].astype(np.float64)
    length = np.sqrt((normal * normal).sum(axis=2, keepdims=True))
    unit = np.divide(normal, length, out=np.zeros_like(normal), where=length > 0)
    write_image(a.features + "-normal.png", np.clip((unit * 0.5 + 0.5) * 255.0 + 0.5, 0, 255).astype(np.uint8).reshape(-1, 3), a.width, a.height)
    depth = np.divide(aux[:, :, 1], aux[:, :, 0], out=np.zeros(aux.shape[:2]), where=aux[:, :, 0] > 0)
    grey = np.clip(depth / (depth.max() if depth.max() > 0 else 1.0) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    write_image(a.features + "-depth.png", np.repeat(grey.reshape(-1, 1), 3, axis=1), a.width, a.height)
    print("features: paths %d, segments %d, void %d, emitter %d, diffuse %d, limit %d; wrote %s.npz"
          % ((total["paths"], total["segments"]) + tuple(total["kinds"]) + (a.features,)))
    return films, total, gathers


def spectral_film(a):
    """The batches x photons_per_batch paths of stream 0 once more, un-fused -- TraceUnit.render in runs of at most 2^22 paths,
    SpectralUnit.plot of each.  Returns the spectral unit (--spectral and --glare)."""
    from . import Scene, SpectralUnit, TraceUnit, WavelengthTable
    scene = Scene.builtin(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, device=a.device)
    film = SpectralUnit(a.width, a.height, a.spectral_nodes, device=a.device)
    table = None
    if a.wavelength_importance is not None:       # the image's paths: the same table, so the same wavelengths and weights
        table = WavelengthTable(a.wavelength_importance, a.wavelength_uniform_share, device=a.device)
    total = a.batches * a.photons_per_batch
    run = max(1, min(total, 1 << 22))
    traces = {}
    for first in range(0, total, run):
        n = min(run, total - first)
        if n not in traces:
            traces[n] = TraceUnit(0, a.width, a.height, n_photons=n, device=a.device)
            traces[n].set_wavelengths(table)
        traces[n].render(scene, seed=a.seed, stream=0, first_path_index=first)
        film.plot([traces[n]])
    return film


def render_spectral(a, film):
    """--spectral PATH: the cube of spectral_film(a) saved with numpy.save.  Returns the cube, float32 (nodes, height, width)."""
    import numpy as np
    total = a.batches * a.photons_per_batch
    cube = film.download()
    with open(a.spectral, "wb") as f:     # (numpy.save would append .npy to a name that lacks it)
        np.save(f, cube)
    print("spectral film: %d nodes, %d paths; wrote %s" % (a.spectral_nodes, total, a.spectral))
    return cube


def render_glare(a, film):
    """--glare PATH: the film of spectral_film(a) under the tables of glare_kernels_scaled -- the base function of --glare-psf or the
    veil of --glare-r0 on 2 * taps - 1 samples, so that the longest wavelength's table is still cut by the table and not by the base --
    and the CIE observer, tonemapped to PATH.  Returns the gather unit that holds the glared XYZ image."""
    import numpy as np
    from . import GatherUnit, GlareUnit, TonemapUnit, glare_kernels_scaled, glare_psf_veil, spectral_observer_cie1931
    if a.glare_psf is not None:
        psf = np.load(a.glare_psf)
    else:
        side = 2 * a.glare_taps - 1     # (the veil itself is written up to 65 taps; a wider base is the same formula in numpy)
        d = np.arange(side, dtype=np.float64) - (side - 1) // 2
        q = 1.0 + (d[None, :] ** 2 + d[:, None] ** 2) / (a.glare_r0 * a.glare_r0)
        psf = glare_psf_veil(side, a.glare_r0) if side <= 65 else (1.0 / (q * np.sqrt(q))).astype(np.float32)
    tables = glare_kernels_scaled(psf, a.glare_lambda0, a.spectral_nodes, a.glare_strength, a.glare_taps)
    glare = GlareUnit(a.width, a.height, a.spectral_nodes, a.glare_taps, device=a.device)
    glare.set_kernels(tables)
    gather, tonemap = GatherUnit(a.width, a.height, device=a.device), TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(glare.apply(film, spectral_observer_cie1931(a.spectral_nodes), gather))
    write_image(a.glare, tonemap.rgb_buffer, a.width, a.height)
    print("glare: %d taps on %d nodes, strength %g, %s at %g nm, %.3f ms; wrote %s"
          % (a.glare_taps, a.spectral_nodes, a.glare_strength, a.glare_psf or "veil r0 = %g px" % a.glare_r0, a.glare_lambda0, glare.launch_ms(),
             a.glare))
    return gather


def render_relight(a):
    """--relight PATH: the batches x photons_per_batch paths of stream 0 once more by RelightUnit.render, one group per black body
    (relight_groups), and the cubes saved with numpy.save; with --light the mix under those gains and the CIE observer, tonemapped,
    beside them.  Returns the cubes, float32 (groups, nodes, height, width)."""
    import numpy as np
    from . import (MATERIAL_BLACK_BODY, RL_RELIGHT_MAX_GROUPS, GatherUnit, RelightUnit, Scene, TonemapUnit, builtin_scene_desc,
                   relight_gains_black_body, relight_groups, spectral_observer_cie1931)
    objs, cam = builtin_scene_desc(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS)
    scene = Scene(objs, cam, device=a.device)
    lights = np.nonzero(objs["material_kind"] == MATERIAL_BLACK_BODY)[0]
    n_groups = max(1, min(len(lights), RL_RELIGHT_MAX_GROUPS))
    table = relight_groups(objs, n_groups)
    for group, _, _ in a.light:
        if group >= n_groups or not (table == group).any():
            raise SystemExit("--light %d: the scene's lights make groups 0 .. %d" % (group, min(len(lights), n_groups) - 1))
    film = RelightUnit(a.width, a.height, a.spectral_nodes, n_groups, device=a.device)
    film.set_groups(table)
    total = a.batches * a.photons_per_batch
    film.render(scene, a.seed, 0, 0, total)
    cubes = film.download()
    with open(a.relight, "wb") as f:      # (numpy.save would append .npy to a name that lacks it)
        np.save(f, cubes)
    print("relight film: %d groups of %d nodes, %d paths; wrote %s" % (n_groups, a.spectral_nodes, total, a.relight))
    if a.light:
        gains = np.ones((n_groups, a.spectral_nodes), np.float32)
        for group, kelvins, intensity in a.light:
            m = objs["m"][np.nonzero(table == group)[0][0]]     # (the first light of the group: its own kelvins and intensity)
            gains[group] = relight_gains_black_body(a.spectral_nodes, float(m[0]), float(m[1]), kelvins, float(m[1]) if intensity is None else intensity)
        gather, tonemap = GatherUnit(a.width, a.height, device=a.device), TonemapUnit(a.width, a.height, device=a.device)
        tonemap.tonemap(film.mix(gains, spectral_observer_cie1931(a.spectral_nodes), gather))
        path = os.path.splitext(a.relight)[0] + ".png"
        write_image(path, tonemap.rgb_buffer, a.width, a.height)
        print("relit: %s; wrote %s" % (", ".join("group %d at %g K" % (g, k) for g, k, _ in a.light), path))
    return cubes


def report_error(a, st, err):
    """The estimate's line, and --error-map: per tile rel = t_se / max(t_y, mean t_y) (error_tile_rel), grey = rel over the worst
    tile's, every pixel of a tile alike."""
    import numpy as np
    from . import RL_ERROR_TILE, error_tile_rel
    last = err["at_stop"] if err["reached"] else err["at_end"]
    if not err["estimates"]:
        print("no estimate: fewer than two plot buffers were gathered (%d batches)" % st["batches"])
        return None
    print("relative_error %.6g, worst tile (%d, %d) %.6g, from %d observations of %d paths; reached %d, %d of %d batches used"
          % (last["relative_error"], last["worst_tile_x"], last["worst_tile_y"], last["worst_tile_error"], last["observations"],
             last["paths"], err["reached"], st["batches"], a.batches))
    if err["reached"]:
        print("after the last gather: relative_error %.6g from %d observations" % (err["at_end"]["relative_error"], err["at_end"]["observations"]))
    if a.error_map is None:
        return None
    return write_error_map(a, a.error_map, err["tiles"])


def write_error_map(a, path, tiles):
    """An estimate's (tiles_y, tiles_x, 2) tile pairs as a grey image at `path`: per tile rel = t_se / max(t_y, mean t_y)
    (error_tile_rel), grey = rel over the worst tile's, every pixel of a tile alike."""
    import numpy as np
    from . import RL_ERROR_TILE, error_tile_rel
    rel = error_tile_rel(tiles)
    finite = rel[np.isfinite(rel)]
    worst = float(finite.max()) if finite.size and finite.max() > 0 else 1.0
    grey = np.clip(np.where(np.isfinite(rel), rel, worst) / worst * 255.0 + 0.5, 0, 255).astype(np.uint8)
    grey = np.repeat(np.repeat(grey, RL_ERROR_TILE, axis=0), RL_ERROR_TILE, axis=1)[:a.height, :a.width]
    write_image(path, np.repeat(grey.reshape(-1, 1), 3, axis=1), a.width, a.height)
    print("error map: wrote %s" % path)
    return grey


def render_adaptive(a):
    """--adaptive: render_adaptive_to_error over units of its own; batch b is paths [b * photons_per_batch, (b + 1) * photons_per_batch)
    of stream 0.  One tonemap at the end.  Returns (rgb, batches made, the last estimate's stats, the gather unit)."""
    from . import AdaptiveUnit, ErrorUnit, GatherUnit, PlotUnit, Scene, TonemapUnit, render_adaptive_to_error
    scene = Scene.builtin(SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, device=a.device)
    plot = PlotUnit(0, a.width, a.height, device=a.device)
    gather = GatherUnit(a.width, a.height, device=a.device)
    error = ErrorUnit(a.width, a.height, device=a.device)
    adaptive = AdaptiveUnit(a.width, a.height, device=a.device)
    t0 = time.perf_counter()
    batches, stats, tiles = render_adaptive_to_error(scene, plot, gather, error, adaptive, a.photons_per_batch, a.batches, a.target_error,
                                                     uniform_share=a.uniform_share or 0.25, min_observations=a.min_observations or 16,
                                                     seed=a.seed)
    tonemap = TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(gather)
    rgb = tonemap.rgb_buffer
    seconds = time.perf_counter() - t0
    write_image(a.output, rgb, a.width, a.height)
    if a.checkpoint:
        gather.save(a.checkpoint)
    reached = stats is not None and stats["relative_error"] <= a.target_error
    err = {"at_stop": stats, "at_end": stats, "reached": int(reached), "estimates": int(stats is not None), "tiles": tiles}
    report_error(a, {"batches": batches}, err)
    print("adaptive: %d of %d batches, %.1f Mpaths in %.2f s, target %s; wrote %s"
          % (batches, a.batches, batches * a.photons_per_batch / 1e6, seconds, "reached" if reached else "not reached", a.output))
    return rgb, batches, stats, gather


def denoise(a, image, guides, error=None):
    """--denoise PATH: gather unit `image` filtered over the three guide gather units into a gather unit of its own, tonemapped as
    the image was, written to PATH.  With --denoise-variance `error` is the ErrorUnit that observed what `image` gathered."""
    from . import DenoiseUnit, GatherUnit, TonemapUnit
    clean = GatherUnit(a.width, a.height, device=a.device)
    unit = DenoiseUnit(a.width, a.height, device=a.device)
    if a.denoise_variance:
        unit.denoise_variance(image, error, albedo=guides[0], normal=guides[1], aux=guides[2], dst=clean)
    else:
        unit.denoise(image, albedo=guides[0], normal=guides[1], aux=guides[2], dst=clean)
    tonemap = TonemapUnit(a.width, a.height, device=a.device)
    tonemap.tonemap(clean)
    rgb = tonemap.rgb_buffer
    write_image(a.denoise, rgb, a.width, a.height)
    print("denoised%s: wrote %s" % (" with the variance term" if a.denoise_variance else "", a.denoise))
    return rgb


def main(argv=None):
    a = parse_args(argv)
    print("rendering %d batches at %dx%d" % (a.batches, a.width, a.height))
    if a.direct:
        image, error = render_direct(a)[2:]
        if a.features is not None:
            guides = render_features(a)[2]
            if a.denoise is not None:
                denoise(a, image, guides, error)
        return
    if a.adaptive or a.robust is not None:
        image = render_adaptive(a)[3] if a.adaptive else render_robust(a)[1]
        if a.features is not None:
            guides = render_features(a)[2]
            if a.denoise is not None:
                denoise(a, image, guides)
        return
    # rl_app_run hands out no gather unit: --denoise reads the image back from the checkpoint, a temporary one if none was asked for
    scratch = tempfile.TemporaryDirectory() if a.denoise is not None and a.checkpoint is None else None
    checkpoint = os.path.join(scratch.name, "buffer.raw") if scratch else a.checkpoint
    common = dict(concurrency=a.concurrency, device=a.device, seed=a.seed, photons_per_batch=a.photons_per_batch,
                  scene=SCENE_DEMO if a.scene == "demo" else SCENE_GLASS_STRESS, fused=not a.unfused,
                  output_ppm=a.output, checkpoint=checkpoint, resume=a.resume, verbose=not a.quiet)
    if a.wavelength_importance is not None:
        common.update(wavelength_importance=a.wavelength_importance, wavelength_uniform_share=a.wavelength_uniform_share)
    if a.target_error is not None or a.error_map is not None:
        # without a target the rule is 0, which no noisy render meets: the run goes to the cap and estimates at its end
        rgb, st, err = app_run_to_error(a.width, a.height, a.batches, target_error=a.target_error or 0.0,
                                        min_observations=a.min_observations or 0,
                                        tonemap_interval_ms=TARGET_TONEMAP_INTERVAL_MS if a.target_error is not None else 30000, **common)
        report_error(a, st, err)
    else:
        rgb, st = app_run(a.width, a.height, a.batches, **common)
    print("%d trace tasks, %.1f Mpaths, %.1f Mrays in %.2f s (%.1f Mrays/s, %.1f reference batches/sec); wrote %s"
          % (st["batches"], st["paths"] / 1e6, st["segments"] / 1e6, st["seconds"], st["segments"] / st["seconds"] / 1e6,
             st["paths"] / 524288.0 / st["seconds"], a.output))
    if a.features is not None:
        guides = render_features(a)[2]
        if a.denoise is not None:
            from . import GatherUnit
            image = GatherUnit(a.width, a.height, device=a.device)
            image.load(checkpoint)
            error = None
            if a.denoise_variance:
                # the App's error unit dies with the run: its state goes into one of our own
                from . import ErrorUnit, app_error_state
                s, q, k, n = app_error_state()
                if k < 2:
                    raise SystemExit("--denoise-variance: the run gathered %d plot buffers and the variance needs two observations; "
                                     "%s was not written (more --batches, or a lower --concurrency)" % (k, a.denoise))
                error = ErrorUnit(a.width, a.height, device=a.device)
                error.upload(s, q, k, n)
            denoise(a, image, guides, error)
    if a.spectral is not None or a.glare is not None:
        film = spectral_film(a)
        if a.spectral is not None:
            render_spectral(a, film)
        if a.glare is not None:
            render_glare(a, film)
    if a.relight is not None:
        render_relight(a)
    if scratch:
        scratch.cleanup()


if __name__ == "__main__":
    main()
