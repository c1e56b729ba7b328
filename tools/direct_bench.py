"""What one persistent launch saves the direct render: PlotUnit.render_direct (rl_plot_unit_render_direct) against what a caller
wrote before it existed.  One process, the built-in scene, LDS fetch, a 1280x720 plot unit, paths 0 .. n-1 of the RNG for each n of
--paths (default 2^20 and 2^24).  Measured, each as the host clock around calls that end synchronised, after one warm-up round, the
candidates alternated --reps times (median and min-max):
  (a) direct: rl_plot_unit_render_direct, no results;
  (b) loop: rl_scene_camera_rays_device into a resident buffer, then rl_plot_unit_render_samples_direct_device over it;
  (c) plain: rl_plot_unit_render_samples_device on the same samples -- no direct light; without a bar: the price of the light.
Checked in the run: the films of (a) and (b) agree by the film tests' tolerance, and (a)'s stats for paths 0 .. 2^16 - 1 equal the
counts derived from the sample statuses of the loop of public device calls (camera_rays, begin_paths, step_path_list with hits,
light_paths) over the same paths.
The acceptance: (a)'s median is not above (b)'s median plus (b)'s own min-max spread, at every size.  Prints one JSON line per size.
Usage (on a GPU machine): python tools/direct_bench.py [--paths 1048576 16777216] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H = 1280, 720
SEED, STREAM = 1, 0
SLICE = 1 << 16


def timed(fn):
    torch.cuda.synchronize()   # (the library runs on streams of its own: torch's work must be done before it reads a tensor)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts, n):
    s = {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}
    s["mpaths_per_s"] = round(n / (s["median_ms"] * 1e-3) / 1e6, 3)
    return s


def loop_counts(scene, n, dev):
    """RlDirectStats of paths 0 .. n-1 from the loop of public device calls, counted from the sample statuses."""
    n_objects = len(R.builtin_scene_desc(R.SCENE_DEMO)[0])
    is_emitter = torch.zeros(n_objects + 1, dtype=torch.bool, device=dev)     # (the last slot: RL_OBJECT_NONE, clamped)
    is_emitter[torch.from_numpy(scene.emitters().astype(np.int64)).to(dev)] = True
    cam = torch.empty((n, 12), dtype=torch.float32, device=dev)        # RlCameraSample
    torch.cuda.synchronize()
    scene.camera_rays_device(W, H, SEED, STREAM, 0, cam)
    rays = cam[:, :8].contiguous()                                     # RlSpectralRay
    states = torch.empty((n, 16), dtype=torch.float32, device=dev)     # RlPathState
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)       # RlRayHit
    samples = torch.zeros((n, 8), dtype=torch.float32, device=dev)     # RlLightSample
    lists = [torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
    sampled = torch.zeros(n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    scene.begin_paths_device(rays, states, 0)
    end, value, obj = states[:, 10].view(torch.int32), states[:, 11], states[:, 14].view(torch.int32)
    status = samples[:, 7].view(torch.int32)
    counts = dict.fromkeys(("paths", "segments", "light_samples", "shadow_rays", "visible", "endings_kept", "endings_dropped"), 0)
    counts["paths"] = n
    lst, n_list = None, n
    for segment in range(R.RL_PATH_MAX_SEGMENTS):
        if n_list == 0:
            break
        live = lists[segment & 1]
        torch.cuda.synchronize()
        n_live = scene.step_path_list_device(states, SEED, STREAM, lst, n_list, live, hits=hits)
        scene.light_paths_device(states, hits, samples, SEED, STREAM, list=lst, n_list=n_list)
        rows = torch.arange(n_list, device=dev) if lst is None else lst[:n_list].long()
        st = status[rows]
        ending = (end[rows] == R.RL_PATH_END_EMITTER) & (value[rows] != 0)
        counted = sampled[rows] & is_emitter[obj[rows].clamp(0, n_objects).long()]
        counts["segments"] += n_list
        counts["light_samples"] += int((st != R.RL_LIGHT_SKIPPED).sum().item())
        counts["shadow_rays"] += int(((st == R.RL_LIGHT_OCCLUDED) | (st == R.RL_LIGHT_VISIBLE)).sum().item())
        counts["visible"] += int((st == R.RL_LIGHT_VISIBLE).sum().item())
        counts["endings_kept"] += int((ending & ~counted).sum().item())
        counts["endings_dropped"] += int((ending & counted).sum().item())
        sampled[rows] = st != R.RL_LIGHT_SKIPPED
        lst, n_list = live, n_live
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert R.device_count() > 0 and torch.cuda.is_available(), "direct_bench.py needs a GPU"
    assert args.reps >= 5, "alternate the candidates at least five times"
    dev = torch.device("cuda", 0)
    scene = R.Scene.builtin(R.SCENE_DEMO)
    plot_a, plot_b = R.PlotUnit(0, W, H), R.PlotUnit(1, W, H)

    want = loop_counts(scene, SLICE, dev)
    got = plot_a.render_direct(scene, SEED, STREAM, 0, SLICE)
    plot_a.clear()
    assert got == want, "rl_plot_unit_render_direct's stats and the loop's counts disagree: %r against %r" % (got, want)

    for n in args.paths:
        cam = torch.empty((n, 12), dtype=torch.float32, device=dev)        # RlCameraSample: (b)'s 48 bytes per path
        torch.cuda.synchronize()
        stats = {}

        def direct():
            stats.update(plot_a.render_direct(scene, SEED, STREAM, 0, n))

        def loop():
            scene.camera_rays_device(W, H, SEED, STREAM, 0, cam)
            plot_b.render_samples_direct_device(scene, cam, SEED, STREAM, 0)

        def plain():
            plot_b.render_samples_device(scene, cam, SEED, STREAM, 0)

        candidates = {"direct": direct, "loop": loop, "plain": plain}
        times = {k: [] for k in candidates}
        for rep in range(args.reps + 1):   # round 0 warms up
            if rep == 1:                   # the check below compares one call of each onto a cleared film
                plot_a.clear(), plot_b.clear()
            for name, fn in candidates.items():
                t = timed(fn)
                if rep:
                    times[name].append(t)
                if rep == 1 and name == "loop":
                    fa, fb = plot_a.tristimulus_buffer, plot_b.tristimulus_buffer
                    films_agree = bool(np.allclose(fa, fb, rtol=2e-5, atol=1e-6 * float(np.abs(fb).max())))
                    film_gap = float(np.abs(fa - fb).max() / np.abs(fb).max())
        assert films_agree, "rl_plot_unit_render_direct's film and the loop's disagree (max gap %.3e of the image's max)" % film_gap
        a, b, c = (summary(times[k], n) for k in ("direct", "loop", "plain"))
        bar = b["median_ms"] + (b["max_ms"] - b["min_ms"])
        print(json.dumps({"tool": "direct_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": "lds", "film_size": [W, H], "paths": n,
                          "reps": args.reps, "direct": a, "loop": b, "plain": c, "a_bar_ms": round(bar, 3), "a_within_bar": a["median_ms"] <= bar,
                          "loop_over_direct": round(b["median_ms"] / a["median_ms"], 4), "direct_over_plain": round(a["median_ms"] / c["median_ms"], 4),
                          "films_agree": films_agree, "film_gap_of_max": film_gap, "stats": stats, "slice_stats_equal": got == want}), flush=True)
        del cam


if __name__ == "__main__":
    main()
