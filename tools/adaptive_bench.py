"""What adaptive sampling costs.  One process on one MI355X, 1280 x 720, the demo scene, 2^24 paths per call:
  adaptive  rl_plot_unit_render_adaptive of the whole plan, under the uniform plan and under a one-hot plan (everything on the last
            tile, uniform_share 0.25): 16 chunks of 2^20 samples, three launches each (sample kernel, path kernel, splat kernel);
  baseline  what the library could already do for as many paths: rl_scene_camera_rays_device, rl_scene_render_rays_device on the
            rays, rl_plot_unit_plot_photons_device on the photons.  The copies between them (the rays out of the samples, the photons
            out of samples and results: torch, on the device) are not timed: the baseline is the sum of the three calls.
The two are alternated in one run: --reps calls (default 20) after --warmup (default 3), the host's clock around the synchronous calls,
median with min - max; and events around the three launches of the adaptive call's last chunk (rl_debug_adaptive_ms).  The bar:
adaptive <= 1.10 x baseline in the same run ("within_bar"), the spread the committed profiles show between repeats.  Per sample the
new route writes 48 + 32 B and reads 32 B of rays, writes 16 B of results and reads 16 + 4 B of them in the splat; the baseline writes
48 B, reads 32 B, writes 16 B and reads 16 B of photons.  Prints one JSON line per measurement, and appends them to --out if given.
Usage (on a GPU machine): python tools/adaptive_bench.py [--reps 20] [--out profiles/adaptive_bench.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H, SEED, STREAM = 1280, 720, 1, 0


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert R.device_count() > 0, "adaptive_bench.py needs a GPU"
    n = a.paths
    lines = []

    def report(**fields):
        fields.update(paths=n, size="%dx%d" % (W, H), reps=a.reps, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    dev = torch.device("cuda:0")
    samples = torch.empty((n, 12), dtype=torch.float32, device=dev)   # RlCameraSample
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)       # RlSpectralRay
    results = torch.empty((n, 4), dtype=torch.float32, device=dev)    # RlPathResult
    photons = torch.empty((n, 4), dtype=torch.float32, device=dev)    # RlMappedPhoton
    base_plot, plot = R.PlotUnit(0, W, H), R.PlotUnit(1, W, H)
    unit = R.AdaptiveUnit(W, H)
    one_hot = np.zeros(unit.tiles_x * unit.tiles_y)
    one_hot[-1] = 1.0
    plans = {"uniform": None, "one_hot": one_hot}

    def baseline():
        """(camera ms, paths ms, photons ms) of one round."""
        t_camera = clock(lambda: scene.camera_rays_device(W, H, SEED, STREAM, 0, samples))
        rays.copy_(samples[:, :8])
        torch.cuda.synchronize()
        t_paths = clock(lambda: scene.render_rays_device(rays, results, SEED, STREAM, 0))
        photons[:, 0:2] = samples[:, 8:10]
        photons[:, 2] = results[:, 0]
        photons[:, 3] = samples[:, 3]
        torch.cuda.synchronize()
        t_photons = clock(lambda: base_plot.plot_photons_device(photons))
        return t_camera, t_paths, t_photons

    for name, importance in plans.items():
        stats = unit.plan(importance, 0.25, n)
        base, parts, adaptive, launches = [], [], [], []
        for k in range(a.warmup + a.reps):
            b = baseline()
            t = clock(lambda: plot.render_adaptive(unit, scene, SEED, STREAM, 0))
            if k >= a.warmup:
                base.append(sum(b))
                parts.append(b)
                adaptive.append(t)
                launches.append(unit.launch_ms())
        if name == "uniform":       # the two films estimate the same image: their sums agree to the noise of 2^24 paths
            ya = float(plot.tristimulus_buffer[:, 1].astype(np.float64).sum())
            yb = float(base_plot.tristimulus_buffer[:, 1].astype(np.float64).sum())
            report(what="films", plan=name, adaptive_sum_y=round(ya, 3), baseline_sum_y=round(yb, 3), ratio=round(ya / yb, 5))
        base_plot.clear()
        plot.clear()
        parts, launches = np.array(parts), np.array(launches)
        ratio = float(np.median(adaptive)) / float(np.median(base))
        report(what="render_adaptive against the composed calls", plan=name, counts=[stats["min_count"], stats["max_count"]],
               adaptive_ms=spread(adaptive), baseline_ms=spread(base),
               baseline_calls_ms={"camera_rays": spread(parts[:, 0]), "render_rays": spread(parts[:, 1]), "plot_photons": spread(parts[:, 2])},
               last_chunk_launch_ms={"samples": spread(launches[:, 0]), "paths": spread(launches[:, 1]), "splat": spread(launches[:, 2])},
               chunks=-(-n // (1 << 20)), adaptive_over_baseline=round(ratio, 4), within_bar=bool(ratio <= 1.10))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
