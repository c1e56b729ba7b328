"""What DenoiseUnit.denoise_variance (rl_denoise_unit_denoise_variance) costs beside DenoiseUnit.denoise, in one process.  The
built-in scene rendered with --paths paths (default 2^22) as 16 fused renders, each observed by an error unit and then accumulated,
and its three guides; then, at each size of --sizes (default 1280x720 and 1920x1080), the variance call and the plain call
alternated, five passes and each call's default sigmas.  Measured after --warmup calls of each (default 3), over --reps (default 20):
  call: the host clock around each call, which returns synchronised -- median and min-max, and the ratio of the medians, which the
  bar is about: variance call <= 1.15 x plain call;
  v0, guides, pass 0 .. 4: device time of each launch from events on dst's stream (rl_debug_denoise_variance_ms,
  rl_debug_denoise_pass_ms) -- medians, of both calls side by side.
Prints one JSON line per size.
Usage (on a GPU machine): python tools/denoise_variance_bench.py [--sizes 1280x720 1920x1080] [--reps 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

ITERATIONS = 5
BATCHES = 16
BAR = 1.15


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def measure(w, h, paths, warmup, reps):
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    trace = R.TraceUnit(0, w, h, n_photons=64)
    plots = [R.PlotUnit(i, w, h) for i in range(4)]
    image, albedo, normal, aux, dst = (R.GatherUnit(w, h) for _ in range(5))
    error = R.ErrorUnit(w, h)
    for b in range(BATCHES):
        trace.render_fused(scene, plots[0], paths // BATCHES, seed=1, stream=0, first_path_index=b * (paths // BATCHES))
        error.observe(plots[0], paths // BATCHES)
        image.accumulate(plots[0])
    scene.render_features(w, h, 1, 0, 0, paths, albedo=plots[1], normal=plots[2], aux=plots[3])
    for g, p in zip((albedo, normal, aux), plots[1:]):
        g.accumulate(p)
    for g in (image, albedo, normal, aux):
        g.sync()
    error.download()        # (drains the error unit's stream)
    unit = R.DenoiseUnit(w, h)
    guides = dict(albedo=albedo, normal=normal, aux=aux)
    calls, launches, v0 = {"variance": [], "plain": []}, {"variance": [], "plain": []}, []
    for k in range(warmup + reps):
        for name in ("variance", "plain"):
            t0 = time.perf_counter()
            if name == "variance":
                unit.denoise_variance(image, error, dst=dst, iterations=ITERATIONS, **guides)
            else:
                unit.denoise(image, dst=dst, iterations=ITERATIONS, **guides)
            t = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                calls[name].append(t)
                launches[name].append(unit.pass_ms()[:1 + ITERATIONS])
                if name == "variance":
                    v0.append(unit.variance_ms())
    out = {"size": "%dx%d" % (w, h), "paths": paths, "reps": reps, "v0_ms": spread(v0)}
    for name in ("variance", "plain"):
        ms = np.array(launches[name])
        out[name] = {"call_ms": spread(calls[name]), "guides_ms": round(float(np.median(ms[:, 0])), 4),
                     "pass_ms": [round(float(x), 4) for x in np.median(ms[:, 1:], axis=0)],
                     "passes_ms_sum_of_medians": round(float(np.median(ms[:, 1:], axis=0).sum()), 4)}
    ratio = out["variance"]["call_ms"]["median"] / out["plain"]["call_ms"]["median"]
    out.update(call_ratio=round(ratio, 4), passes_ratio=round(out["variance"]["passes_ms_sum_of_medians"] / out["plain"]["passes_ms_sum_of_medians"], 4),
               bar=BAR, bar_met=bool(ratio <= BAR))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1280x720", "1920x1080"])
    ap.add_argument("--paths", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for size in a.sizes:
        w, h = (int(x) for x in size.split("x"))
        out = measure(w, h, a.paths, a.warmup, a.reps)
        out.update(build=R.build_id())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
