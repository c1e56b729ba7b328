"""What DenoiseUnit.denoise (rl_denoise_unit_denoise) costs, pass by pass.  One process, the built-in scene rendered with --paths
paths (default 2^22) into the image and the three guides, then the denoise call with five passes and the default sigmas at each
size of --sizes (default 1280x720 and 1920x1080).  Measured after --warmup calls (default 3), over --reps calls (default 20):
  call: the host clock around the call, which returns synchronised -- median and min-max;
  guides, pass 0 .. 4: device time of each launch from events on dst's stream (rl_debug_denoise_pass_ms) -- median and min-max;
  effective GB/s of each pass: the bytes it cannot avoid -- C_i read (12), the guide record read (32), C_{i+1} written (12) per
  pixel -- over the pass's median time, beside the 8000 GB/s of HBM that bench.py's roofline uses.  A pass well below that figure
  is not memory-bound: its time goes to the 25 taps' arithmetic.
The library under test is the one RL_LIBRARY names (robigo_luculenta_amd/_lib.py), so an alternative build made with
tools/build_alt.sh is measured by the same tool; --label names it in the output.  Prints one JSON line per size.
Usage (on a GPU machine): python tools/denoise_bench.py [--sizes 1280x720 1920x1080] [--reps 20] [--label NAME]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

HBM_GBS = 8000.0        # bench.py: roofline["hbm"]["peak"]
PASS_BYTES = 12 + 32 + 12
ITERATIONS = 5


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def measure(w, h, paths, warmup, reps):
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    trace = R.TraceUnit(0, w, h, n_photons=64)
    plots = [R.PlotUnit(i, w, h) for i in range(4)]
    image, albedo, normal, aux, dst = (R.GatherUnit(w, h) for _ in range(5))
    trace.render_fused(scene, plots[0], paths, seed=1, stream=0, first_path_index=0)
    scene.render_features(w, h, 1, 0, 0, paths, albedo=plots[1], normal=plots[2], aux=plots[3])
    for g, p in zip((image, albedo, normal, aux), plots):
        g.accumulate(p)
        g.sync()
    unit = R.DenoiseUnit(w, h)
    calls, launches = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        unit.denoise(image, albedo=albedo, normal=normal, aux=aux, dst=dst, iterations=ITERATIONS)
        t = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            calls.append(t)
            launches.append(unit.pass_ms()[:1 + ITERATIONS])
    launches = np.array(launches)
    live = float((aux.tristimulus_buffer[:, 0] > 0).mean())
    out = {"size": "%dx%d" % (w, h), "paths": paths, "live_share": round(live, 4), "reps": reps, "call_ms": spread(calls), "guides_ms": spread(launches[:, 0])}
    for i in range(ITERATIONS):
        s = spread(launches[:, 1 + i])
        s["effective_gbs"] = round(PASS_BYTES * w * h / (s["median"] * 1e-3) / 1e9, 1)
        s["share_of_hbm"] = round(s["effective_gbs"] / HBM_GBS, 4)
        out["pass%d_ms" % i] = s
    out["passes_ms_sum_of_medians"] = round(float(np.median(launches[:, 1:], axis=0).sum()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1280x720", "1920x1080"])
    ap.add_argument("--paths", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="library")
    a = ap.parse_args()
    for size in a.sizes:
        w, h = (int(x) for x in size.split("x"))
        out = measure(w, h, a.paths, a.warmup, a.reps)
        out.update(label=a.label, build=R.build_id(), hbm_gbs=HBM_GBS)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
