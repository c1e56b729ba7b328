"""What direct light at a vertex costs: Scene.light_paths_device (rl_scene_light_paths_device) against the composition a caller
writes without it.  One process, the built-in scene, LDS fetch, device forms with everything resident: rl_scene_camera_rays_device
makes the camera rays of paths 0 .. n-1 at 1920x1080, rl_scene_begin_paths_device their states, one rl_scene_step_paths_device
with hits moves them to their first vertex.  Measured, each as the host clock around calls that end synchronised, after one
warm-up round, the candidates alternated --reps times (median and min-max):
  (a) light: rl_scene_light_paths_device over all states (the identity list);
  (b) composed: torch ops that rebuild the shadow rays from samples.direction / distance and hits.position (32-byte RlRay records
      written and read back), then rl_scene_occluded_device, then a torch multiply of state.intensity, weight and the visibility.
      It is handed the directions, distances and weights of (a): the sampling and the Planck term it would also need are not in it.
  (c) occluded: rl_scene_occluded_device alone on those rays.
Checked in the run: the statuses of (a) equal the bytes of (c) -- OCCLUDED where 1, VISIBLE where 0 -- on every cast ray.
The acceptance: (a)'s median is not above (b)'s median plus (b)'s own min-max spread.  (a) over (c) is the price of the sampling
and the Planck term.  Prints one JSON line.  Usage (on a GPU machine): python tools/light_bench.py [--paths 16777216] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H = 1920, 1080
SEED, STREAM = 1, 0


def timed(fn):
    torch.cuda.synchronize()   # (the library runs on streams of its own: torch's work must be done before it reads a tensor)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert R.device_count() > 0 and torch.cuda.is_available(), "light_bench.py needs a GPU"
    assert args.reps >= 5, "alternate the candidates at least five times"
    n, dev = args.paths, torch.device("cuda", 0)
    scene = R.Scene.builtin(R.SCENE_DEMO)

    cam = torch.empty((n, 12), dtype=torch.float32, device=dev)        # RlCameraSample
    torch.cuda.synchronize()
    scene.camera_rays_device(W, H, SEED, STREAM, 0, cam)
    rays = cam[:, :8].contiguous()                                     # RlSpectralRay
    del cam
    states = torch.empty((n, 16), dtype=torch.float32, device=dev)     # RlPathState
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)       # RlRayHit
    torch.cuda.synchronize()
    scene.begin_paths_device(rays, states, 0)
    scene.step_paths_device(states, SEED, STREAM, hits=hits)
    del rays
    samples = torch.zeros((n, 8), dtype=torch.float32, device=dev)     # RlLightSample
    shadow = torch.zeros((n, 8), dtype=torch.float32, device=dev)      # RlRay
    blocked = torch.zeros(n, dtype=torch.uint8, device=dev)
    value = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    before = R.light_launches()
    scene.light_paths_device(states, hits, samples, SEED, STREAM)
    variant = next(i for i, (a, b) in enumerate(zip(R.light_launches(), before)) if a != b)
    status = samples[:, 7].view(torch.int32)
    cast = status >= R.RL_LIGHT_OCCLUDED

    def build_rays():
        d = samples[:, 0:3]
        shadow[:, 0:3] = hits[:, 0:3] + d * 1e-5
        shadow[:, 4:7] = d
        shadow[:, 3] = torch.where(cast, (samples[:, 3] - 1e-5) * 0.9990234375, torch.zeros_like(samples[:, 3]))   # t_max 0: never blocked, not scanned

    def composed():
        build_rays()
        torch.cuda.synchronize()
        scene.occluded_device(shadow, blocked)
        torch.mul(states[:, 7] * samples[:, 5], (blocked == 0) & cast, out=value)

    candidates = {
        "light": lambda: scene.light_paths_device(states, hits, samples, SEED, STREAM),
        "composed": composed,
        "occluded": lambda: scene.occluded_device(shadow, blocked),
    }
    times = {k: [] for k in candidates}
    for rep in range(args.reps + 1):   # round 0 warms up
        for name, fn in candidates.items():
            t = timed(fn)
            if rep:
                times[name].append(t)
    # the statuses of (a) against the bytes of (c), and the composition's values against (a)'s
    torch.cuda.synchronize()
    same_status = bool(((status == R.RL_LIGHT_OCCLUDED) == ((blocked == 1) & cast)).all().item())
    same_value = bool((value == samples[:, 4]).all().item())
    assert same_status, "rl_scene_light_paths_device and rl_scene_occluded_device disagree on a shadow ray"
    shares = [round(float((status == k).sum().item()) / n, 4) for k in range(4)]

    a, b, c = summary(times["light"]), summary(times["composed"]), summary(times["occluded"])
    bar = b["median_ms"] + (b["max_ms"] - b["min_ms"])
    out = {"tool": "light_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": "lds", "variant": variant, "paths": n, "reps": args.reps,
           "status_shares": dict(zip(("skipped", "backfacing", "occluded", "visible"), shares)), "light": a, "composed": b, "occluded": c,
           "a_bar_ms": round(bar, 3), "a_within_bar": a["median_ms"] <= bar, "a_light_over_composed": round(a["median_ms"] / b["median_ms"], 4),
           "a_light_over_occluded": round(a["median_ms"] / c["median_ms"], 4), "statuses_equal_occluded_bytes": same_status,
           "composed_values_equal": same_value}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
