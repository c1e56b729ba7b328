"""What the film in the light kernel saves: PlotUnit.light_paths_device (rl_plot_unit_light_paths_device) against the composition
a caller wrote before it existed.  One process, the built-in scene, LDS fetch, device forms with everything resident, a 1280x720
plot unit: rl_scene_camera_rays_device makes the camera samples of paths 0 .. n-1, rl_scene_begin_paths_device their states, one
rl_scene_step_paths_device with hits moves them to their first vertex (so some have ended on a light and most stand on a vertex);
`sampled` holds ones, so the drop rule is at work.  Measured, each as the host clock around calls that end synchronised, after one
warm-up round, the candidates alternated --reps times (median and min-max):
  (a) film: rl_plot_unit_light_paths_device over all states (the identity list), no sample records;
  (b) composed: rl_scene_light_paths_device, then torch ops that build the 16-byte photon records from the samples, the states and
      the camera samples with the drop rule (a byte per object says which are sampleable emitters) and write the new `sampled`
      bytes, then rl_plot_unit_plot_photons_device.
Checked in the run: the two films agree by the film tests' bar, and so do the bytes.
The acceptance: (a)'s median is not above (b)'s median plus (b)'s own min-max spread.
Also printed, without a bar: Msamples/s of render_samples_direct_device against render_samples_device on --render camera samples:
the price of the direct light.  Prints one JSON line.
Usage (on a GPU machine): python tools/light_film_bench.py [--paths 1048576] [--reps 5] [--render 1048576]"""
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
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--render", type=int, default=1 << 20)
    args = ap.parse_args()
    assert R.device_count() > 0 and torch.cuda.is_available(), "light_film_bench.py needs a GPU"
    assert args.reps >= 5, "alternate the candidates at least five times"
    n, dev = args.paths, torch.device("cuda", 0)
    scene = R.Scene.builtin(R.SCENE_DEMO)
    n_objects = len(R.builtin_scene_desc(R.SCENE_DEMO)[0])
    is_emitter = torch.zeros(n_objects + 1, dtype=torch.bool, device=dev)     # (the last slot: RL_OBJECT_NONE, clamped)
    is_emitter[torch.from_numpy(scene.emitters().astype(np.int64)).to(dev)] = True

    cam = torch.empty((n, 12), dtype=torch.float32, device=dev)        # RlCameraSample
    torch.cuda.synchronize()
    scene.camera_rays_device(W, H, SEED, STREAM, 0, cam)
    rays = cam[:, :8].contiguous()                                     # RlSpectralRay
    states = torch.empty((n, 16), dtype=torch.float32, device=dev)     # RlPathState
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)       # RlRayHit
    torch.cuda.synchronize()
    scene.begin_paths_device(rays, states, 0)
    scene.step_paths_device(states, SEED, STREAM, hits=hits)
    del rays
    samples = torch.zeros((n, 8), dtype=torch.float32, device=dev)     # RlLightSample
    photons = torch.zeros((n, 4), dtype=torch.float32, device=dev)     # RlMappedPhoton
    sampled_a = torch.ones(n, dtype=torch.uint8, device=dev)
    sampled_b = torch.ones(n, dtype=torch.uint8, device=dev)
    plot_a, plot_b = R.PlotUnit(0, W, H), R.PlotUnit(1, W, H)
    end = states[:, 10].view(torch.int32)
    obj = states[:, 14].view(torch.int32)
    torch.cuda.synchronize()

    def film():
        plot_a.light_paths_device(scene, states, hits, cam, SEED, STREAM, sampled=sampled_a)

    def composed():
        scene.light_paths_device(states, hits, samples, SEED, STREAM)
        status = samples[:, 7].view(torch.int32)
        vertex = (status == R.RL_LIGHT_VISIBLE) & (samples[:, 4] != 0)
        counted = (sampled_b != 0) & is_emitter[obj.clamp(0, n_objects).long()]
        ending = (end == R.RL_PATH_END_EMITTER) & (states[:, 11] != 0) & ~counted
        photons[:, 0:2] = cam[:, 8:10]
        photons[:, 2] = torch.where(vertex, samples[:, 4], torch.where(ending, states[:, 11], torch.zeros_like(states[:, 11])))
        photons[:, 3] = states[:, 3]
        sampled_b.copy_((status != R.RL_LIGHT_SKIPPED).to(torch.uint8))
        torch.cuda.synchronize()
        plot_b.plot_photons_device(photons)

    candidates = {"film": film, "composed": composed}
    times = {k: [] for k in candidates}
    for rep in range(args.reps + 1):   # round 0 warms up
        if rep == 1:                   # the check below compares one call of each onto a cleared film under the same bytes
            plot_a.clear(), plot_b.clear(), sampled_a.fill_(1), sampled_b.fill_(1)
        for name, fn in candidates.items():
            t = timed(fn)
            if rep:
                times[name].append(t)
        if rep == 1:
            fa, fb = plot_a.tristimulus_buffer, plot_b.tristimulus_buffer
            films_agree = bool(np.allclose(fa, fb, rtol=2e-5, atol=1e-6 * float(np.abs(fb).max())))
            bytes_equal = bool((sampled_a == sampled_b).all().item())
            splats = int((photons[:, 2] != 0).sum().item())
    assert films_agree and bytes_equal, "rl_plot_unit_light_paths_device and the composition disagree"

    # the whole render with and without direct light on the same camera samples
    m = args.render
    cam2 = torch.empty((m, 12), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    scene.camera_rays_device(W, H, SEED, STREAM, 1 << 32, cam2)
    render = {"render_samples": lambda: plot_a.render_samples_device(scene, cam2, SEED, STREAM, 1 << 32),
              "render_samples_direct": lambda: plot_a.render_samples_direct_device(scene, cam2, SEED, STREAM, 1 << 32)}
    rtimes = {k: [] for k in render}
    for rep in range(args.reps + 1):
        for name, fn in render.items():
            t = timed(fn)
            if rep:
                rtimes[name].append(t)

    a, b = summary(times["film"]), summary(times["composed"])
    bar = b["median_ms"] + (b["max_ms"] - b["min_ms"])
    out = {"tool": "light_film_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": "lds", "film_size": [W, H], "paths": n, "reps": args.reps,
           "splats": splats, "film": a, "composed": b, "a_bar_ms": round(bar, 3), "a_within_bar": a["median_ms"] <= bar,
           "a_film_over_composed": round(a["median_ms"] / b["median_ms"], 4), "films_agree": films_agree, "sampled_bytes_equal": bytes_equal,
           "render_paths": m}
    for name, ts in rtimes.items():
        s = summary(ts)
        s["msamples_per_s"] = round(m / (s["median_ms"] * 1e-3) / 1e6, 3)
        out[name] = s
    out["direct_over_plain"] = round(out["render_samples_direct"]["median_ms"] / out["render_samples"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
