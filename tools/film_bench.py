"""What the film costs: PlotUnit.render_samples_device (trace and splat in one kernel) against the two-call form and against the
path kernel alone, on the built-in scene at 1920x1080.  rl_scene_camera_rays_device makes the camera samples of paths 0 .. n-1 (64 M
by default) on the device; then, alternated --rounds times in this one process with everything resident,
  fused     rl_plot_unit_render_samples_device(results = NULL)
  two_call  rl_scene_render_rays_device, a pack of (x, y, value, wavelength) into RlMappedPhoton records (torch, on the device),
            rl_plot_unit_plot_photons_device
  paths     rl_scene_render_rays_device alone (what the splat costs the path loop)
and, for the 2^20 photons of one rl_trace_unit_render, rl_plot_unit_plot_photons_device against rl_plot_unit_plot + sync.  Each time
is the host clock around calls that end synchronised, after one warm-up round.  The films of the fused and the two-call form are
compared (np.allclose, the suite's tolerance).  Prints one JSON line with every round's times, medians and spreads.
Usage (on a GPU machine): python tools/film_bench.py [--paths 67108864] [--rounds 5]"""
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


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3),
            "rounds_ms": [round(t * 1e3, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fetch", choices=["lds", "global"], default="lds")
    args = ap.parse_args()
    assert R.device_count() > 0, "film_bench.py needs a GPU"
    n = args.paths
    fetch = R.FETCH_LDS if args.fetch == "lds" else R.FETCH_GLOBAL
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    dev = torch.device("cuda:0")

    samples = torch.empty((n, 12), dtype=torch.float32, device=dev)   # RlCameraSample: 48 bytes
    scene.camera_rays_device(W, H, SEED, STREAM, 0, samples)
    rays = samples[:, :8].contiguous()                                 # RlSpectralRay: the first 32 bytes
    results = torch.empty((n, 4), dtype=torch.float32, device=dev)    # RlPathResult (value is its first float)
    photons = torch.empty((n, 4), dtype=torch.float32, device=dev)    # RlMappedPhoton
    torch.cuda.synchronize()
    fused_unit, two_unit = R.PlotUnit(0, W, H), R.PlotUnit(1, W, H)

    def fused():
        fused_unit.render_samples_device(scene, samples, SEED, STREAM, 0, fetch=fetch)

    def paths():
        scene.render_rays_device(rays, results, SEED, STREAM, 0, fetch=fetch)

    def two_call():
        paths()
        photons[:, 0:2] = samples[:, 8:10]
        photons[:, 2] = results[:, 0]
        photons[:, 3] = samples[:, 3]
        torch.cuda.synchronize()
        two_unit.plot_photons_device(photons)

    # the films agree (one round each onto cleared units), and which variant ran
    before = R.film_launches()
    fused()
    variant = next(i for i, (a, b) in enumerate(zip(R.film_launches(), before)) if a != b)
    two_call()
    a, b = fused_unit.tristimulus_buffer, two_unit.tristimulus_buffer
    assert np.count_nonzero(b) and np.allclose(a, b, rtol=2e-5, atol=1e-6 * np.abs(b).max()), float(np.abs(a - b).max())
    res = results.cpu().numpy().view(R.PATH_RESULT_DTYPE).reshape(-1)
    segments, contributing = int(res["segments"].sum(dtype=np.uint64)), int((res["value"] != 0).sum())
    del res, a, b

    times = {"fused": [], "two_call": [], "paths": []}
    for _ in range(args.rounds):
        for name, fn in (("fused", fused), ("two_call", two_call), ("paths", paths)):
            times[name].append(clock(fn))

    # PlotUnit::plot of one batch's photons: the caller's-photons kernel against the trace-unit one
    m = 1 << 20
    trace = R.TraceUnit(0, W, H, n_photons=m)
    trace.render(scene, SEED, STREAM, 0)
    batch = torch.from_numpy(trace.mapped_photons.view(np.float32).reshape(m, 4)).to(dev)
    torch.cuda.synchronize()
    unit = R.PlotUnit(2, W, H)

    def plot_unit():
        unit.plot([trace])
        unit.sync()

    def plot_photons():
        unit.plot_photons_device(batch)

    plot_unit(), plot_photons()
    small = {"plot": [], "plot_photons": []}
    for _ in range(max(args.rounds, 20)):
        small["plot"].append(clock(plot_unit))
        small["plot_photons"].append(clock(plot_photons))

    f, t, p = (float(np.median(times[k])) for k in ("fused", "two_call", "paths"))
    out = {"tool": "film_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": args.fetch, "variant": variant, "paths": n,
           "segments": segments, "contributing": contributing, "rounds": args.rounds,
           "fused": summary(times["fused"]), "two_call": summary(times["two_call"]), "paths_alone": summary(times["paths"]),
           "fused_gsegments_per_s": round(segments / f / 1e9, 3), "paths_alone_gsegments_per_s": round(segments / p / 1e9, 3),
           "fused_over_two_call": round(f / t, 4), "fused_over_paths_alone": round(f / p, 4),
           "fused_spread_ms": round((max(times["fused"]) - min(times["fused"])) * 1e3, 3),
           "fused_within_spread_of_two_call": bool(f <= t + (max(times["fused"]) - min(times["fused"]))),
           "plot_1m_photons": summary(small["plot"]), "plot_photons_1m": summary(small["plot_photons"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
