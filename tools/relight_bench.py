"""What the relight film costs.  One process on one MI355X, 1280 x 720, 81 nodes, 3 groups, the demo scene; one warm-up and --reps
(default 5) repetitions, the calls of a comparison alternated in the same run; every figure is a median (min - max) in milliseconds.
  (a) rl_relight_unit_render of --paths paths (default 2^24), by the host clock around the call (it returns synchronised), against
      the three calls that make the group-less film of the same paths: rl_scene_camera_rays_device, rl_scene_render_rays_device
      and rl_spectral_unit_plot_photons_device, each by the host clock, the rays and photons assembled outside the timed region.
      The bar: render's median <= the sum of the three medians plus the sum of their spreads (max - min).  Beside it the ratio to
      rl_plot_unit_render_samples_device of the same samples: the price over the XYZ film.
  (b) rl_relight_unit_mix, by events around its launch, against rl_spectral_unit_project on a 243-node spectral unit holding the
      same planes -- the same kernel at the same plane count.  The bar: the mix's median <= the projection's median plus its
      spread.  Beside it the mix as a multiple of a device copy of the bytes it reads.
A bar that is missed is written as it came out.  Prints one JSON line per measurement and appends them to --out if given.
Usage (on a GPU machine): python tools/relight_bench.py [--paths N] [--reps 5] [--out profiles/relight_bench.txt]"""
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

W, H, NODES, GROUPS = 1280, 720, 81, 3
SEED, STREAM = 1, 0


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**fields):
        fields.update(size="%dx%d" % (W, H), nodes=NODES, groups=GROUPS, reps=a.reps, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    n = a.paths
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    relight = R.RelightUnit(W, H, NODES, GROUPS)
    relight.set_groups(R.relight_groups(objs, GROUPS))
    spectral, plot = R.SpectralUnit(W, H, NODES), R.PlotUnit(0, W, H)
    samples = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
    results = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    # the rays and the photons of the three-call path, assembled once outside the timed region
    scene.camera_rays_device(W, H, SEED, STREAM, 0, samples)
    rays = samples[:, :8].contiguous()
    scene.render_rays_device(rays, results, SEED, STREAM, 0)
    photons = torch.stack([samples[:, 8], samples[:, 9], results[:, 0], samples[:, 3]], dim=1).contiguous()
    torch.cuda.synchronize()
    t = {"render": [], "camera": [], "paths": [], "splat": [], "xyz": []}
    for k in range(a.warmup + a.reps):
        row = {"render": timed(lambda: relight.render(scene, SEED, STREAM, 0, n)),
               "camera": timed(lambda: scene.camera_rays_device(W, H, SEED, STREAM, 0, samples)),
               "paths": timed(lambda: scene.render_rays_device(rays, results, SEED, STREAM, 0)),
               "splat": timed(lambda: spectral.plot_photons(photons)),
               "xyz": timed(lambda: plot.render_samples_device(scene, samples, SEED, STREAM, 0))}
        if k >= a.warmup:
            for name, ms in row.items():
                t[name].append(ms)
    s = {name: spread(xs) for name, xs in t.items()}
    three = sum(s[name]["median"] for name in ("camera", "paths", "splat"))
    slack = sum(s[name]["max"] - s[name]["min"] for name in ("camera", "paths", "splat"))
    report(what="(a) render", paths=n, render_ms=s["render"], camera_rays_ms=s["camera"], render_rays_ms=s["paths"],
           spectral_plot_photons_ms=s["splat"], three_calls_ms=round(three, 4), three_calls_spread_ms=round(slack, 4),
           bar="render median <= three calls + their spread", met=bool(s["render"]["median"] <= three + slack),
           render_over_three_calls=round(s["render"]["median"] / three, 4), plot_render_samples_ms=s["xyz"],
           render_over_xyz_film=round(s["render"]["median"] / s["xyz"]["median"], 4), last_chunk_launch_ms=[round(x, 4) for x in relight.launch_ms()[:2]])

    # (b) the mix against the projection of a 243-node spectral unit that holds the same planes
    del samples, results, rays, photons
    planes = NODES * GROUPS
    wide, dst = R.SpectralUnit(W, H, planes), R.GatherUnit(W, H)
    wide.upload(relight.download().reshape(planes, H, W))
    cie = R.spectral_observer_cie1931(NODES)
    gains = np.ones((GROUPS, NODES), np.float32)
    gains[0] = R.relight_gains_black_body(NODES, 6504.0, 1.0, 3200.0, 0.5)
    composed = (gains[:, :, None] * cie[None, :, :]).reshape(planes, 3)
    src = torch.zeros(planes * W * H, dtype=torch.float32, device="cuda")
    into = torch.empty_like(src)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    m = {"mix": [], "project": [], "copy": []}
    for k in range(a.warmup + a.reps):
        # (whichever comes second finds the chip as the first left it: the order changes with every repetition)
        for call in ((lambda: relight.mix(gains, cie, dst)), (lambda: wide.project(composed, dst)))[::1 if k % 2 == 0 else -1]:
            call()
        start.record()
        into.copy_(src)
        stop.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            m["mix"].append(relight.launch_ms()[2])
            m["project"].append(wide.launch_ms()[1])
            m["copy"].append(start.elapsed_time(stop))
    s = {name: spread(xs) for name, xs in m.items()}
    bar = s["project"]["median"] + (s["project"]["max"] - s["project"]["min"])
    read_mb = planes * W * H * 4 / 1e6
    report(what="(b) mix", mix_ms=s["mix"], project_243_nodes_ms=s["project"], bar="mix median <= projection median + its spread",
           met=bool(s["mix"]["median"] <= bar), mix_over_projection=round(s["mix"]["median"] / s["project"]["median"], 4),
           read_mb=round(read_mb, 1), device_copy_ms=s["copy"], mix_over_device_copy=round(s["mix"]["median"] / s["copy"]["median"], 4),
           read_gbs=round(read_mb / 1e3 / (s["mix"]["median"] * 1e-3), 1), kernel="rl_spectral_project_kernel on the composed matrix")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
