"""What the spectral film costs beside the XYZ film.  One process on one MI355X:
  the splat: --photons photons (default 2^24) of the built-in scene at 1280 x 720, held in device memory, through
  rl_spectral_unit_plot_photons_device into --nodes nodes (default 81) and through rl_plot_unit_plot_photons_device, the two calls
  alternated in the same run.  Both calls return synchronised, so both are timed by the host clock around the call; the spectral
  launch is timed by events as well (rl_debug_spectral_ms).  Live photons (probability != 0) make 8 atomics here and 12 there;
  atomic_gbs is those atomics' added bytes over the median time.
  the projection: rl_spectral_unit_project of that film at 1280 x 720, and of a film splatted at 1920 x 1080, timed by events
  around the launch; it reads nodes x 4 bytes and writes 12 per pixel, and effective_gbs is that over the median time, beside the
  8000 GB/s of HBM that bench.py's roofline uses.
Medians with min-max of --reps calls (default 20) after --warmup (default 3).  Prints one JSON line per measurement, and appends them
to --out if given.  --only splat | plot | project runs that part alone, for a profiler's counters.
Usage (on a GPU machine): python tools/spectral_bench.py [--photons N] [--nodes K] [--reps 20] [--out profiles/spectral_bench.txt]"""
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

HBM_GBS = 8000.0        # bench.py: roofline["hbm"]["peak"]
CHUNK = 1 << 22         # paths per un-fused render


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def device_photons(scene, w, h, n):
    """n photons of paths 0 .. n - 1 (seed 1, stream 0) as a device tensor of 4 n floats, and how many are live."""
    trace = R.TraceUnit(0, w, h, n_photons=min(n, CHUNK))
    parts = []
    for first in range(0, n, CHUNK):
        trace.render(scene, seed=1, stream=0, first_path_index=first)
        parts.append(trace.mapped_photons[:min(CHUNK, n - first)].copy())
    photons = np.concatenate(parts)
    live = int((photons["probability"] != 0).sum())
    return torch.from_numpy(photons.view(np.float32).copy()).cuda(), live


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photons", type=int, default=1 << 24)
    ap.add_argument("--nodes", type=int, default=81)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["splat", "plot", "project"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**fields):
        fields.update(nodes=a.nodes, reps=a.reps, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    w, h = 1280, 720
    photons, live = device_photons(scene, w, h, a.photons)
    spectral, plot = R.SpectralUnit(w, h, a.nodes), R.PlotUnit(0, w, h)
    host = {"spectral": [], "xyz": []}
    events = []
    for k in range(a.warmup + a.reps):
        if a.only in (None, "splat", "project") and (a.only != "project" or k == 0):
            t = timed(lambda: spectral.plot_photons(photons))
            if k >= a.warmup:
                host["spectral"].append(t)
                events.append(spectral.launch_ms()[0])
        if a.only in (None, "plot"):
            t = timed(lambda: plot.plot_photons_device(photons))
            if k >= a.warmup:
                host["xyz"].append(t)
    if host["spectral"]:
        s = spread(host["spectral"])
        report(what="splat", film="spectral", size="%dx%d" % (w, h), photons=a.photons, live=live, atomics_per_live_photon=8, call_ms=s,
               launch_ms=spread(events), atomic_gbs=round(live * 8 * 4 / (s["median"] * 1e-3) / 1e9, 1),
               film_mb=round(w * h * a.nodes * 4 / 1e6, 1))
    if host["xyz"]:
        s = spread(host["xyz"])
        report(what="splat", film="xyz", size="%dx%d" % (w, h), photons=a.photons, live=live, atomics_per_live_photon=12, call_ms=s,
               atomic_gbs=round(live * 12 * 4 / (s["median"] * 1e-3) / 1e9, 1), film_mb=round(w * h * 12 / 1e6, 1))
    if host["spectral"] and host["xyz"]:
        report(what="splat ratio", spectral_over_xyz=round(float(np.median(host["spectral"]) / np.median(host["xyz"])), 4))
    if a.only in (None, "project"):
        matrix = R.spectral_observer_cie1931(a.nodes)
        for pw, ph_ in ((1280, 720), (1920, 1080)):
            unit = spectral
            if (pw, ph_) != (w, h):
                unit = R.SpectralUnit(pw, ph_, a.nodes)
                some, _ = device_photons(scene, pw, ph_, min(a.photons, CHUNK))
                unit.plot_photons(some)
            dst = R.GatherUnit(pw, ph_)
            calls, launches = [], []
            for k in range(a.warmup + a.reps):
                t = timed(lambda: unit.project(matrix, dst))
                if k >= a.warmup:
                    calls.append(t)
                    launches.append(unit.launch_ms()[1])
            s = spread(launches)
            gbs = (a.nodes * 4 + 12) * pw * ph_ / (s["median"] * 1e-3) / 1e9
            report(what="project", size="%dx%d" % (pw, ph_), call_ms=spread(calls), launch_ms=s, effective_gbs=round(gbs, 1),
                   share_of_hbm=round(gbs / HBM_GBS, 4), hbm_gbs=HBM_GBS)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
