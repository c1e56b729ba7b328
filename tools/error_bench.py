"""What the noise estimate costs.  One process on one MI355X:
  the kernels: at 1280 x 720 and 1920 x 1080, a plot buffer of a real render is shown to an error unit and gathered, again and again;
  rl_error_observe_kernel and rl_error_estimate_kernel are timed by events around their launches (rl_debug_error_ms) and
  rl_gather_kernel by events around rl_gather_unit_accumulate's launch (rl_debug_gather_accumulate_ms), the three alternated in the
  same run.  Per pixel observe reads 12 B of plot buffer and 16 B of state and writes 16 B (44 B); the gather kernel reads 36 B and
  writes 36 B (72 B); the estimate reads 16 B and writes 4 B (20 B; the tile pairs are 16 B per 256 pixels more).  effective_gbs is
  those bytes over the median time, beside the 8000 GB/s of HBM that bench.py's roofline uses.  The bar: observe moves 44 B where the
  gather kernel moves 72, so its median must not exceed the gather kernel's ("observe_within_gather").
  the gather loop: what a Gather task of the App does, on the host's clock: --loop-gathers rl_gather_unit_accumulate calls over 32
  plot units holding a film, queued without waiting and synchronised once at the end, against the same loop with an
  rl_error_unit_observe in front of each; the difference per observation is what an observation costs a pipeline of gathers, beside
  the kernel's own time: the rest is its four event records, two cross-stream waits and one launch, and the hops between three
  streams (plot, error unit, gather unit) where there was one.
  the App: rl_app_run against rl_app_run_to_error with target 0 (every observation and every estimate made, the run never stopped
  early) on bench.py's App configuration, alternated, in Grays/s from the runs' own segment counts and wall time.
Medians with min-max of --reps launches (default 20) after --warmup (default 3).  Prints one JSON line per measurement, and appends
them to --out if given.
Usage (on a GPU machine): python tools/error_bench.py [--reps 20] [--app-batches 8192] [--out profiles/error_bench.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import time  # noqa: E402

import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

HBM_GBS = 8000.0        # bench.py: roofline["hbm"]["peak"]
BYTES = {"observe": 44, "gather": 72, "estimate": 20}


def spread(xs):
    return {"median": round(float(np.median(xs)), 5), "min": round(float(min(xs)), 5), "max": round(float(max(xs)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-gathers", type=int, default=64)
    ap.add_argument("--app-batches", type=int, default=8192)
    ap.add_argument("--app-threads", type=int, default=4)
    ap.add_argument("--app-tonemap-ms", type=int, default=250)
    ap.add_argument("--app-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def report(**fields):
        fields.update(reps=a.reps, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    for w, h in ((1280, 720), (1920, 1080)):
        trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
        unit, gather = R.ErrorUnit(w, h), R.GatherUnit(w, h)
        n = 1 << 22
        trace.render_fused(scene, plot, n, seed=1, stream=0, first_path_index=0)
        film = plot.tristimulus_buffer
        ms = {"observe": [], "gather": [], "estimate": []}
        for k in range(a.warmup + a.reps):
            plot.upload(film)                       # (the gather kernel clears the buffer: the same film every round)
            unit.observe(plot, n)
            t_observe = unit.launch_ms()[0]         # waits for the launch
            t_gather = R.gather_accumulate_ms(gather, plot)
            t_estimate = None
            if k >= 1:
                unit.estimate(se=False, tiles=False)
                t_estimate = unit.launch_ms()[1]
            if k >= a.warmup:
                ms["observe"].append(t_observe)
                ms["gather"].append(t_gather)
                ms["estimate"].append(t_estimate)
        med = {}
        for what in ("observe", "gather", "estimate"):
            s = spread(ms[what])
            med[what] = s["median"]
            gbs = BYTES[what] * w * h / (s["median"] * 1e-3) / 1e9
            report(what=what, size="%dx%d" % (w, h), launch_ms=s, bytes_per_pixel=BYTES[what], effective_gbs=round(gbs, 1),
                   share_of_hbm=round(gbs / HBM_GBS, 4), hbm_gbs=HBM_GBS)
        report(what="observe against gather", size="%dx%d" % (w, h), observe_over_gather=round(med["observe"] / med["gather"], 4),
               observe_within_gather=bool(med["observe"] <= med["gather"]))

    w, h = 1280, 720
    plots = [R.PlotUnit(i, w, h) for i in range(32)]
    unit, gather = R.ErrorUnit(w, h), R.GatherUnit(w, h)
    trace = R.TraceUnit(0, w, h, n_photons=64)
    trace.render_fused(scene, plots[0], 1 << 22, seed=1, stream=0, first_path_index=0)
    film = plots[0].tristimulus_buffer
    loop = {"gather": [], "observe+gather": []}
    for k in range(a.warmup + a.reps):
        for label in ("gather", "observe+gather"):
            for p in plots:
                p.upload(film)
            gather.sync()
            t0 = time.perf_counter()
            for j in range(a.loop_gathers):
                p = plots[j % len(plots)]
                if label != "gather":
                    unit.observe(p, 1 << 22)
                gather.accumulate(p)
            gather.sync()
            ms = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                loop[label].append(ms)
    extra = (float(np.median(loop["observe+gather"])) - float(np.median(loop["gather"]))) / a.loop_gathers
    report(what="gather loop", size="%dx%d" % (w, h), gathers=a.loop_gathers, plot_units=len(plots), loop_ms={k: spread(v) for k, v in loop.items()},
           extra_ms_per_observation=round(extra, 5))
    del plots, unit, gather, trace

    # bench.py's App configuration (measure_app): 1280 x 720, Trace tasks of 524,288 paths, scheduler depth 64, fused; a tonemap,
    # and with it an estimate, every --app-tonemap-ms (bench.py's 30 s would leave the final estimate alone)
    app = dict(concurrency=64, threads=a.app_threads, photons_per_batch=1024 * 512, fused=True, tonemap_interval_ms=a.app_tonemap_ms)
    grays = {"rl_app_run": [], "rl_app_run_to_error": []}
    detail = None
    for k in range(1 + a.app_reps):
        rgb, st = R.app_run(1280, 720, a.app_batches, **app)
        rgb, st2, err = R.app_run_to_error(1280, 720, a.app_batches, target_error=0.0, **app)
        if k >= 1:
            grays["rl_app_run"].append(st["segments"] / st["seconds"] / 1e9)
            grays["rl_app_run_to_error"].append(st2["segments"] / st2["seconds"] / 1e9)
            detail = {"seconds": [round(st["seconds"], 4), round(st2["seconds"], 4)], "observations": err["at_end"]["observations"],
                      "estimates": err["estimates"], "gathers": st2["tasks"]["gather"], "tonemaps": st2["tonemaps"],
                      "relative_error": round(err["at_end"]["relative_error"], 6)}
    base, with_error = float(np.median(grays["rl_app_run"])), float(np.median(grays["rl_app_run_to_error"]))
    report(what="app", size="1280x720", batches=a.app_batches, config=app, grays_per_s={k: spread(v) for k, v in grays.items()},
           with_error_over_without=round(with_error / base, 4), last_run=detail)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
