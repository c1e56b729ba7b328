"""What the robust film costs.  One process on one MI355X, at 1280 x 720 with M = 15 and M = 32 buckets:
  observe: a plot buffer of a real render is shown to a robust unit (the buckets in turn) and to an error unit, again and again;
  rl_robust_observe_kernel and rl_error_observe_kernel are timed by events around their launches (rl_debug_robust_ms,
  rl_debug_error_ms), and a device-to-device copy of as many bytes as the robust kernel moves -- it reads 12 B of plot buffer and 24 B
  of state and writes 24 B per pixel, 60 B: the copy reads 30 and writes 30 -- by torch events, the three alternated in the same run.
  resolve: rl_robust_resolve_kernel by the events around its launch, at gain 1; it reads 24 M B and writes 13 B per pixel
  (12 B of film and the trim byte; the compensation's memset is not part of the launch), and a copy of as many bytes beside it.
effective_gbs is those bytes over the median time, beside the 8000 GB/s of HBM that bench.py's roofline uses.  Records, not bars.
Medians with min-max of --reps launches (default 20) after --warmup (default 5).  Prints one JSON line per measurement and appends
them to --out if given.
Usage (on a GPU machine): python tools/robust_bench.py [--reps 20] [--out profiles/robust_bench.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

HBM_GBS = 8000.0        # bench.py: roofline["hbm"]["peak"]


def spread(xs):
    return {"median": round(float(np.median(xs)), 5), "min": round(float(min(xs)), 5), "max": round(float(max(xs)), 5)}


def copy_ms(dst, src):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    dst.copy_(src)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robust_bench needs a GPU: nothing is measured without one")
    lines = []

    def report(**fields):
        fields.update(reps=a.reps, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    w, h = 1280, 720
    pixels = w * h
    scene = R.Scene(*R.builtin_scene_desc(R.SCENE_GLASS_STRESS))
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    n = 1 << 22
    trace.render_fused(scene, plot, n, seed=1, stream=0, first_path_index=0)
    plot.sync()
    error, dst = R.ErrorUnit(w, h), R.GatherUnit(w, h)
    for m in (15, 32):
        unit = R.RobustUnit(w, h, m)
        observe_bytes, resolve_bytes = 60, 24 * m + 13
        a60, b60 = (torch.empty(pixels * observe_bytes // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        ar, br = (torch.empty(pixels * resolve_bytes // 2 + 1, dtype=torch.uint8, device="cuda") for _ in range(2))
        ms = {"robust observe": [], "error observe": [], "copy of 60 B per pixel": [], "resolve": [], "copy of the resolve's bytes": []}
        for k in range(a.warmup + a.reps + m):       # (the first m rounds fill the buckets: the resolve needs every one)
            unit.observe(plot, n)
            t_robust = unit.launch_ms()[0]            # waits for the launch
            error.observe(plot, n)
            t_error = error.launch_ms()[0]
            t_copy = copy_ms(b60, a60)
            if k < m - 1:
                continue
            unit.resolve(dst, gain=1.0)
            t_resolve = unit.launch_ms()[1]
            t_copy_r = copy_ms(br, ar)
            if k >= m + a.warmup:
                for key, t in zip(ms, (t_robust, t_error, t_copy, t_resolve, t_copy_r)):
                    ms[key].append(t)
        med = {}
        for what, nbytes in (("robust observe", observe_bytes), ("error observe", 44), ("copy of 60 B per pixel", observe_bytes),
                             ("resolve", resolve_bytes), ("copy of the resolve's bytes", resolve_bytes)):
            s = spread(ms[what])
            med[what] = s["median"]
            gbs = nbytes * pixels / (s["median"] * 1e-3) / 1e9
            report(what=what, size="%dx%d" % (w, h), buckets=m, launch_ms=s, bytes_per_pixel=nbytes, effective_gbs=round(gbs, 1),
                   share_of_hbm=round(gbs / HBM_GBS, 4), hbm_gbs=HBM_GBS)
        report(what="ratios", size="%dx%d" % (w, h), buckets=m, observe_over_copy=round(med["robust observe"] / med["copy of 60 B per pixel"], 4),
               observe_over_error_observe=round(med["robust observe"] / med["error observe"], 4),
               resolve_over_copy=round(med["resolve"] / med["copy of the resolve's bytes"], 4))
        del unit, a60, b60, ar, br
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
