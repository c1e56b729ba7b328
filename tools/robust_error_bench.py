"""What the robust film's noise estimate costs.  One process on one MI355X, at 1280 x 720 with M = 15 and M = 32 buckets, over the
plot buffer of a real render shown to every bucket: rl_robust_estimate_kernel by the events around its launch
(rl_debug_robust_estimate_ms), at gain 1 -- it reads the M Y planes, 8 M B per pixel, and writes 5 B (se and the trim byte; the tiles
are 16 B per 256 pixels) --, alternated in the same run with rl_robust_resolve_kernel (rl_debug_robust_ms, 24 M + 13 B per pixel),
rl_error_estimate_kernel (rl_debug_error_ms, 20 B per pixel) and a device-to-device copy of as many bytes as the estimate moves
(torch events).  The expectation this checks: the estimate takes no longer than 1.1 times the resolve at the same M in the same
run -- it reads a third of the planes and runs the same M^2 rank loop; the 10 % cover the spread between alternated runs.  The
"ratios" line records estimate_over_resolve and whether it is within 1.1; a record, not a bar.
effective_gbs is the bytes over the median time, beside the 8000 GB/s of HBM that bench.py's roofline uses.
Medians with min-max of --reps launches (default 20) after --warmup (default 5).  Prints one JSON line per measurement and appends
them to --out if given.
Usage (on a GPU machine): python tools/robust_error_bench.py [--reps 20] [--out profiles/robust_error_bench.txt]"""
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
        raise SystemExit("robust_error_bench needs a GPU: nothing is measured without one")
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
    error, dst = R.ErrorUnit(w, h), R.GatherUnit(w, h)
    for m in (15, 32):
        unit = R.RobustUnit(w, h, m)
        for b in range(m):                            # a batch of its own for every bucket: the keys of a pixel differ
            plot.clear()
            trace.render_fused(scene, plot, n, seed=1, stream=0, first_path_index=b * n)
            plot.sync()
            unit.observe(plot, n)
            if m == 15:
                error.observe(plot, n)
        estimate_bytes, resolve_bytes, error_bytes = 8 * m + 5, 24 * m + 13, 20
        ac, bc = (torch.empty(pixels * estimate_bytes // 2 + 1, dtype=torch.uint8, device="cuda") for _ in range(2))
        ms = {"estimate": [], "resolve": [], "error estimate": [], "copy of the estimate's bytes": []}
        for k in range(a.warmup + a.reps):
            stats = unit.estimate(gain=1.0, se=False)[0]
            t_estimate = unit.estimate_ms()           # waits for the launch
            unit.resolve(dst, gain=1.0)
            t_resolve = unit.launch_ms()[1]
            error.estimate(se=False)
            t_error = error.launch_ms()[1]
            t_copy = copy_ms(bc, ac)
            if k >= a.warmup:
                for key, t in zip(ms, (t_estimate, t_resolve, t_error, t_copy)):
                    ms[key].append(t)
        med = {}
        for what, nbytes in (("estimate", estimate_bytes), ("resolve", resolve_bytes), ("error estimate", error_bytes),
                             ("copy of the estimate's bytes", estimate_bytes)):
            s = spread(ms[what])
            med[what] = s["median"]
            gbs = nbytes * pixels / (s["median"] * 1e-3) / 1e9
            report(what=what, size="%dx%d" % (w, h), buckets=m, launch_ms=s, bytes_per_pixel=nbytes, effective_gbs=round(gbs, 1),
                   share_of_hbm=round(gbs / HBM_GBS, 4), hbm_gbs=HBM_GBS)
        over = med["estimate"] / med["resolve"]
        report(what="ratios", size="%dx%d" % (w, h), buckets=m, estimate_over_resolve=round(over, 4), within_1_1_of_the_resolve=bool(over <= 1.1),
               estimate_over_error_estimate=round(med["estimate"] / med["error estimate"], 4),
               estimate_over_copy=round(med["estimate"] / med["copy of the estimate's bytes"], 4), relative_error=stats["relative_error"])
        del unit, ac, bc
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
