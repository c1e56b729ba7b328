"""What wavelength importance sampling costs and buys.  One process on one MI355X, 1280 x 720, the demo scene, LDS fetch:
  time    rl_trace_unit_render_fused of 2^26 paths without a table and with the CIE table at a uniform share of 0.1, alternated in
          one run: --reps calls (default 20) after --warmup (default 3); the host's clock around the call and its sync, and the
          events around the launch (rl_trace_unit_stats); median with min - max.
  error   batches of 2^22 paths, each observed by an error unit and gathered, both ways: the Y relative_error after 64 batches, and
          the batches until it is at most --target-error (default 0.02), looked at every 8 batches from the 16th on.
The bar is the pay-off: (time with the table / time without) x (relative_error with / without)^2 < 1, both measured here.
Prints one JSON line per measurement, and appends them to --out if given.
Usage (on a GPU machine): python tools/wavelength_bench.py [--reps 20] [--out profiles/wavelength_bench.txt]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H, SEED, STREAM = 1280, 720, 1, 0
SHARE = 0.1


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--budget", type=int, default=64)
    ap.add_argument("--max-batches", type=int, default=3072)
    ap.add_argument("--target-error", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert R.device_count() > 0, "wavelength_bench.py needs a GPU"
    lines = []

    def report(**fields):
        fields.update(size="%dx%d" % (W, H), uniform_share=SHARE, build=R.build_id())
        lines.append(json.dumps(fields))
        print(lines[-1], flush=True)

    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    table = R.WavelengthTable("cie", SHARE)
    units = {"uniform": R.TraceUnit(0, W, H, n_photons=64), "importance": R.TraceUnit(1, W, H, n_photons=64)}
    units["importance"].set_wavelengths(table)
    plot = R.PlotUnit(0, W, H)

    # ---- time ----
    host, device = {k: [] for k in units}, {k: [] for k in units}
    plain0, wl0 = R.variant_launches(), R.wavelength_variant_launches()
    for k in range(a.warmup + a.reps):
        for name, unit in units.items():
            ms0 = unit.stats()[2]
            t0 = time.perf_counter()
            unit.render_fused(scene, plot, a.paths, seed=SEED, stream=STREAM, first_path_index=0)
            unit.sync()
            t = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                host[name].append(t)
                device[name].append(unit.stats()[2] - ms0)
            plot.clear()
    ran = {"plain": [i for i, (x, y) in enumerate(zip(R.variant_launches(), plain0)) if x != y],
           "wl": [i for i, (x, y) in enumerate(zip(R.wavelength_variant_launches(), wl0)) if x != y]}
    time_ratio = float(np.median(device["importance"])) / float(np.median(device["uniform"]))
    report(what="render_fused", paths=a.paths, reps=a.reps, variants=ran, uniform_ms=spread(device["uniform"]), importance_ms=spread(device["importance"]),
           uniform_host_ms=spread(host["uniform"]), importance_host_ms=spread(host["importance"]),
           uniform_gpaths_s=round(a.paths / float(np.median(device["uniform"])) / 1e6, 3),
           importance_gpaths_s=round(a.paths / float(np.median(device["importance"])) / 1e6, 3),
           importance_over_uniform=round(time_ratio, 4),
           within_own_spread=bool(min(device["importance"]) / max(device["uniform"]) <= 1.0 <= max(device["importance"]) / min(device["uniform"])))

    # ---- error ----
    at_budget, reached = {}, {}
    for name, unit in units.items():
        gather, error = R.GatherUnit(W, H), R.ErrorUnit(W, H)
        for batch in range(a.max_batches):
            unit.render_fused(scene, plot, a.batch, seed=SEED, stream=STREAM, first_path_index=batch * a.batch)
            error.observe(plot, a.batch)
            gather.accumulate(plot)
            if batch + 1 < 16 or ((batch + 1) % 8 != 0 and batch + 1 != a.budget):
                continue
            rel = error.estimate(se=False, tiles=False)[0]["relative_error"]
            if batch + 1 == a.budget:
                at_budget[name] = rel
            if name not in reached and rel <= a.target_error:
                reached[name] = (batch + 1, rel)
            if name in reached and name in at_budget:
                break
    error_ratio = at_budget["importance"] / at_budget["uniform"]
    report(what="relative_error", batch=a.batch, budget=a.budget, uniform=at_budget["uniform"], importance=at_budget["importance"],
           importance_over_uniform=round(error_ratio, 4), paths_for_equal_error=round(error_ratio ** 2, 4))
    report(what="batches to the target", batch=a.batch, target_error=a.target_error,
           uniform={"batches": reached.get("uniform", (None, None))[0], "relative_error": reached.get("uniform", (None, None))[1]},
           importance={"batches": reached.get("importance", (None, None))[0], "relative_error": reached.get("importance", (None, None))[1]})
    payoff = time_ratio * error_ratio ** 2
    report(what="pay-off", time_ratio=round(time_ratio, 4), error_ratio=round(error_ratio, 4), payoff=round(payoff, 4), within_bar=bool(payoff < 1.0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
