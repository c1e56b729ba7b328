"""Uniform against adaptive sampling on the CPU oracle, with the seeds and budget of tests/test_gpu_adaptive.py: 64 x 36, the demo
scene, seed 1, batches of 2^16 paths of stream 0, uniform plans for the first 4, then (adaptive) re-planned from the error oracle's
tile map before every batch with a uniform share of 0.25, or (uniform) never; relative_error and worst_tile_error of the error
oracle's estimate and the mean squared error of the XYZ mean against 2^23 paths of stream 1, after 8, 16 and 32 batches.  No GPU.
Prints the table and writes the figures the device test is held to.
Usage: python tools/adaptive_gain.py [--out tests/golden/adaptive_gain.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _adaptive_oracle as AO  # noqa: E402
import _mirror as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "adaptive_gain.json"))
    a = ap.parse_args()
    objs, cam = M.builtin_desc(0)
    ref = AO.cpu_reference_mean(objs, cam)
    runs = {"uniform": AO.cpu_gain(objs, cam, False, ref), "adaptive": AO.cpu_gain(objs, cam, True, ref)}
    table = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in AO.GAIN.items()}, "budgets": {}}
    print("batches  metric            uniform      adaptive     adaptive / uniform")
    for budget in AO.GAIN["budgets"]:
        row = {}
        for metric in ("relative_error", "worst_tile_error", "mse"):
            u, ad = runs["uniform"][budget][metric], runs["adaptive"][budget][metric]
            row[metric] = {"uniform": u, "adaptive": ad, "ratio": ad / u}
            print("%7d  %-16s  %.6g  %.6g  %.4f" % (budget, metric, u, ad, ad / u))
        table["budgets"][str(budget)] = row
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
