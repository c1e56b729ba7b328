"""The re-trace identity of the relight film on the CPU oracles alone: the demo scene (A) and the demo scene with the sun sphere at
3200 K and half the intensity (B), the same 2^16 paths at 64 x 36 by tests/_path_oracle.py; A's 81-node relight film mixed with that
light's gains under the CIE table against B's XYZ film.  Writes the largest gap as a fraction of the image maximum and of the
per-pixel bound the data gives (tests/_relight_oracle.py: retrace_bound).  No GPU.  What comes out is written as it comes out.
Usage: python tools/relight_gain.py [--out tests/golden/relight_retrace.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _relight_cases as RC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "relight_retrace.json"))
    a = ap.parse_args()
    gap, bound, data, rounding, retraced = RC.retrace_figures()
    on = bound > 0
    samples, results, _ = RC.retrace()
    table = {"config": dict(RC.RETRACE, light=RC.SUN, light_from=list(RC.SUN_FROM), light_to=list(RC.SUN_TO), nodes=81, groups=3),
             "paths": int(len(samples)), "paths_on_the_light": int((results["object"] == RC.SUN).sum()),
             "lit_pixels": int((retraced.sum(axis=1) > 0).sum()), "image_maximum": float(retraced.max()), "largest_gap": float(gap.max()),
             "largest_gap_of_image_maximum": float(gap.max() / retraced.max()), "largest_gap_of_bound": float((gap[on] / bound[on]).max()),
             "data_share_of_bound_mean": float((data[on] / bound[on]).mean())}
    for key in sorted(table):
        print("%-32s %s" % (key, table[key]))
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
