"""The plain film against the robust film on the CPU oracle alone: 64 x 36, the glass-stress scene and the demo scene, M = 15 buckets,
gain 1; the film is B batches of stream 0, batch b into bucket b mod M, taken as the plain sum and as the robust oracle's resolve
(tests/_robust_oracle.py), both against a reference of 16 times the paths from stream 1.  Per configuration: the relative mean squared
error of Y and the number of pixels whose Y exceeds the reference's by a factor of 4, for both films, and the histogram of the trim.
No GPU.  Nothing is promised: what comes out is printed and written, a loss included.
Usage: python tools/robust_gain.py [--out tests/golden/robust_gain.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _mirror as M  # noqa: E402
import _robust_oracle as RO  # noqa: E402

SCENES = {0: "demo", 1: "glass"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "robust_gain.json"))
    a = ap.parse_args()
    table = {"config": dict(RO.GAIN), "runs": []}
    print("scene  batches x paths   rel. MSE of Y: plain  robust  ratio    pixels > 4 x reference: plain  robust   trim histogram")
    for which, batches, n in RO.GAIN_CONFIGS:
        objs, cam = M.builtin_desc(which)
        run = RO.gain_figures(objs, cam, batches, n)
        run["scene"] = SCENES[which]
        table["runs"].append(run)
        p, r = run["plain"], run["robust"]
        print("%-5s  %4d x %-6d    %.6g  %.6g  %.4f    %d  %d    %s" % (run["scene"], batches, n, p["rel_mse_y"], r["rel_mse_y"],
                                                                        r["rel_mse_y"] / p["rel_mse_y"], p["firefly_pixels"], r["firefly_pixels"],
                                                                        run["trim_histogram"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
