"""The plain noise estimate against the robust film's on the CPU oracles alone: 64 x 36, the glass-stress scene and the demo scene,
M = 15 buckets, gain 1; B batches of stream 0, each shown to the error oracle (tests/_error_oracle.py) and to bucket b mod M of the
robust state, whose estimate is tests/_robust_error_oracle.py's.  Per configuration: relative_error of both estimates on the same
buffers; the firefly pixels (tools/robust_gain.py's definition and reference: plain Y above 4 times that of 16 times the paths from
stream 1); and the share of the next adaptive batch that the plan rule (tests/_adaptive_oracle.py, uniform_share 0.25) gives to the
tiles that hold them, under each of the two tile maps.  No GPU.  Nothing is promised: what comes out is printed and written, a loss
included.
Usage: python tools/robust_error_gain.py [--out tests/golden/robust_error_gain.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _mirror as M  # noqa: E402
import _robust_error_oracle as REO  # noqa: E402

SCENES = {0: "demo", 1: "glass"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "robust_error_gain.json"))
    a = ap.parse_args()
    table = {"config": dict(REO.GAIN), "runs": []}
    print("scene  batches x paths   relative_error: plain  robust  ratio    firefly pixels  tiles    their share of the next batch: plain  robust")
    for which, batches, n in REO.GAIN_CONFIGS:
        objs, cam = M.builtin_desc(which)
        run = REO.gain_figures(objs, cam, batches, n)
        run["scene"] = SCENES[which]
        table["runs"].append(run)
        p, r = run["plain"], run["robust"]
        print("%-5s  %4d x %-6d    %.6g  %.6g  %.4f    %d  %d of %d    %s  %s"
              % (run["scene"], batches, n, p["relative_error"], r["relative_error"], r["relative_error"] / p["relative_error"],
                 run["firefly_pixels"], run["firefly_tiles"], run["tiles"], p["firefly_tile_share"], r["firefly_tile_share"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
