"""The uniform wavelength draw against the CIE table at a uniform share of 0.1, on the CPU, with the seeds and budgets of
tests/test_gpu_wavelength.py: 64 x 36, the demo scene, seed 1, batches of 2^16 paths of stream 0 through tests/wavelength_host (the
g++ compile of the kernel's per-path header and of rl_wavelength.h), each batch's film observed by tests/_error_oracle.py;
relative_error and worst_tile_error of the estimate and the mean squared error of the mean against 2^23 uniform paths of stream 1
from the CPU oracle, for each of X, Y and Z, after 8, 16 and 32 batches.  No GPU.  Prints the table and writes the figures the device
test is held to.
Usage: python tools/wavelength_gain.py [--out tests/golden/wavelength_gain.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _adaptive_oracle as AO  # noqa: E402
import _mirror as M  # noqa: E402
import _wavelength_oracle as WO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wavelength_gain.json"))
    a = ap.parse_args()
    cfg = WO.GAIN
    objs, cam = M.builtin_desc(0)
    ref = AO.cpu_reference_mean(objs, cam, cfg)
    status, q, w = WO.table(WO.cie_importance(), 81, cfg["share"])
    assert status == WO.OK
    runs = {"uniform": WO.cpu_gain(objs, cam, None, ref), "importance": WO.cpu_gain(objs, cam, WO.packed(q, w), ref)}
    table = {"config": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "ratio_relative_error": {}}
    print("batches  component  metric            uniform      importance   importance / uniform")
    for name, run in runs.items():
        table[name] = {str(budget): run[budget] for budget in cfg["budgets"]}
    for budget in cfg["budgets"]:
        table["ratio_relative_error"][str(budget)] = {}
        for component in "XYZ":
            for metric in ("relative_error", "worst_tile_error", "mse"):
                u, im = runs["uniform"][budget][component][metric], runs["importance"][budget][component][metric]
                print("%7d  %-9s  %-16s  %.6g  %.6g  %.4f" % (budget, component, metric, u, im, im / u))
            table["ratio_relative_error"][str(budget)][component] = (runs["importance"][budget][component]["relative_error"] /
                                                                     runs["uniform"][budget][component]["relative_error"])
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
