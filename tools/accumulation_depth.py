"""How far the accumulated XYZ film lies from the float64 sum of its photons at depth: the cases of tests/test_gpu_accumulation.py
through the same helpers (tests/_accumulation.py), with the figures the test only bounds.  9,437,184 paths of the built-in scene
on 16x9 (65,536 paths per pixel) and 64x36 (4,096 per pixel), {fused, un-fused} x {1,024 gathers of one 9,216-path launch, 16
gathers of nine 65,536-path launches}; the reference is the device's own un-fused records summed in float64 on the host.
Per case: the maximum and the median of |got - exact| / exact over the lit components, the maximum of |got - exact| / bound
(accumulation_bound), the maximum |delta sRGB| of the tonemapped film against the oracle's tonemap of the exact film, and the
share of photons whose single loss the bound is certain to catch.
Usage (on a GPU machine): python tools/accumulation_depth.py > profiles/accumulation_depth.txt"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402
import _accumulation as A  # noqa: E402
import _oracle as O  # noqa: E402


def main():
    assert R.device_count() > 0, "accumulation_depth.py needs a GPU"
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    print("accumulation_depth: build %s, built-in scene, seed %d, stream %d, %d paths per film" % (R.build_id(), A.DEPTH_SEED, A.DEPTH_STREAM, A.PATHS))
    print("%-7s %-5s %-8s %12s %12s %12s %12s %8s" % ("film", "G", "mode", "max rel", "median rel", "max / bound", "max dsRGB", "single"))
    for w, h in A.DEPTH_SHAPES:
        path, records, _ = A.device_records(R, scene, w, h)
        _, idx, terms = A.lit_terms(w, h, records)
        for gathers in sorted(A.DEPTH_SPLITS, reverse=True):
            k, s, exact = A.film_terms(w, h, records, path // (A.PATHS // gathers), gathers)
            bound, exact = A.accumulation_bound(k, s), exact.sum(axis=0)
            _, want_srgb, _ = O.tonemap(exact.astype(np.float32), w, h)
            single = float(A.caught_if_lost(terms, idx, bound).mean())
            for fused in (True, False):
                g = A.run_depth_case(R, scene, w, h, fused, gathers)
                tm = R.TonemapUnit(w, h)
                tm.tonemap(g)
                f = A.error_figures(g.tristimulus_buffer, exact, bound, tm.srgb_float()[0], want_srgb)
                print("%-7s %-5d %-8s %12.3e %12.3e %12.4f %12.3e %8.3f" % ("%dx%d" % (w, h), gathers, "fused" if fused else "unfused", f["max_rel"],
                                                                         f["median_rel"], f["max_over_bound"], f["max_dsrgb"], single), flush=True)


if __name__ == "__main__":
    main()
