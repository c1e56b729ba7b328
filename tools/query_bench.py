"""Throughput of Scene.intersect's device path (rl_scene_intersect_device): queries per second of the blocking call on rays that
are already on the device, for camera-like rays (the built-in camera's position, directions through a 1920x1080 jittered grid in
row order, eight passes) and bounce-like rays (from those rays' hits, offset 1e-5 * direction, uniform directions), on the built-in
scene, the built-in scene with 1,500 seeds and the 20,000-sphere random scene of tools/spill_ab.py, in both fetch modes.  The time
of a call is its wall time (launch, kernel and the wait for it: the call returns when the hits are written), the median of --reps
calls after one warm-up call.  Prints one JSON line.  Usage (on a GPU machine): python tools/query_bench.py [--passes 8] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402
import _query_rays as QR  # noqa: E402
import _random_scene as RS  # noqa: E402

W, H = 1920, 1080


def rays_of(o, d):
    rays = np.zeros(len(o), dtype=R.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["t_max"] = o, d, np.inf
    return rays


def timed(scene, rays_dev, hits_dev, fetch, reps):
    before = R.query_launches()
    scene.intersect_device(rays_dev, hits_dev, fetch=fetch)   # warm-up (and the launch set-up of the variant)
    ran = [a - b for a, b in zip(R.query_launches(), before)]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        scene.intersect_device(rays_dev, hits_dev, fetch=fetch)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), next(i for i, r in enumerate(ran) if r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8, help="jittered passes over the 1920x1080 grid per call (8: 16.6 M rays)")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert R.device_count() > 0, "query_bench.py needs a GPU"
    scenes = [("built-in", R.builtin_scene_desc(R.SCENE_DEMO)),
              ("built-in, 1500 seeds", R.builtin_scene_desc(R.SCENE_DEMO, 1500)),
              ("random, 20000 spheres", RS.random_scene(35, n_spheres=20000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1))]
    rng = np.random.default_rng(1)
    results = []
    for name, (objs, cam) in scenes:
        scene = R.Scene(objs, cam)
        cams = [QR.camera_rays(cam, W, H, rng) for _ in range(args.passes)]
        o = np.concatenate([c[0] for c in cams])
        d = np.concatenate([c[1] for c in cams])
        del cams
        camera = rays_of(o, d)
        n = len(camera)
        rays_dev, hits_dev = QR.DeviceBuffer(camera.nbytes), QR.DeviceBuffer(n * R.HIT_DTYPE.itemsize)
        rays_dev.upload(camera)
        scene.intersect_device(rays_dev, hits_dev)
        hits = np.empty(n, dtype=R.HIT_DTYPE)
        hits_dev.download(hits)
        bo, bd = QR.bounce_rays(o, d, hits, rng)
        bounce = rays_of(bo, bd)
        del hits, o, d, bo, bd
        bounce_dev = QR.DeviceBuffer(bounce.nbytes)
        bounce_dev.upload(bounce)
        for kind, rays, dev in (("camera", camera, rays_dev), ("bounce", bounce, bounce_dev)):
            for fetch in (R.FETCH_LDS, R.FETCH_GLOBAL):
                s, variant = timed(scene, dev, hits_dev, fetch, args.reps)
                results.append({"scene": name, "objects": len(objs), "rays": kind, "fetch": "lds" if fetch == R.FETCH_LDS else "global",
                                "variant": variant, "n_rays": len(rays), "ms_per_call": round(s * 1e3, 3),
                                "gqueries_per_s": round(len(rays) / s / 1e9, 3)})
        del rays_dev, bounce_dev, hits_dev
    head = next(r for r in results if r["scene"] == "built-in" and r["rays"] == "camera" and r["fetch"] == "lds")
    print(json.dumps({"tool": "query_bench", "build_id": R.build_id(), "camera_builtin_lds_gqueries_per_s": head["gqueries_per_s"],
                      "results": results}))


if __name__ == "__main__":
    main()
