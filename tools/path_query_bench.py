"""Throughput of Scene.render_rays' device path (rl_scene_render_rays_device) against the trace kernel on the same paths.  On the
built-in scene at 1920x1080: rl_scene_camera_rays_device makes the camera rays of paths 0 .. n-1 (64 M by default) on the device,
a device-to-device 2-D copy packs their RlSpectralRay records, and rl_scene_render_rays_device traces them; then
rl_trace_unit_render_async + rl_trace_unit_sync renders the same paths with the trace kernel.  Each time is the host clock around
a call that ends synchronised, the median of --reps calls after one warm-up call of each.  Both give the same paths, so the same
segment count (checked).  Prints one JSON line: G segments/s and G paths/s of each, and their ratio.
Usage (on a GPU machine): python tools/path_query_bench.py [--paths 67108864] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402
import _query_rays as QR  # noqa: E402

W, H = 1920, 1080
SEED, STREAM = 1, 0


def median_time(fn, reps):
    fn()   # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fetch", choices=["lds", "global"], default="lds")
    args = ap.parse_args()
    assert R.device_count() > 0, "path_query_bench.py needs a GPU"
    n = args.paths
    fetch = R.FETCH_LDS if args.fetch == "lds" else R.FETCH_GLOBAL
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)

    samples = QR.DeviceBuffer(n * R.CAMERA_SAMPLE_DTYPE.itemsize)
    t0 = time.perf_counter()
    scene.camera_rays_device(W, H, SEED, STREAM, 0, samples)
    camera_s = time.perf_counter() - t0
    rays = QR.DeviceBuffer(n * R.SPECTRAL_RAY_DTYPE.itemsize)
    hip = QR.DeviceBuffer._hip
    # hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice): the first 32 bytes of every 48-byte sample
    assert hip.hipMemcpy2D(rays.ptr, C.c_size_t(32), samples.ptr, C.c_size_t(48), C.c_size_t(32), C.c_size_t(n), 3) == 0
    del samples
    results = QR.DeviceBuffer(n * R.PATH_RESULT_DTYPE.itemsize)

    before = R.path_launches()
    paths_s = median_time(lambda: scene.render_rays_device(rays, results, SEED, STREAM, 0, fetch=fetch), args.reps)
    variant = next(i for i, (a, b) in enumerate(zip(R.path_launches(), before)) if a != b)
    res = np.empty(n, dtype=R.PATH_RESULT_DTYPE)
    results.download(res)
    segments = int(res["segments"].sum(dtype=np.uint64))
    contributing = int((res["value"] != 0).sum())
    del res

    trace = R.TraceUnit(0, W, H, n_photons=n)
    trace.set_fetch(fetch)

    def render():
        trace.render_async(scene, SEED, STREAM, 0)
        trace.sync()

    trace_s = median_time(render, args.reps)
    t_paths, t_segments, t_ms = trace.stats()
    trace_segments = t_segments // (args.reps + 1)
    assert trace_segments == segments, (trace_segments, segments)
    out = {"tool": "path_query_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": args.fetch, "variant": variant,
           "paths": n, "segments": segments, "contributing": contributing, "camera_rays_ms": round(camera_s * 1e3, 3),
           "render_rays_ms": round(paths_s * 1e3, 3), "render_rays_gsegments_per_s": round(segments / paths_s / 1e9, 3),
           "render_rays_gpaths_per_s": round(n / paths_s / 1e9, 3), "trace_ms": round(trace_s * 1e3, 3),
           "trace_kernel_ms": round(t_ms / (args.reps + 1), 3), "trace_gsegments_per_s": round(segments / trace_s / 1e9, 3),
           "trace_gpaths_per_s": round(n / trace_s / 1e9, 3), "ratio": round(trace_s / paths_s, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
