#!/usr/bin/env python3
"""Where the path kernel's time goes, next to the trace kernel's on the same paths (diagnostic build `make -C
robigo_luculenta_amd/csrc stats`, -DRL_STATS: s_memtime region timers and event counts summed over all waves, read with
rl_stats_read).  The built-in scene at 1920x1080: rl_scene_camera_rays_device makes the camera rays of `n` paths, a 2-D copy packs
them, rl_scene_render_rays_device traces them (the path kernel), then rl_trace_unit_render_async renders the same paths (the
trace kernel).  Prints wave cycles per iteration by region for each kernel, and one JSON line.  The timers' reads wait for
outstanding loads, so this build runs slower than the product; compare shares, not absolute rates.
Usage (GPU box): python tools/path_kernel_stats.py [n_paths=16777216]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["RL_LIBRARY"] = os.path.join(ROOT, "robigo_luculenta_amd", "librobigo_luculenta_stats.so")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import robigo_luculenta_amd as R  # noqa: E402
from robigo_luculenta_amd import _lib  # noqa: E402
import _query_rays as QR  # noqa: E402

NAMES = ["iter", "scan_lanes", "a_rounds", "a_lanes", "b_rounds", "b_lanes", "p_rounds", "p_lanes", "shade_diffuse",
         "shade_glass", "shade_soap", "end_emitter", "end_void", "any_glass", "any_soap", "any_coloured", "any_glossy",
         "refills", "emit_batches", "emit_lanes", "a_items", "p_items", "any_diffuse", "s_rounds", "s_lanes", "s_items", "p_slow",
         "t_total", "t_refill", "t_small", "t_direct", "t_cluster", "t_tail", "t_prism", "t_shade", "t_emit", "t_a_rounds",
         "t_b_rounds", "t_p_rounds", "t_camera", "t_s_rounds", "x_lanes", "x_iters", "t_exhaustive"]
# (label, counter): the scan's regions are the same code in both kernels; t_camera is rl_begin_path in the trace kernel and the
# new rays' loads + their SF10 index in the path kernel; t_emit is the emitter queue + records in the trace kernel and the emitter
# term + result stores in the path kernel.
ROWS = (("refill (hand-out of new paths)", "t_refill"), ("  of which camera rays / ray loads + SF10", "t_camera"),
        ("planes / circles / paraboloids", "t_small"), ("direct spheres", "t_direct"), ("cluster culls + rounds", "t_cluster"),
        ("final sphere-tail flush", "t_tail"), ("prism culls + CSG rounds", "t_prism"), ("exact linear scans (path kernel only)", "t_exhaustive"),
        ("bounce (hit completion, material, roulette)", "t_shade"), ("emitter term + results", "t_emit"))
W, H = 1920, 1080


def counters(read, buf):
    assert read(buf, 48) == 0
    return dict(zip(NAMES, list(buf)))


def report(name, c):
    it, tt = float(c["iter"]), float(c["t_total"])
    print("%s: %d wave-iterations, %.1f active lanes per iteration (of 64), %.0f wave cycles per iteration"
          % (name, c["iter"], c["scan_lanes"] / it, tt / it))
    for label, key in ROWS:
        print("    %-46s %5.1f %%  (%6.0f cycles per iteration)" % (label, 100.0 * c[key] / tt, c[key] / it))
    print("    linear scans: %.3f lanes per iteration, in %.1f %% of iterations" % (c["x_lanes"] / it, 100.0 * c["x_iters"] / it))
    scanned = c["t_small"] + c["t_direct"] + c["t_cluster"] + c["t_tail"] + c["t_prism"]
    out = {"iterations": c["iter"], "lanes_per_iteration": round(c["scan_lanes"] / it, 2), "cycles_per_iteration": round(tt / it),
           "scan_cycles_per_iteration": round(scanned / it), "untimed_share": round(1.0 - (c["t_refill"] + scanned + c["t_exhaustive"] + c["t_shade"] + c["t_emit"]) / tt, 4),
           "exhaustive_lanes_per_iteration": round(c["x_lanes"] / it, 4), "exhaustive_iteration_share": round(c["x_iters"] / it, 4)}
    for label, key in ROWS:
        out[key + "_per_iteration"] = round(c[key] / it)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 24
    assert R.device_count() > 0, "path_kernel_stats.py needs a GPU"
    read = _lib.lib.rl_stats_read
    read.restype, read.argtypes = C.c_int, [C.POINTER(C.c_uint64), C.c_int]
    buf = (C.c_uint64 * 48)()
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    samples = QR.DeviceBuffer(n * R.CAMERA_SAMPLE_DTYPE.itemsize)
    scene.camera_rays_device(W, H, 1, 0, 0, samples)
    rays = QR.DeviceBuffer(n * R.SPECTRAL_RAY_DTYPE.itemsize)
    assert QR.DeviceBuffer._hip.hipMemcpy2D(rays.ptr, C.c_size_t(32), samples.ptr, C.c_size_t(48), C.c_size_t(32), C.c_size_t(n), 3) == 0
    del samples
    results = QR.DeviceBuffer(n * R.PATH_RESULT_DTYPE.itemsize)
    trace = R.TraceUnit(0, W, H, n_photons=n)
    scene.render_rays_device(rays, results, 1, 0, 0)   # warm-up of both
    trace.render_async(scene, 1, 0, 0)
    trace.sync()
    counters(read, buf)
    scene.render_rays_device(rays, results, 1, 0, 0)
    path = report("path kernel", counters(read, buf))
    trace.render_async(scene, 1, 0, 0)
    trace.sync()
    tr = report("trace kernel", counters(read, buf))
    print(json.dumps({"tool": "path_kernel_stats", "paths": n, "path_kernel": path, "trace_kernel": tr}))


if __name__ == "__main__":
    main()
