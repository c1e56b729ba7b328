"""What an occlusion query costs: Scene.occluded_device (rl_scene_occluded_device) against rl_scene_intersect_device on the same
rays.  Device forms, LDS fetch, everything resident.  Workloads, on the built-in scene with the camera rays of paths 0 .. n-1 at
1920x1080 from rl_scene_camera_rays_device (64 M by default):
  (a)  the camera rays, t_max = inf;
  (b)  shadow rays: from the camera rays' first hits (1e-5 off the surface, on the side the ray came from) towards a point on the
       largest black-body sphere, t_max the distance to it;
  (c)  rays from the first hits in uniform directions, t_max = 0.5;
  (c') workload (c) on the 20,019-object random scene of tools/spill_ab.py, camera rays at that tool's 1280x720 (--rays-big).
Candidates, each run in a process of its own per round, alternated --reps times after a warm-up round (median and min-max of the
host clock around one call that ends synchronised; every process makes one untimed call per workload first):
  baseline   rl_scene_intersect_device of the PARENT commit's library (--baseline: built with tools/build_alt.sh from a checkout of
             the parent, e.g. robigo_luculenta_amd/librl_alt_parent.so);
  intersect  rl_scene_intersect_device of this build, as a check that it did not move;
  occluded   rl_scene_occluded_device of this build.
The rays are made the same way in every process (same calls, same seeds), and the number of blocked rays of every workload must agree
between the three candidates.  Every GPU process runs under `timeout -k 10`, and the run stops at the first one that fails.
Acceptance (reported as within_bar / beats_bar, nothing is targeted): (a), (b): occluded median <= baseline median + the baseline's
min-max spread; (c), (c'): occluded median < baseline median - that spread.
Usage (on a GPU machine): python tools/occlusion_bench.py --baseline robigo_luculenta_amd/librl_alt_parent.so [--rays 67108864]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, os.path.join(HERE, ".."))

W, H = 1920, 1080
W_BIG, H_BIG = 1280, 720
SEED, STREAM = 1, 0
WORKLOADS = ("a", "b", "c", "c_big")
CANDIDATES = ("baseline", "intersect", "occluded")


def worker(candidate, library, n, n_big):
    """One process: makes the four workloads' rays, then one untimed and one timed call of the candidate on each."""
    import numpy as np
    import torch

    import robigo_luculenta_amd as R   # (host-side helpers and, unless --library names another, the library under test)
    from robigo_luculenta_amd import _lib
    import _random_scene as RS

    lib = R.lib
    if library:   # the parent's build: it has no occlusion entry points, so the package's loader cannot bind it
        assert candidate == "baseline"
        lib = C.CDLL(os.path.abspath(library))
        for name in ("rl_last_error", "rl_build_id", "rl_scene_create", "rl_scene_destroy", "rl_scene_camera_rays_device", "rl_scene_intersect_device"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]

    def check(rc):
        assert rc == 0, lib.rl_last_error()

    assert torch.cuda.is_available(), "occlusion_bench.py needs a GPU"
    dev = torch.device("cuda", 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    gen = torch.Generator(device=dev)

    def timed(fn):
        torch.cuda.synchronize()   # (the library runs on streams of its own: torch's work must be done before it reads a tensor)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def unit(k):
        v = torch.randn((k, 3), generator=gen, device=dev, dtype=torch.float32)
        return v / v.norm(dim=1, keepdim=True)

    out, blocked = {}, {}
    for big in (False, True):
        objs, cam = (RS.random_scene(35, n_spheres=20000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1) if big
                     else R.builtin_scene_desc(R.SCENE_DEMO))
        objs = np.ascontiguousarray(objs, dtype=R.OBJECT_DTYPE)
        desc = _lib.RlSceneDesc(len(objs), objs.ctypes.data_as(C.c_void_p), _lib.RlCameraDesc.from_buffer_copy(bytes(cam)))
        scene = C.c_void_p()
        check(lib.rl_scene_create(C.byref(desc), 0, C.byref(scene)))
        k = n_big if big else n
        gen.manual_seed(7 if big else 5)
        samples = torch.empty((k, 12), dtype=torch.float32, device=dev)   # RlCameraSample
        torch.cuda.synchronize()
        check(lib.rl_scene_camera_rays_device(scene, W_BIG if big else W, H_BIG if big else H, SEED, STREAM, 0, k, ptr(samples)))
        camera = samples[:, :8].contiguous()                               # RlRay: t_max in the wavelength's place
        del samples
        camera[:, 3] = float("inf")
        camera[:, 7] = 0.0
        hits = torch.empty((k, 12), dtype=torch.float32, device=dev)      # RlRayHit
        flags = torch.empty(k, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        check(lib.rl_scene_intersect_device(scene, R.FETCH_LDS, ptr(camera), k, ptr(hits)))
        torch.cuda.synchronize()
        hit = hits.view(torch.int32)[:, 10] != -1
        normal, d = hits[:, 3:6], camera[:, 4:7]
        side = torch.where((normal * d).sum(dim=1) > 0, -1.0, 1.0).to(torch.float32)
        start = torch.where(hit[:, None], hits[:, 0:3] + 1e-5 * side[:, None] * normal, camera[:, 0:3])   # (a miss keeps the camera's origin)
        del normal, d, side, hit

        def rays_of(direction, t_max):
            r = torch.zeros((k, 8), dtype=torch.float32, device=dev)
            r[:, 0:3], r[:, 3], r[:, 4:7] = start, t_max, direction
            return r

        work = {}
        if not big:
            work["a"] = camera
            lights = objs[(objs["material_kind"] == 0) & (objs["surface_kind"] == 0)]
            sun = lights[np.argmax(lights["f"][:, 0])]
            centre = torch.tensor(sun["v0"].tolist(), dtype=torch.float32, device=dev)
            to = centre[None, :] + float(sun["f"][0]) * unit(k) - start
            dist = to.norm(dim=1)
            work["b"] = rays_of(to / dist[:, None], dist)
            del to, dist
        work["c_big" if big else "c"] = rays_of(unit(k), 0.5)
        del start
        for name, rays in work.items():
            if candidate == "occluded":
                call = lambda: check(lib.rl_scene_occluded_device(scene, R.FETCH_LDS, ptr(rays), k, ptr(flags)))
            else:
                call = lambda: check(lib.rl_scene_intersect_device(scene, R.FETCH_LDS, ptr(rays), k, ptr(hits)))
            timed(call)
            out[name] = timed(call) * 1e3
            blocked[name] = int(flags.sum(dtype=torch.int64).item()) if candidate == "occluded" else int((hits.view(torch.int32)[:, 10] != -1).sum().item())
        del work, camera, hits, flags
        check(lib.rl_scene_destroy(scene))
    print(json.dumps({"candidate": candidate, "build_id": lib.rl_build_id().decode(), "ms": out, "blocked": blocked}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="the parent commit's library (tools/build_alt.sh)")
    ap.add_argument("--rays", type=int, default=1 << 26)
    ap.add_argument("--rays-big", type=int, default=16 * 524288)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a candidate's process may take")
    ap.add_argument("--worker", choices=CANDIDATES)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.baseline if args.worker == "baseline" else None, args.rays, args.rays_big)
    assert args.baseline and os.path.exists(args.baseline), "--baseline: the parent commit's library"
    assert args.reps >= 5, "alternate the candidates at least five times"
    import numpy as np

    times = {c: {w: [] for w in WORKLOADS} for c in CANDIDATES}
    build, blocked = {}, {}
    for rep in range(args.reps + 1):   # round 0 warms up
        for cand in CANDIDATES:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", cand, "--rays", str(args.rays),
                   "--rays-big", str(args.rays_big)] + (["--baseline", args.baseline] if cand == "baseline" else [])
            run = subprocess.run(cmd, capture_output=True, text=True)
            if run.returncode != 0:   # nothing more is started on the device after a failure
                sys.exit("round %d, %s: exit status %d; stopping.\n%s" % (rep, cand, run.returncode, run.stderr[-2000:]))
            res = json.loads(run.stdout.strip().splitlines()[-1])
            build[cand] = res["build_id"]
            assert blocked.setdefault("all", res["blocked"]) == res["blocked"], (cand, res["blocked"], blocked["all"])
            print("# round %d %-9s %s" % (rep, cand, " ".join("%s %.3f" % (w, res["ms"][w]) for w in WORKLOADS)), flush=True)
            if rep:
                for w in WORKLOADS:
                    times[cand][w].append(res["ms"][w])
    summary = lambda ts: {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    out = {"tool": "occlusion_bench", "build_id": build["occluded"], "baseline_build_id": build["baseline"], "fetch": "lds", "rays": args.rays,
           "rays_big": args.rays_big, "reps": args.reps, "workloads": {}}
    n_of = {"a": args.rays, "b": args.rays, "c": args.rays, "c_big": args.rays_big}
    for w in WORKLOADS:
        b, i, o = (summary(times[c][w]) for c in CANDIDATES)
        spread = b["max_ms"] - b["min_ms"]
        entry = {"n_rays": n_of[w], "blocked_share": round(blocked["all"][w] / n_of[w], 4), "baseline": b, "intersect": i, "occluded": o,
                 "occluded_over_baseline": round(o["median_ms"] / b["median_ms"], 4), "baseline_spread_ms": round(spread, 3)}
        if w in ("a", "b"):
            entry["within_bar"] = o["median_ms"] <= b["median_ms"] + spread
        else:
            entry["beats_bar"] = o["median_ms"] < b["median_ms"] - spread
        out["workloads"][w] = entry
        print("%-6s baseline %9.3f (%9.3f - %9.3f)  intersect %9.3f (%9.3f - %9.3f)  occluded %9.3f (%9.3f - %9.3f)  x%.3f  blocked %.1f %%" % (
            w, b["median_ms"], b["min_ms"], b["max_ms"], i["median_ms"], i["min_ms"], i["max_ms"], o["median_ms"], o["min_ms"], o["max_ms"],
            entry["occluded_over_baseline"], 100.0 * entry["blocked_share"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
