"""What a wavefront step costs: Scene.step_paths_device (rl_scene_step_paths_device) against the query and the path kernel on the
same rays.  One process, the built-in scene, LDS fetch, device forms with everything resident: rl_scene_camera_rays_device makes
the camera rays of paths 0 .. n-1 at 1920x1080 (64 M by default, as tools/path_query_bench.py), rl_scene_begin_paths_device their
states.  Measured, each as the host clock around calls that end synchronised, after one warm-up round, the candidates alternated
--reps times (median and min-max):
  (a) one step of every state on its first segment with hits = NULL, against rl_scene_intersect_device on the same rays.  The
      step does the query's scan plus a bounce and the emitter term, which the path kernel's region timers put at
      (5.4 + 2.5) / 18.1 = 0.44 of the scan's cycles: the bar is 1.44 x the query's median plus the min-max
      spread of the query's own runs.
  (b) the same step with hits written, as a ratio to (a).
  (c) the whole wavefront loop to the last live path -- step, keep the live states by torch indexing, step again -- against
      rl_scene_render_rays_device on the same rays; its final states are checked against that call's results.  Reported only.
  (d) list_step: one listed step of every state (rl_scene_step_path_list_device, the identity list, live_list written, hits =
      NULL) against (a)'s step in the same run.  It moves at most (128 + 16) / 128 = 1.125 x the step's bytes per state and does
      the same arithmetic: the bar is 1.125 x the step's median plus the step's min-max spread.
  (e) wavefront_list: the whole loop through rl_scene_step_path_list_device, two index buffers taking turns as list and
      live_list, the states staying where they are; final states checked as (c)'s.  Against (c)'s wavefront, the torch-compaction
      loop: its median must be below wavefront's by more than wavefront's own min-max spread.  Both as ratios to render_rays.
The variant reported is the step kernel's; the list-step kernel runs the same one (one scene, one fetch mode).
Prints one JSON line.  Usage (on a GPU machine): python tools/step_bench.py [--paths 67108864] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H = 1920, 1080
SEED, STREAM = 1, 0
END_WORD = 10   # RlPathState::end, in 32-bit words


def timed(fn):
    torch.cuda.synchronize()   # (the library runs on streams of its own: torch's work must be done before it reads a tensor)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1 << 26)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert R.device_count() > 0 and torch.cuda.is_available(), "step_bench.py needs a GPU"
    assert args.reps >= 5, "alternate the candidates at least five times"
    n, dev = args.paths, torch.device("cuda", 0)
    scene = R.Scene.builtin(R.SCENE_DEMO)

    samples = torch.empty((n, 12), dtype=torch.float32, device=dev)   # RlCameraSample
    torch.cuda.synchronize()
    scene.camera_rays_device(W, H, SEED, STREAM, 0, samples)
    rays = samples[:, :8].contiguous()                                # RlSpectralRay
    del samples
    query_rays = rays.clone()                                         # RlRay: t_max in the wavelength's place
    query_rays[:, 3] = float("inf")
    begun = torch.empty((n, 16), dtype=torch.int32, device=dev)       # RlPathState
    work = torch.empty_like(begun)
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)      # RlRayHit
    results = torch.empty((n, 4), dtype=torch.int32, device=dev)      # RlPathResult
    torch.cuda.synchronize()
    scene.begin_paths_device(rays, begun, 0)

    def reset():
        work.copy_(begun)

    def wavefront():
        """The loop of (c): returns the number of steps and leaves the final states, scattered back by path index, in `work`."""
        live = work
        steps = 0
        while live.shape[0]:
            torch.cuda.synchronize()
            scene.step_paths_device(live, SEED, STREAM)
            steps += 1
            ended = live[:, END_WORD] != -1
            done = live[ended]
            if live is not work:
                work[done[:, 12].long()] = done   # path_index < 2^31 here: its low word is the row
            live = live[~ended].contiguous()
        return steps

    ping = torch.empty(n, dtype=torch.int32, device=dev)
    pong = torch.empty(n, dtype=torch.int32, device=dev)

    def wavefront_list():
        """The loop of (e): returns the number of steps; the final states are in `work`, where they always were."""
        lst, out, n_list, steps = None, ping, n, 0
        while n_list and steps < R.RL_PATH_MAX_SEGMENTS:   # (render_rays ends every path by then)
            n_list = scene.step_path_list_device(work, SEED, STREAM, lst, n_list, out)
            steps += 1
            lst, out = out, (pong if out is ping else ping)
        return steps

    def check_against_results(what):
        torch.cuda.synchronize()
        same = bool((work[:, [11, 9, 14, 10]] == results).all().item())   # value, segments, object, end
        assert same, "the %s loop and rl_scene_render_rays_device disagree" % what
        return same

    candidates = {
        "query": lambda: scene.intersect_device(query_rays, hits),
        "step": lambda: scene.step_paths_device(work, SEED, STREAM),
        "step_hits": lambda: scene.step_paths_device(work, SEED, STREAM, hits=hits),
        "render_rays": lambda: scene.render_rays_device(rays, results, SEED, STREAM, 0),
        "wavefront": wavefront,
        "list_step": lambda: scene.step_path_list_device(work, SEED, STREAM, None, n, ping),
        "wavefront_list": wavefront_list,
    }
    times = {k: [] for k in candidates}
    before = R.step_launches()
    steps = {}
    for rep in range(args.reps + 1):   # round 0 warms up
        for name, fn in candidates.items():
            reset()
            if name in ("wavefront", "wavefront_list"):
                box = []
                t = timed(lambda: box.append(fn()))
                steps[name] = box[0]
                if name == "wavefront_list" and rep in (0, args.reps):
                    check_against_results(name)   # (results: render_rays has run in this round)
            else:
                t = timed(fn)
            if rep:
                times[name].append(t)
    reset()
    steps["wavefront"] = wavefront()   # (c)'s check below reads `work`: the last candidate above left its own states there
    variant = next(i for i, (a, b) in enumerate(zip(R.step_launches(), before)) if a != b)

    # (c)'s final states against the path kernel's results: value, segments, object, end
    same = check_against_results("wavefront")
    segments = int(results[:, 1].sum(dtype=torch.int64).item())

    q, a, b = summary(times["query"]), summary(times["step"]), summary(times["step_hits"])
    r, c = summary(times["render_rays"]), summary(times["wavefront"])
    d, e = summary(times["list_step"]), summary(times["wavefront_list"])
    bar = 1.44 * q["median_ms"] + (q["max_ms"] - q["min_ms"])
    d_bar = 1.125 * a["median_ms"] + (a["max_ms"] - a["min_ms"])
    c_spread = c["max_ms"] - c["min_ms"]
    out = {"tool": "step_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": "lds", "variant": variant, "paths": n,
           "reps": args.reps, "segments": segments, "query": q, "step": a, "step_hits": b, "render_rays": r, "wavefront": c,
           "wavefront_steps": steps["wavefront"], "a_step_over_query": round(a["median_ms"] / q["median_ms"], 4), "a_bar_ms": round(bar, 3),
           "a_within_bar": a["median_ms"] <= bar, "b_hits_over_step": round(b["median_ms"] / a["median_ms"], 4),
           "c_wavefront_over_render_rays": round(c["median_ms"] / r["median_ms"], 4), "wavefront_equals_render_rays": same,
           "list_step": d, "wavefront_list": e, "wavefront_list_steps": steps["wavefront_list"],
           "d_list_step_over_step": round(d["median_ms"] / a["median_ms"], 4), "d_bar_ms": round(d_bar, 3), "d_within_bar": d["median_ms"] <= d_bar,
           "e_wavefront_list_over_wavefront": round(e["median_ms"] / c["median_ms"], 4), "e_wavefront_spread_ms": round(c_spread, 3),
           "e_below_wavefront_by_more_than_its_spread": e["median_ms"] < c["median_ms"] - c_spread,
           "e_wavefront_list_over_render_rays": round(e["median_ms"] / r["median_ms"], 4), "wavefront_list_equals_render_rays": True}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
