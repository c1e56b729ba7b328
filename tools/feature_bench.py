"""What one persistent launch saves the denoising guides: Scene.render_features (rl_scene_render_features) against what a caller
wrote before it existed.  One process, the built-in scene, LDS fetch, 1280x720 films, paths 0 .. n-1 of the RNG for each n of
--paths (default 2^20 and 2^24).  Measured, each as the host clock around calls that end synchronised, after one warm-up round, the
candidates alternated --reps times (median and min-max):
  (a) features: rl_scene_render_features with all three units, no records;
  (b) loop: rl_scene_camera_rays_device, rl_scene_begin_paths_device, then rl_scene_step_path_list_device(RL_STEP_NO_ROULETTE, hits)
      over the paths still in their chain with the classification and the compaction of the list in torch between the steps, and
      index_add_ of the three films' terms at the end;
  (c) records: (a) with records only and no film -- the difference to (a) prices the atomics;
  (d) plain: rl_plot_unit_render_samples_device on the same camera samples -- the render itself, as the scale.
Checked in the run: (a)'s films and (b)'s both lie within the per-pixel splat bound of the exact (float64) sum of (b)'s terms, and
(a)'s stats equal the counts from (b)'s records.
The acceptance: (a)'s median is not above (b)'s median plus (b)'s own min-max spread, at every size.  Prints one JSON line per size.
Usage (on a GPU machine): python tools/feature_bench.py [--paths 1048576 16777216] [--reps 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H = 1280, 720
SEED, STREAM = 1, 0
FILMS = ("albedo", "normal", "aux")


def timed(fn):
    torch.cuda.synchronize()   # (the library runs on streams of its own: torch's work must be done before it reads a tensor)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts, n):
    s = {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}
    s["mpaths_per_s"] = round(n / (s["median_ms"] * 1e-3) / 1e6, 3)
    return s


def cie_table(dev):
    """The CIE 1931 table the library splats with (cie1931.rs), (81, 3) float32."""
    tab = json.load(open(os.path.join(ROOT, "tests", "golden", "cie1931_xyz.json")))
    return torch.tensor(np.stack([np.array(tab[k], np.float32) for k in "XYZ"], axis=1), device=dev)


def tristimulus(cie, wl):
    """cie1931.rs:20-48 for a float32 tensor of wavelengths: (n, 3)."""
    indexf = (wl - 380.0) / torch.full_like(wl, 5.0)      # (a tensor: torch turns a division by a scalar into a product with its reciprocal)
    fl = torch.floor(indexf)
    ok = torch.isfinite(fl) & (fl >= -1) & (fl <= 80)
    index = torch.where(ok, fl, torch.zeros_like(fl)).long()
    rem = (indexf - index.float())[:, None]
    inner = cie[index.clamp(0, 80)] * (1.0 - rem) + cie[(index + 1).clamp(0, 80)] * rem
    out = torch.where((index == -1)[:, None], cie[0][None, :] * rem, torch.where((index == 80)[:, None], cie[80][None, :] * (1.0 - rem), inner))
    return torch.where(ok[:, None], out, torch.zeros_like(out))


def splat_terms(w, h, x, y, colours):
    """plot_unit.rs:56-84 for samples that bring their colour: pixel indices (n, 4) and float32 terms (n, 4, 3)."""
    aspect = float(np.float32(w) / np.float32(h))
    px = (x * 0.5 + 0.5) * float(w - 1)
    py = (y * aspect * 0.5 + 0.5) * float(h - 1)
    px1, px2 = torch.floor(px).long().clamp(0, w - 1), torch.ceil(px).long().clamp(0, w - 1)
    py1, py2 = torch.floor(py).long().clamp(0, h - 1), torch.ceil(py).long().clamp(0, h - 1)
    cx, cy = px - px1.float(), py - py1.float()
    wts = torch.stack([(1.0 - cx) * (1.0 - cy), cx * (1.0 - cy), (1.0 - cx) * cy, cx * cy], dim=1)
    idx = torch.stack([py1 * w + px1, py1 * w + px2, py2 * w + px1, py2 * w + px2], dim=1)
    return idx, colours[:, None, :] * wts[:, :, None]


def film_terms(cie, rec, w, h):
    """{film: (idx (m, 4), terms (m, 4, 3))} of the three films for the records of the loop (a dict of per-path tensors)."""
    surface = (rec["kind"] == R.FEATURE_EMITTER) | (rec["kind"] == R.FEATURE_DIFFUSE)
    on = rec["albedo"] != 0
    out = {"albedo": splat_terms(w, h, rec["x"][on], rec["y"][on], tristimulus(cie, rec["wavelength"][on]) * rec["albedo"][on][:, None]),
           "normal": splat_terms(w, h, rec["x"][surface], rec["y"][surface], rec["normal"][surface])}
    aux = torch.stack([torch.ones_like(rec["depth"]), rec["depth"], rec["segments"].float()], dim=1)
    out["aux"] = splat_terms(w, h, rec["x"], rec["y"], aux)
    return out


def loop_records(scene, materials, n, dev, cam, max_segments=R.RL_FEATURE_MAX_SEGMENTS):
    """(b) up to the films: the feature records of paths 0 .. n-1 from the public device calls, as a dict of per-path tensors."""
    scene.camera_rays_device(W, H, SEED, STREAM, 0, cam)
    rays = cam[:, :8].contiguous()                                     # RlSpectralRay
    states = torch.empty((n, 16), dtype=torch.float32, device=dev)     # RlPathState
    hits = torch.empty((n, 12), dtype=torch.float32, device=dev)       # RlRayHit
    torch.cuda.synchronize()
    scene.begin_paths_device(rays, states, 0)
    end, intensity = states[:, 10].view(torch.int32), states[:, 7]
    hit_object = hits[:, 10].view(torch.int32)
    rec = {"x": cam[:, 8], "y": cam[:, 9], "wavelength": cam[:, 3],
           "albedo": torch.zeros(n, device=dev), "normal": torch.zeros((n, 3), device=dev), "depth": torch.zeros(n, device=dev),
           "segments": torch.zeros(n, dtype=torch.int32, device=dev), "kind": torch.zeros(n, dtype=torch.int32, device=dev)}
    lst = torch.arange(n, dtype=torch.int32, device=dev)
    for segment in range(1, max_segments + 1):
        n_list = int(lst.numel())
        if n_list == 0:
            break
        rows = lst.long()
        arriving = states[rows, 4:7]                                   # the state's direction before the step
        torch.cuda.synchronize()
        scene.step_path_list_device(states, SEED, STREAM, lst, n_list, None, flags=R.RL_STEP_NO_ROULETTE, hits=hits)
        obj = hit_object[rows]
        found = obj != -1                                              # RL_OBJECT_NONE
        if segment == 1:
            rec["depth"] = torch.where(found, hits[:, 9], torch.zeros_like(hits[:, 9]))
        material = torch.where(found, materials[obj.clamp(0, materials.numel() - 1).long()], torch.full_like(obj, -1))
        kind = torch.full_like(obj, R.FEATURE_LIMIT if segment == max_segments else -1)
        kind[(material == 1) | (material == 2)] = R.FEATURE_DIFFUSE   # RL_MATERIAL_DIFFUSE_GREY, RL_MATERIAL_DIFFUSE_COLOURED
        kind[end[rows] == R.RL_PATH_END_EMITTER] = R.FEATURE_EMITTER
        kind[end[rows] == R.RL_PATH_END_VOID] = R.FEATURE_VOID
        done = kind >= 0
        at = rows[done]
        surface = (kind[done] == R.FEATURE_EMITTER) | (kind[done] == R.FEATURE_DIFFUSE)
        nrm, d = hits[at, 3:6], arriving[done]
        facing = d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1] + d[:, 2] * nrm[:, 2] < 0
        rec["kind"][at], rec["segments"][at] = kind[done], segment
        rec["albedo"][at] = torch.where(surface, intensity[at], torch.zeros_like(intensity[at]))
        rec["normal"][at] = torch.where(surface[:, None], torch.where(facing[:, None], nrm, -nrm), torch.zeros_like(nrm))
        lst = lst[~done].contiguous()                                  # the compaction
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert R.device_count() > 0 and torch.cuda.is_available(), "feature_bench.py needs a GPU"
    assert args.reps >= 5, "alternate the candidates at least five times"
    dev = torch.device("cuda", 0)
    scene = R.Scene.builtin(R.SCENE_DEMO)
    objs = np.ascontiguousarray(R.builtin_scene_desc(R.SCENE_DEMO)[0]).view(R.OBJECT_DTYPE)
    materials = torch.from_numpy(objs["material_kind"].astype(np.int32)).to(dev)
    cie = cie_table(dev)
    plots_a = [R.PlotUnit(k, W, H) for k in range(3)]
    plot_d = R.PlotUnit(3, W, H)

    for n in args.paths:
        cam = torch.empty((n, 12), dtype=torch.float32, device=dev)        # RlCameraSample
        records = torch.empty((n, 12), dtype=torch.float32, device=dev)    # RlFeatureSample: (c)'s 48 bytes per path
        films_b = {name: torch.zeros((W * H, 3), dtype=torch.float32, device=dev) for name in FILMS}
        torch.cuda.synchronize()
        stats, kept = {}, {}

        def features():
            stats.update(scene.render_features(W, H, SEED, STREAM, 0, n, albedo=plots_a[0], normal=plots_a[1], aux=plots_a[2]))

        def loop():
            rec = loop_records(scene, materials, n, dev, cam)
            for name, (idx, terms) in film_terms(cie, rec, W, H).items():
                films_b[name].index_add_(0, idx.reshape(-1), terms.reshape(-1, 3))
            kept["rec"] = rec

        def records_only():
            scene.render_features(W, H, SEED, STREAM, 0, n, records=records)

        def plain():
            plot_d.render_samples_device(scene, cam, SEED, STREAM, 0)

        candidates = {"features": features, "loop": loop, "records": records_only, "plain": plain}
        times = {k: [] for k in candidates}
        check = {}
        for rep in range(args.reps + 1):   # round 0 warms up
            if rep == 1:                   # the check below compares one call of each onto cleared films
                for p in plots_a:
                    p.clear()
                for f in films_b.values():
                    f.zero_()
            for name, fn in candidates.items():
                t = timed(fn)
                if rep:
                    times[name].append(t)
                if rep == 1 and name == "loop":
                    rec = kept["rec"]
                    kinds = torch.bincount(rec["kind"].long(), minlength=4)
                    check["loop_stats"] = {"paths": n, "segments": int(rec["segments"].long().sum().item()), "kinds": [int(k) for k in kinds.tolist()]}
                    worst = {}
                    for (name_f, (idx, terms)), plot in zip(film_terms(cie, rec, W, H).items(), plots_a):
                        idx, t64 = idx.reshape(-1), terms.reshape(-1, 3).double()
                        exact = torch.zeros((W * H, 3), dtype=torch.float64, device=dev).index_add_(0, idx, t64)
                        s = torch.zeros_like(exact).index_add_(0, idx, t64.abs())
                        k = torch.zeros_like(exact).index_add_(0, idx, (t64 != 0).double())
                        bound = (k - 1).clamp(min=0) * 2.0 ** -24 * s * (1 + 1e-6)
                        fa = torch.from_numpy(plot.tristimulus_buffer).to(dev).double()
                        worst[name_f] = {"a_violations": int(((fa - exact).abs() > bound).sum().item()),
                                         "b_violations": int(((films_b[name_f].double() - exact).abs() > bound).sum().item()),
                                         "a_gap_of_max": float(((fa - exact).abs().max() / exact.abs().max()).item()),
                                         "max_terms": int(k.max().item())}
                    check["films"] = worst
            kept.clear()
        within = all(f["a_violations"] == 0 and f["b_violations"] == 0 for f in check["films"].values())
        a, b, c, d = (summary(times[k], n) for k in ("features", "loop", "records", "plain"))
        bar = b["median_ms"] + (b["max_ms"] - b["min_ms"])
        print(json.dumps({"tool": "feature_bench", "build_id": R.build_id(), "scene": "built-in", "fetch": "lds", "film_size": [W, H], "paths": n,
                          "reps": args.reps, "features": a, "loop": b, "records": c, "plain": d, "a_bar_ms": round(bar, 3),
                          "a_within_bar": a["median_ms"] <= bar, "loop_over_features": round(b["median_ms"] / a["median_ms"], 4),
                          "atomics_ms": round(a["median_ms"] - c["median_ms"], 3), "features_over_plain": round(a["median_ms"] / d["median_ms"], 4),
                          "films_within_bound": within, "films": check["films"], "stats": stats, "stats_equal": stats == check["loop_stats"]}), flush=True)
        # (after the line, so that a failed check still leaves the figures)
        assert stats == check["loop_stats"], "rl_scene_render_features' stats and the loop's counts disagree: %r against %r" % (stats, check["loop_stats"])
        assert within, "a film is not within the per-pixel bound of the exact sum of the loop's terms: %r" % (check["films"],)
        del cam, records, films_b


if __name__ == "__main__":
    main()
