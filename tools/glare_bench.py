"""What the glare unit costs.  One process on one MI355X, 1280 x 720, the demo scene's spectral film of --paths paths; one shape
(--nodes, --taps) per run, --warmup warm-ups and --reps repetitions, the calls of the comparison alternated in the same run; every
figure is a median (min - max) in milliseconds from events around the work itself.
  apply      rl_glare_unit_apply with the tables of rl_glare_kernels_scaled (the veil, strength 0.3), the CIE observer: the events
             around its launch (rl_debug_glare_ms).
  project    rl_spectral_unit_project of the same film under the same observer (rl_debug_spectral_ms): the K = 1 floor.
  copy       a device copy of as many bytes as the film has: what apply must at least read.
  torch      what a user would write today on the same data on the same device: a depthwise conv2d (groups = n_nodes, padding = R)
             over the cube, then the (pixels, n_nodes) x (n_nodes, 3) matmul; torch events around the two.  Its result is compared with
             apply's (the largest difference over the largest value: the two sum in different orders, so not bit for bit).
  floor      2 K^2 n_nodes pixels / 78.6e12 s, the un-fused vector rate (half the 157.3 TF peak of packed f32 multiply-add), and
             apply's share of it.
The bar: apply's median <= the torch composition's median.  A bar that is missed is written as it came out.  Prints one JSON line
and appends it to --out if given.
Usage (on a GPU machine): python tools/glare_bench.py --nodes 16 --taps 33 [--reps 7] [--out profiles/glare_bench.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import robigo_luculenta_amd as R  # noqa: E402

W, H = 1280, 720
VECTOR_FLOPS = 78.6e12


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--taps", type=int, required=True)
    ap.add_argument("--paths", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch composition out (the bar is then not evaluated)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, K = a.nodes, a.taps
    assert R.device_count() > 0 and torch.cuda.is_available(), "glare_bench needs a GPU: nothing here is measured without one"

    scene = R.Scene.builtin(R.SCENE_DEMO)
    trace = R.TraceUnit(0, W, H, n_photons=a.paths)
    trace.render(scene, seed=1, stream=0, first_path_index=0)
    spectral, glare, dst, plain = R.SpectralUnit(W, H, n), R.GlareUnit(W, H, n, K), R.GatherUnit(W, H), R.GatherUnit(W, H)
    spectral.plot([trace])
    side = min(2 * K - 1, 65)
    tables = R.glare_kernels_scaled(R.glare_psf_veil(side, 4.0), 550.0, n, 0.3, K)
    glare.set_kernels(tables)
    observer = R.spectral_observer_cie1931(n)

    cube = torch.from_numpy(spectral.download()).cuda().reshape(1, n, H, W)
    weight = torch.from_numpy(tables).cuda().reshape(n, 1, K, K)
    matrix = torch.from_numpy(observer).cuda()
    src = torch.zeros(n * W * H, dtype=torch.float32, device="cuda")
    into = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def torch_composition():
        blurred = torch.nn.functional.conv2d(cube, weight, padding=K // 2, groups=n)
        return blurred.reshape(n, H * W).t() @ matrix

    t = {"apply": [], "project": [], "copy": [], "torch": []}
    result = None
    for k in range(a.warmup + a.reps):
        glare.apply(spectral, observer, dst)
        spectral.project(observer, plain)
        ev[0].record()
        into.copy_(src)
        ev[1].record()
        if not a.no_torch:
            ev[2].record()
            result = torch_composition()
            ev[3].record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            t["apply"].append(glare.launch_ms())
            t["project"].append(spectral.launch_ms()[1])
            t["copy"].append(ev[0].elapsed_time(ev[1]))
            if not a.no_torch:
                t["torch"].append(ev[2].elapsed_time(ev[3]))
    s = {name: spread(xs) for name, xs in t.items() if xs}
    floor_ms = 2.0 * K * K * n * W * H / VECTOR_FLOPS * 1e3
    fields = dict(what="glare apply", size="%dx%d" % (W, H), nodes=n, taps=K, paths=a.paths, reps=a.reps, build=R.build_id(),
                  apply_ms=s["apply"], project_ms=s["project"], film_mb=round(n * W * H * 4 / 1e6, 1), device_copy_ms=s["copy"],
                  apply_over_project=round(s["apply"]["median"] / s["project"]["median"], 2),
                  apply_over_device_copy=round(s["apply"]["median"] / s["copy"]["median"], 2),
                  floor_ms=round(floor_ms, 4), share_of_floor=round(floor_ms / s["apply"]["median"], 4),
                  achieved_tflops=round(2.0 * K * K * n * W * H / (s["apply"]["median"] * 1e-3) / 1e12, 2))
    if not a.no_torch:
        got = dst.tristimulus_buffer.reshape(H * W, 3).astype(np.float64)
        ref = result.cpu().numpy().astype(np.float64)
        fields.update(torch_conv2d_matmul_ms=s["torch"], bar="apply median <= torch composition median",
                      met=bool(s["apply"]["median"] <= s["torch"]["median"]),
                      torch_over_apply=round(s["torch"]["median"] / s["apply"]["median"], 2),
                      largest_difference_over_largest_value=float(np.abs(got - ref).max() / np.abs(ref).max()), torch=torch.__version__)
    line = json.dumps(fields)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
