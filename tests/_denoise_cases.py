"""Inputs of the denoiser's tests (tests/test_denoise.py, tests/test_gpu_denoise.py): shapes, image classes, guide classes and
parameter sets, all deterministic.  Images and films are (h, w, 3) float32.  Test-only."""
import numpy as np

# (w, h): every tap but the centre outside; one pixel wide; one pixel high; a small square; one past a 16 x 16 tile either way;
# steps 16 and 32 exceed the image; several tiles, and partial residue classes at every step
SHAPES = [(1, 1), (1, 7), (5, 1), (3, 3), (17, 16), (16, 17), (33, 19), (67, 35)]
IMAGES = ["loguniform", "constant", "zeros", "nonfinite"]
GUIDES = ["random", "halfplanes", "depth_steps", "checker", "dead", "no_albedo", "no_normal", "no_aux"]
PARAMS = {
    "defaults": {},
    "colour_alone": dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
    "normal_alone": dict(sigma_colour=0.0, sigma_depth=0.0, sigma_albedo=0.0),
    "depth_alone": dict(sigma_colour=0.0, sigma_normal=0.0, sigma_albedo=0.0),
    "albedo_alone": dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0),
    "all_off": dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
    "one_pass": dict(iterations=1),
    "six_passes": dict(iterations=6),
    "sigmas_smallest": dict(sigma_colour=1e-3, sigma_normal=1e-3, sigma_depth=1e-3, sigma_albedo=1e-3),
    "sigmas_largest": dict(sigma_colour=1e3, sigma_normal=1e3, sigma_depth=1e3, sigma_albedo=1e3),
}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))   # (hash() of a string changes from process to process)


def image(kind, w, h):
    g = np.random.default_rng([_seed(kind), w, h])
    if kind == "zeros":
        return np.zeros((h, w, 3), np.float32)
    if kind == "constant":
        return np.full((h, w, 3), 0.75, np.float32)
    out = np.exp(g.uniform(np.log(1e-3), np.log(1e3), (h, w, 3))).astype(np.float32)
    if kind == "nonfinite":
        flat = out.reshape(-1, 3)
        where = g.permutation(len(flat))[:min(3, len(flat))]
        for value, p in zip((np.inf, np.nan, -np.inf), where):
            flat[p, g.integers(0, 3)] = value
            if len(flat) > 8:
                flat[p, 1] = value      # (the luminance too, where the image is large enough to have finite pixels beside it)
    return out


def guides(kind, w, h):
    """{albedo, normal, aux}: the tristimulus buffers of the three guide gather units, or None for a unit that is not given."""
    g = np.random.default_rng([_seed(kind if not kind.startswith("no_") and kind not in ("checker", "dead") else "random"), w, h])
    weight = g.uniform(0.5, 4.0, (h, w, 1)).astype(np.float32)
    direction = g.normal(size=(h, w, 3))
    direction /= np.linalg.norm(direction, axis=2, keepdims=True)
    depth = g.uniform(0.5, 20.0, (h, w, 1)).astype(np.float32)
    colour = g.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    segments = g.integers(1, 6, (h, w, 1)).astype(np.float32)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    if kind == "halfplanes":
        weight = np.ones((h, w, 1), np.float32)
        direction = np.zeros((h, w, 3))
        direction[..., 2] = np.where(xs < (w + 1) // 2, 1.0, -1.0)
        depth = np.full((h, w, 1), 2.0, np.float32)
        colour = np.full((h, w, 3), 0.5, np.float32)
    elif kind == "depth_steps":
        direction = np.zeros((h, w, 3))
        direction[..., 1] = 1.0
        depth = (1.0 + 3.0 * ((xs // 3 + ys // 2) % 4))[..., None].astype(np.float32)
        colour = np.full((h, w, 3), 0.25, np.float32)
    elif kind == "checker":
        weight = weight * ((xs + ys) % 2)[..., None].astype(np.float32)
    elif kind == "dead":
        weight = np.zeros((h, w, 1), np.float32)
    out = {"albedo": (colour * weight).astype(np.float32), "normal": (direction * weight).astype(np.float32),
           "aux": np.concatenate([weight, depth * weight, segments * weight], axis=2).astype(np.float32)}
    if kind.startswith("no_"):
        out[kind[3:]] = None
    return out
