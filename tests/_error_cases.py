"""Shapes and observation sets for the noise estimate (rl_error_unit_*), shared by tests/test_error.py and tests/test_gpu_error.py.
A case is {"initial": None or (S, Q, k, N) to upload first, "observations": [(xyz (h, w, 3) float32, n_paths), ...]}.  Test-only."""
import zlib

import numpy as np

# the smallest shapes at which the kernels can still go wrong: one pixel; an odd pixel count that is no multiple of four (the observe
# kernel's tail); one full tile; a one-pixel partial tile in each direction; partial tiles both ways over several tile rows; 64 x 36
SHAPES = [(1, 1), (5, 3), (16, 16), (17, 16), (16, 17), (33, 47), (64, 36)]
PARTIAL = [(17, 16), (16, 17), (33, 47)]
CASES = ("zeros", "single_hit", "proportional", "clamp", "negative", "huge", "nonfinite", "n_one", "n_unequal", "n_big", "k_two")


def _rng(name, w, h):
    return np.random.default_rng(zlib.crc32(("%s %d %d" % (name, w, h)).encode()))


def noisy(rng, w, h, n_paths, scale=1.0):
    """A plot buffer like a render's: per pixel a Poisson number of hits (mean 0.002 n_paths, capped) of exponential size."""
    hits = rng.poisson(min(0.002 * n_paths, 50.0), size=(h, w, 3))
    return (hits * rng.exponential(1.0, size=(h, w, 3)) * scale).astype(np.float32)


def case(name, w, h):
    rng = _rng(name, w, h)
    if name == "zeros":
        return {"initial": None, "observations": [(np.zeros((h, w, 3), np.float32), 5)] * 3}
    if name == "single_hit":
        obs = [np.zeros((h, w, 3), np.float32) for _ in range(3)]
        obs[1][h // 2, w // 2] = (7.0, 2.5, 1.0)
        return {"initial": None, "observations": [(o, 9) for o in obs]}
    if name == "proportional":      # y_j = c n_j with small integers: S = c N, Q = c^2 N and S^2 / N are exact, d = 0, se = +0
        c = rng.integers(0, 6, size=(h, w)).astype(np.float32)
        out = []
        for n in (1, 3, 8, 2):
            xyz = rng.random((h, w, 3)).astype(np.float32)
            xyz[:, :, 1] = c * np.float32(n)
            out.append((xyz, n))
        return {"initial": None, "observations": out}
    if name == "clamp":             # an uploaded state whose Q lies one step below (even pixels) or above (odd) the rounded S^2 / N
        n, k = 7, 3
        s = (rng.random((h, w)) * 100.0 + 1.0).astype(np.float64)
        exact = (s * s) / np.float64(n)
        below = (np.arange(h * w).reshape(h, w) % 2) == 0
        q = np.where(below, np.nextafter(exact, -np.inf), np.nextafter(exact, np.inf))
        assert ((q - exact)[below] < 0).all()
        return {"initial": (s, q, k, n), "observations": []}
    if name == "negative":
        return {"initial": None, "observations": [(rng.normal(0.0, 3.0, size=(h, w, 3)).astype(np.float32), n) for n in (16, 16, 32)]}
    if name == "huge":              # 3e38: the square is finite in f64, the f32 se overflows to inf
        obs = [noisy(rng, w, h, 4096) for _ in range(3)]
        obs[0][0, 0, 1] = 3e38
        obs[2][h - 1, w - 1, 1] = 3e38
        obs[1][h - 1, w - 1, 1] = -3e38
        return {"initial": None, "observations": [(o, 4096) for o in obs]}
    if name == "nonfinite":         # an infinity in the first pixel, a NaN in the last: different tiles wherever there are two
        obs = [noisy(rng, w, h, 4096) for _ in range(3)]
        obs[1][0, 0, 1] = np.inf
        obs[2][h - 1, w - 1, 1] = np.nan
        if h * w > 2:
            obs[0][h // 2, w // 2, 1] = -np.inf
        return {"initial": None, "observations": [(o, 4096) for o in obs]}
    if name == "n_one":
        return {"initial": None, "observations": [(noisy(rng, w, h, 500), 1) for _ in range(4)]}
    if name == "n_unequal":
        return {"initial": None, "observations": [(noisy(rng, w, h, n), n) for n in (1, 7, 4096, 3, 100000)]}
    if name == "n_big":             # 2^33 + 1 is exact as a double and does not fit 32 bits
        return {"initial": None, "observations": [(noisy(rng, w, h, n, scale=1e3), n) for n in ((1 << 33) + 1, 12345, (1 << 33) + 1)]}
    if name == "k_two":
        return {"initial": None, "observations": [(noisy(rng, w, h, n), n) for n in (4096, 8192)]}
    raise KeyError(name)


def compound_poisson(rng, n_pixels, n_paths, rate, shape=2.0):
    """(batch sums (n_pixels,) float64, the true variance of one path's contribution per pixel): per pixel a Poisson(rate n_paths)
    number of hits, each a Gamma(shape, 1) value.  One path contributes a hit with probability ~rate: its variance is
    rate E[g^2] (compound Poisson: lambda E[g^2] for the sum), E[g^2] = shape (shape + 1)."""
    hits = rng.poisson(rate * n_paths)
    sums = np.array([rng.gamma(shape, 1.0, size=k).sum() for k in hits.reshape(-1)]).reshape(hits.shape)
    return sums, rate * shape * (shape + 1.0)
