"""Inputs of the variance-guided denoiser's tests (tests/test_denoise_variance.py, tests/test_gpu_denoise_variance.py).  Shapes,
images and guides are tests/_denoise_cases.py's; the error states here are (S, Q, k, N) for rl_error_unit_upload, built from the
image's own luminance so that the units match.  All deterministic.  Test-only."""
import numpy as np

from _denoise_cases import SHAPES, _seed, guides, image  # noqa: F401  (shared with the plain denoiser's tests)

IMAGES = ["loguniform", "nonfinite"]
GUIDES = ["random", "checker", "dead", "no_aux"]
ERRORS = ["matched", "zero", "checker", "huge", "nonfinite", "k2_unequal"]
PARAMS = {
    "defaults": {},
    "colour_alone": dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
    "all_off": dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0),
    "one_pass": dict(iterations=1),
    "six_passes": dict(iterations=6),
    "colour_smallest": dict(sigma_colour=1e-3),
    "colour_largest": dict(sigma_colour=1e3),
}
f64 = np.float64


def _matched(g, y, k, n):
    """S = y and Q = S^2 / N + u, u log-uniform so that V = u N / (k - 1) is about (0.03 .. 3 |y|)^2."""
    s = y.astype(f64)
    with np.errstate(all="ignore"):
        f = np.exp(g.uniform(np.log(0.03), np.log(3.0), y.shape))
        u = (f * np.abs(s)) ** 2 * (f64(k - 1) / f64(n))
        q = (s * s) / f64(n) + u
    return s, q


def _zero(y, n):
    s = y.astype(f64)
    with np.errstate(all="ignore"):
        return s, (s * s) / f64(n)


def error_state(kind, img):
    """(S, Q, k, N) of an error class for an (h, w, 3) image."""
    h, w = img.shape[:2]
    g = np.random.default_rng([_seed(kind), w, h, 77])
    y = img[..., 1]
    k, n = 8, 8 * 4096
    if kind == "k2_unequal":
        k, n = 2, (1 << 33) + 1
    s, q = _matched(g, y, k, n)
    if kind == "zero":
        s, q = _zero(y, n)
    elif kind == "checker":
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        q = np.where((xs + ys) % 2 == 0, q, _zero(y, n)[1])
    elif kind == "huge":            # v = 1e40 is a double and no float: V_0 = +inf
        q = (s * s) / f64(n) + f64(1e40) * (f64(k - 1) / f64(n))
    elif kind == "nonfinite":
        flat_s, flat_q = s.reshape(-1), q.reshape(-1)
        where = g.permutation(flat_s.size)[:min(3, flat_s.size)]
        for p, (vs, vq) in zip(where, ((np.nan, None), (None, np.inf), (np.inf, np.nan))):
            if vs is not None:
                flat_s[p] = vs
            if vq is not None:
                flat_q[p] = vq
    return np.ascontiguousarray(s), np.ascontiguousarray(q), k, n
