"""Inputs of the spectral film's tests (tests/test_spectral.py, tests/test_gpu_spectral.py): shapes, node counts, photon sets, film
classes and matrices, all deterministic.  Test-only."""
import functools

import numpy as np

import _spectral_oracle as SO

PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])
RL_MAX_PIXELS = 2 ** 31 - 1
# (w, h): one pixel; one pixel wide; one pixel high; a small square; the demo render's size (several workgroups of pixels)
SHAPES = [(1, 1), (1, 7), (5, 1), (3, 3), (64, 36)]
# the smallest film; an odd count with one inner node; the CIE table's own; the largest
NODES = [2, 3, 81, 401]
FILMS = ["loguniform", "with_zeros", "nonfinite"]
MATRICES = ["cie", "signed", "zero", "nonfinite"]
TINY = np.float32(2.0 ** -40)   # a probability far below the others': its products with weights of 2^-24 and more stay normal numbers


def combinations():
    """Every (w, h, n_nodes) whose cube rl_spectral_unit_create accepts."""
    return [(w, h, n) for (w, h) in SHAPES for n in NODES if w * h * n <= RL_MAX_PIXELS]


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))   # (hash() of a string changes from process to process)


def _next(x, towards):
    return np.nextafter(np.float32(x), np.float32(towards))


def edge_wavelengths():
    """Exactly 375, 380, 780 and 785 nm, the f32 neighbours of each on both sides, and every node of the 81."""
    ends = []
    for v in (375.0, 380.0, 780.0, 785.0):
        ends += [_next(v, 0.0), np.float32(v), _next(v, 1000.0)]
    return np.concatenate([np.array(ends, np.float32), SO.node_wavelengths(81)])


def synthetic_photons(w, h, n=3000):
    """A few thousand photons no renderer makes: wavelengths from 300 to 860 nm with edge_wavelengths() among them and far ones;
    x and y inside, exactly on and up to two pixels beyond the screen's borders, a few far beyond (a border pixel then takes two
    large terms of opposite sign), and NaN / +-inf; wavelength NaN / +-inf; probability 0, negative, +inf and TINY.  (x and y stay
    below 100 in size: the pixel coordinate stays far inside int32.)"""
    g = np.random.default_rng([_seed("synthetic"), w, h])
    aspect = np.float32(w) / np.float32(h)
    ph = np.zeros(n, PHOTON_DTYPE)
    ph["x"] = g.uniform(-1.0, 1.0, n)
    ph["y"] = g.uniform(-1.0, 1.0, n) / aspect
    ph["probability"] = g.uniform(0.0, 1.0, n)
    ph["wavelength"] = g.uniform(300.0, 860.0, n)
    order = g.permutation(n)
    taken = [0]

    def take(count):
        """The next `count` rows nobody has set yet."""
        taken[0] += count
        return order[taken[0] - count:taken[0]]

    edges = edge_wavelengths()
    ph["wavelength"][take(len(edges))] = edges
    far = take(12)
    ph["wavelength"][far] = np.array([0.0, -380.0, 1e4, 3e9, -3e9, 1e20, -1e20, 3e38, -3e38, 379.99, 5000.0, 2147483648.0 * 5 + 380], np.float32)
    border = take(120)
    ph["x"][border[0::4]], ph["x"][border[1::4]] = -1.0, 1.0
    ph["y"][border[2::4]], ph["y"][border[3::4]] = np.float32(-1.0) / aspect, np.float32(1.0) / aspect
    beyond = take(200)
    side = np.where(g.random(len(beyond)) < 0.5, -1.0, 1.0)
    ph["x"][beyond[:100]] = side[:100] * (1.0 + g.random(100) * 4.0 / max(w - 1, 1))
    ph["y"][beyond[100:]] = side[100:] * (1.0 + g.random(100) * 4.0 / max(h - 1, 1)) / aspect
    outside = take(8)
    ph["x"][outside[:4]] = np.array([-3.0, 7.5, -40.0, 90.0], np.float32)
    ph["y"][outside[4:]] = np.array([-3.0, 7.5, -40.0, 90.0], np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for field in ("x", "y", "wavelength"):
        rows = take(9)
        ph[field][rows] = bad[np.arange(9) % 3]
        ph["probability"][rows] = 1.0
    both = take(3)
    ph["x"][both], ph["y"][both], ph["wavelength"][both] = np.nan, -np.inf, np.inf
    ph["probability"][take(150)] = 0.0
    negative = take(300)
    ph["probability"][negative] *= -1.0
    # (at the corner, at 377 nm: every term falls on element (node 0, pixel 0), so that the smallest films keep finite elements)
    infinite = take(3)
    ph["x"][infinite], ph["y"][infinite], ph["wavelength"][infinite] = -1.0, np.float32(-1.0) / aspect, 377.0
    ph["probability"][infinite] = np.inf
    ph["probability"][take(60)] = TINY
    return ph


@functools.lru_cache(maxsize=None)
def demo_photons(w, h, n, seed=1, stream=0):
    """Paths 0 .. n - 1 of (seed, stream) of the demo scene on a w x h film by the CPU oracle: (n,) PHOTON_DTYPE, read-only."""
    import _oracle as O
    objs, cam = O.demo_scene_desc()
    photons, _ = O.Scene(objs, cam).render(w, h, seed, stream, 0, n, threads=4)
    photons = photons.view(PHOTON_DTYPE)
    photons.setflags(write=False)
    return photons


def film(kind, w, h, n_nodes):
    """(n_nodes, h, w) float32 to upload."""
    g = np.random.default_rng([_seed(kind), w, h, n_nodes])
    out = np.exp(g.uniform(np.log(1e-3), np.log(1e3), (n_nodes, h, w))).astype(np.float32)
    if kind == "loguniform":
        return out
    out[g.random(out.shape) < 0.3] = 0.0
    if kind == "with_zeros":
        return out
    flat = out.reshape(-1)
    where = g.permutation(len(flat))[:min(6, len(flat))]
    flat[where] = np.array([np.nan, np.inf, -np.inf, np.inf, -np.inf, np.nan], np.float32)[:len(where)]
    return out


def matrix(kind, n_nodes):
    """(n_nodes, 3) float32.  "cie" is the oracle's restatement of the table at the nodes' wavelengths."""
    g = np.random.default_rng([_seed(kind), n_nodes])
    if kind == "cie":
        import _image_cases as IC
        return IC.tristimulus(SO.node_wavelengths(n_nodes))
    if kind == "zero":
        return np.zeros((n_nodes, 3), np.float32)
    out = (g.uniform(-2.0, 2.0, (n_nodes, 3))).astype(np.float32)
    if kind == "nonfinite":
        flat = out.reshape(-1)
        flat[g.permutation(len(flat))[:4]] = np.array([np.nan, np.inf, -np.inf, 0.0], np.float32)
    return out
