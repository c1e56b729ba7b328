"""Inputs of the glare unit's tests (tests/test_glare.py, tests/test_gpu_glare.py): shapes, films, asymmetric tables and matrices,
all deterministic.  Test-only."""
import numpy as np

# (width, height, n_nodes, taps): the smallest shapes that can break a kernel of 64 x 16 tiles with four pixels to a lane --
# one pixel; a film smaller than the table; one pixel wide; one pixel high; no multiple of any tile, several tiles each way;
# exactly one tile; many nodes, three tiles across and down, a width that is no multiple of the lane's strip; the cap, one tile's
# halo far beyond the film.
SHAPES = [(1, 1, 2, 1), (5, 3, 2, 9), (1, 40, 3, 3), (40, 1, 3, 3), (67, 19, 5, 9), (64, 16, 2, 3), (130, 35, 81, 3), (33, 33, 2, 65)]
shape_id = lambda s: "%dx%d-%dnodes-%dtaps" % s


def _rng(*key):
    return np.random.default_rng([7919] + [int(k) for k in key])


def film(w, h, n_nodes, salt=0):
    """(n_nodes, h, w) float32: log-uniform magnitudes over six decades, a third of the values exactly +0, and in every plane a
    -0.0, two denormals and one huge value (2^100: its products with the tables stay finite, its neighbours' sums are swamped)."""
    g = _rng(w, h, n_nodes, salt)
    out = np.exp(g.uniform(np.log(1e-3), np.log(1e3), (n_nodes, h, w))).astype(np.float32)
    out[g.random(out.shape) < 0.33] = 0.0
    special = np.array([-0.0, 1e-40, -3e-42, 2.0 ** 100], np.float32)
    for b in range(n_nodes):
        where = g.permutation(h * w)[:len(special)]
        out[b].reshape(-1)[where] = special[::-1][:len(where)]        # (a one-pixel film keeps the huge value)
    return out


def random_film(w, h, n_nodes, salt=0):
    """Finite, sign-mixed, no special values: what the f64 comparison runs on."""
    g = _rng(w, h, n_nodes, salt, 1)
    return (g.uniform(-1.0, 1.0, (n_nodes, h, w)) * np.exp(g.uniform(-3.0, 3.0, (n_nodes, h, w)))).astype(np.float32)


def tables(n_nodes, taps, salt=0):
    """(n_nodes, taps, taps) float32: asymmetric (no entry equals its mirror image in either axis), sign-mixed, different per node."""
    g = _rng(n_nodes, taps, salt, 2)
    t = g.uniform(-1.0, 1.0, (n_nodes, taps, taps))
    ramp = 1.0 + 0.5 * np.arange(taps)[None, None, :] / taps + 0.25 * np.arange(taps)[None, :, None] / taps
    return (t * ramp / taps).astype(np.float32)


def asymmetric_psf(taps):
    """A non-negative base function with no symmetry: a ramp in x, another in y, a bump off the centre."""
    j, i = np.mgrid[0:taps, 0:taps].astype(np.float64)
    p = 1.0 + 0.5 * i + 0.125 * j * j
    p[taps // 3, (2 * taps) // 3] += 10.0
    return p.astype(np.float32)


def matrix(n_nodes, salt=0):
    """(n_nodes, 3) float32 with entries of both signs."""
    return _rng(n_nodes, salt, 3).uniform(-2.0, 2.0, (n_nodes, 3)).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
