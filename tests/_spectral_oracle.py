"""The spectral film's contract (include/robigo_luculenta.h, rl_spectral_unit_*) restated in float32 numpy, one array operation per
stated operation: the splat's terms and film, the projection, and the bounds the tests hold a film to.  The pixel weights are
_feature_oracle.splat_terms', which restates rl_splat_weights.  Test-only; nothing is built at import."""
import numpy as np

import _feature_oracle as FO

MAX_NODES = 401
U = 2.0 ** -24                       # the unit roundoff of f32
f32 = np.float32


def spacing(n_nodes):
    return f32(400.0) / f32(n_nodes - 1)


def node_wavelengths(n_nodes):
    return f32(380.0) + np.arange(n_nodes).astype(np.float32) * spacing(n_nodes)


def kept(photons):
    """The photons the splat does not skip: probability != 0 and x, y, wavelength all finite."""
    with np.errstate(invalid="ignore"):
        return (photons["probability"] != 0) & np.isfinite(photons["x"]) & np.isfinite(photons["y"]) & np.isfinite(photons["wavelength"])


def splat_terms(w, h, n_nodes, photons):
    """(idx int64 (m, 8), terms float32 (m, 8)) of the m photons that are not skipped, in photon order: the four `lo` products and
    the four `hi` products of each, in rl_splat_weights' pixel order, and where in the flat node-major film each lands -- -1 for a
    node outside 0 .. n_nodes - 1, which is dropped."""
    ph = photons[kept(photons)]
    p, wl = ph["probability"].astype(np.float32), ph["wavelength"].astype(np.float32)
    with np.errstate(all="ignore"):
        f = (wl - f32(380.0)) / spacing(n_nodes)
        fl = np.floor(f)
        r = f - fl
        lo = p * (f32(1.0) - r)
        hi = p * r
        lo_in = (fl >= f32(0.0)) & (fl <= f32(n_nodes - 1))
        hi_in = (fl >= f32(-1.0)) & (fl <= f32(n_nodes - 1) - f32(1.0))
        node = np.where(lo_in | hi_in, fl, f32(0.0)).astype(np.int64)        # (only converted where it is in -1 .. n_nodes - 1)
        pixel, products = FO.splat_terms(w, h, ph["x"], ph["y"], np.stack([lo, hi, np.zeros_like(lo)], axis=1))
    idx = np.concatenate([np.where(lo_in[:, None], node[:, None] * (w * h) + pixel, -1),
                          np.where(hi_in[:, None], (node[:, None] + 1) * (w * h) + pixel, -1)], axis=1)
    return idx, np.concatenate([products[:, :, 0], products[:, :, 1]], axis=1)


def splat(w, h, n_nodes, photons, onto=None):
    """(film float32 (n_nodes, h, w) summed in photon order, k: the non-zero terms of each element, S float64: the sum of their
    magnitudes, exact float64: their sum).  onto: what the film held before, which counts as one more term of each element."""
    idx, terms = splat_terms(w, h, n_nodes, photons)
    on = idx.reshape(-1) >= 0
    idx, terms = idx.reshape(-1)[on], terms.reshape(-1)[on]
    size = n_nodes * w * h
    film = np.zeros(size, np.float32) if onto is None else np.array(onto, np.float32).reshape(size)
    first = film.astype(np.float64)
    with np.errstate(all="ignore"):
        t = terms.astype(np.float64)
        k = np.bincount(idx, weights=(t != 0), minlength=size).astype(np.int64) + (first != 0)
        s = np.bincount(idx, weights=np.abs(t), minlength=size) + np.abs(first)
        exact = np.bincount(idx, weights=t, minlength=size) + first
        np.add.at(film, idx, terms)
    shape = (n_nodes, h, w)
    return film.reshape(shape), k.reshape(shape), s.reshape(shape), exact.reshape(shape)


def violations(got, want, k, s, exact):
    """_feature_oracle.splat_violations for a film: the elements where got is not want's bits (at most two non-zero terms: every
    order of the adds gives the same bits) or not within splat_bound(k, S) of the f64 sum; and the worst excess.  An element whose
    terms are not all finite is held to want's bits too, a NaN for a NaN: an infinity, or a NaN, comes out of every order."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    finite = np.isfinite(s)
    bad, excess = FO.splat_violations(np.where(finite, got, f32(0)), np.where(finite, want, f32(0)), np.where(finite, k, 0),
                                      np.where(finite, s, 0.0), np.where(finite, exact, 0.0))
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    odd = np.argwhere(~finite & ~same)
    return (np.concatenate([bad, odd]) if len(odd) else bad), excess


def project(film, matrix):
    """(n_pixels, 3) float32: acc = 0; acc = acc + matrix[b, k] * film[b, p] for b in order."""
    film = np.asarray(film, np.float32)
    film = film.reshape(film.shape[0], -1)
    matrix = np.asarray(matrix, np.float32).reshape(film.shape[0], 3)
    acc = np.zeros((film.shape[1], 3), np.float32)
    with np.errstate(all="ignore"):
        for b in range(film.shape[0]):
            acc = acc + matrix[b][None, :] * film[b][:, None]
    return acc


def identity_bound(w, h, photons, table):
    """What holds project(observer) of an 81-node film to the XYZ film of the same photons, per pixel component: (bound float64
    (w * h, 3), S, k, nodes).  Both compute E = sum over photons and pixel slots of p w (a (1 - r) + b r), a and b the table's rows
    around the wavelength, from the same f32 r = f - fl and the same f32 weight w; S is the sum of the terms' magnitudes, k the
    number of (photon, slot) terms on the pixel and `nodes` the number of nodes they reach.  Roundings, each at most 2^-24 of a
    quantity that S bounds:
      the XYZ film: (1 - r), a (1 - r), b r, their sum, the product with p, the product with w -- 5 on a term; k - 1 adds, any order;
      the spectral film: (1 - r), the product with p, the product with w -- 3 on a term; at most k - 1 adds on each node, any order;
      the projection: the product with the matrix entry -- 1; nodes - 1 adds that are not of a zero.
    Together (5 + (k - 1)) + (3 + (k - 1)) + (1 + (nodes - 1)) = 2 k + nodes + 6 roundings.  The factor 1.001 covers the products
    of roundings (2 k + nodes stays below 10^4 here, so they are below 10^-3 of the first-order sum) and the f64 sums' own error."""
    table = np.asarray(table, np.float64).reshape(81, 3)
    idx, terms = splat_terms(w, h, 81, photons)
    n_pixels = w * h
    on = (idx >= 0) & (terms != 0)
    node, pixel = idx // n_pixels, idx % n_pixels
    s = np.zeros((n_pixels, 3))
    for c in range(3):
        s[:, c] = np.bincount(pixel[on], weights=(np.abs(terms.astype(np.float64)) * table[np.clip(node, 0, 80), c])[on], minlength=n_pixels)
    slot = (on[:, :4] | on[:, 4:])                                          # a (photon, slot) term: its lo or its hi part, or both
    k = np.bincount(np.where(on[:, :4], pixel[:, :4], pixel[:, 4:])[slot], minlength=n_pixels)
    reached = np.zeros((81, n_pixels), bool)
    reached[node[on], pixel[on]] = True
    nodes = reached.sum(axis=0)
    bound = (2 * k + nodes + 6)[:, None] * U * s * 1.001
    return bound, s, k, nodes
