"""The numpy restatement of the glare unit's contract (include/robigo_luculenta.h, "spectral glare").  apply() is a loop over
(b, j, i) of whole-image f32 multiplies and adds under the in-film mask, in the contract's order, so it holds the device bit for
bit; the two host helpers are f64 with explicit sequential sums (numpy.sum is pairwise and is not the contract), so they hold the
library's bit for bit after the final rounding to f32.  apply_f64() and bound() are what tests/test_glare.py holds apply() to."""
import numpy as np

U = 2.0 ** -24


def apply(film, tables, matrix):
    """film (n, h, w) f32, tables (n, K, K) f32, matrix (n, 3) f32 -> (h, w, 3) f32: the contract, operation for operation."""
    film, tables, matrix = (np.ascontiguousarray(a, np.float32) for a in (film, tables, matrix))
    n, h, w = film.shape
    K = tables.shape[1]
    R = (K - 1) // 2
    acc = np.zeros((h, w, 3), np.float32)
    with np.errstate(all="ignore"):
        for b in range(n):
            g = np.zeros((h, w), np.float32)
            for j in range(K):
                r = np.zeros((h, w), np.float32)
                dy = j - R
                y0, y1 = max(0, -dy), min(h, h - dy)          # the pixels whose tap row y + dy is inside the film
                for i in range(K):
                    dx = i - R
                    x0, x1 = max(0, -dx), min(w, w - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    t = tables[b, j, i]                       # an np.float32: the product and the sum below stay f32
                    r[y0:y1, x0:x1] = r[y0:y1, x0:x1] + t * film[b, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
                g = g + r
            for c in range(3):
                acc[:, :, c] = acc[:, :, c] + matrix[b, c] * g
    return acc


def _correlate_f64(plane, table):
    """sum over taps inside the film of table[j, i] * plane[y + j - R, x + i - R], in f64 (any order: the reference's error is 2^-53)."""
    h, w = plane.shape
    K = table.shape[0]
    R = (K - 1) // 2
    out = np.zeros((h, w), np.float64)
    for j in range(K):
        dy = j - R
        y0, y1 = max(0, -dy), min(h, h - dy)
        for i in range(K):
            dx = i - R
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] += table[j, i] * plane[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def apply_f64(film, tables, matrix):
    """(value, A): the same sums in f64, and A = sum |matrix| * |table| * |film| per output, the scale of its rounding bound."""
    film, tables, matrix = (np.asarray(a, np.float64) for a in (film, tables, matrix))
    n, h, w = film.shape
    value, scale = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for b in range(n):
        g, ga = _correlate_f64(film[b], tables[b]), _correlate_f64(np.abs(film[b]), np.abs(tables[b]))
        value += g[:, :, None] * matrix[b][None, None, :]
        scale += ga[:, :, None] * np.abs(matrix[b])[None, None, :]
    return value, scale


def bound(scale, taps, n_nodes):
    """The rounding bound of the two-level sum: a term passes through its product, at most K - 1 adds of its row sum, at most K adds
    of g, the product with the matrix and at most n_nodes adds of acc -- 2 K + n_nodes + 1 roundings of 2^-24 each, (2 K + n_nodes + 3)
    with the second-order terms rounded up generously, and 1 % on top.  Derived, not measured."""
    return (2 * taps + n_nodes + 3) * U * 1.01 * scale


def psf_veil(taps, r0):
    """rl_glare_psf_veil in f64, elementwise (each element's operations are the library's, in its order), rounded to f32."""
    R = (taps - 1) // 2
    d = np.arange(taps, dtype=np.int64) - R
    d2 = (d[None, :] * d[None, :] + d[:, None] * d[:, None]).astype(np.float64)      # (i - R)^2 + (j - R)^2, exact
    q = 1.0 + d2 / (np.float64(r0) * np.float64(r0))
    return (1.0 / (q * np.sqrt(q))).astype(np.float32)


def _sequential_sum(values):
    """One f64 accumulator over `values` in order (numpy.add.accumulate adds one element at a time: no pairwise tree)."""
    return np.add.accumulate(np.asarray(values, np.float64).reshape(-1))[-1]


def kernels_scaled_f64(psf, lambda0, n_nodes, strength, taps):
    """rl_glare_kernels_scaled before the rounding to f32: (n_nodes, taps, taps) f64, or None where the library refuses (S not > 0)."""
    psf = np.asarray(psf, np.float32).astype(np.float64)
    T = psf.shape[0]
    R_in, R = float((T - 1) // 2), (taps - 1) // 2
    padded = np.zeros((T + 2, T + 2))
    padded[1:-1, 1:-1] = psf                                   # p = 0 outside the base table

    def at(ix, iy):
        inside = (ix >= 0) & (ix < T) & (iy >= 0) & (iy < T)
        cx, cy = np.where(inside, ix, -1).astype(np.int64) + 1, np.where(inside, iy, -1).astype(np.int64) + 1
        return np.where(inside, padded[cy, cx], 0.0)

    out = np.zeros((n_nodes, taps, taps))
    d = (np.arange(taps, dtype=np.int64) - R).astype(np.float64)
    lambda0, strength = np.float64(lambda0), np.float64(strength)
    for b in range(n_nodes):
        lam = 380.0 + np.float64(b) * (400.0 / np.float64(n_nodes - 1))
        s = lam / lambda0
        p = -d / s + R_in                                      # u over i and v over j: the same values
        ip = np.floor(p)
        fp = p - ip
        iu, fu = np.broadcast_to(ip[None, :], (taps, taps)), np.broadcast_to(fp[None, :], (taps, taps))
        iv, fv = np.broadcast_to(ip[:, None], (taps, taps)), np.broadcast_to(fp[:, None], (taps, taps))
        p00, p10, p01, p11 = at(iu, iv), at(iu + 1.0, iv), at(iu, iv + 1.0), at(iu + 1.0, iv + 1.0)
        w = ((1.0 - fu) * p00 + fu * p10) * (1.0 - fv) + ((1.0 - fu) * p01 + fu * p11) * fv
        S = _sequential_sum(w)
        if not S > 0:
            return None
        t = strength * (w / S)
        t[R, R] = t[R, R] + (1.0 - strength)
        out[b] = t
    return out


def kernels_scaled(psf, lambda0, n_nodes, strength, taps):
    t = kernels_scaled_f64(psf, lambda0, n_nodes, strength, taps)
    return None if t is None else t.astype(np.float32)
