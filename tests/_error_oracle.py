"""rl_error_unit_* on the CPU: the arithmetic of include/robigo_luculenta.h's noise-estimate block in numpy, one array operation per
stated operation.  float64 and float32 +, -, *, / of numpy are the IEEE ones, the float64 -> float32 conversion rounds to nearest,
rl_sqrtf is np.sqrt on float32, which is correctly rounded.  S and Q are (h, w) float64 arrays; a plot buffer is (h, w, 3) float32.
Test-only."""
import numpy as np

TILE = 16
f64 = np.float64


def new_state(w, h):
    """(S, Q, k, N) of a fresh or cleared unit."""
    return np.zeros((h, w), f64), np.zeros((h, w), f64), 0, 0


def observe(state, xyz, n_paths):
    """One rl_error_unit_observe: yd = (double)y; S = S + yd; Q = Q + (yd * yd) / (double)n_paths; k += 1; N += n_paths."""
    s, q, k, n = state
    h, w = s.shape
    with np.errstate(all="ignore"):
        yd = np.asarray(xyz, np.float32).reshape(h, w, 3)[:, :, 1].astype(f64)
        s = s + yd
        q = q + (yd * yd) / f64(n_paths)
    assert n_paths > 0 and n + n_paths < 1 << 64
    return s, q, k + 1, n + n_paths


def tile_tree(values):
    """The tree over a (h, w) float64 array per 16 x 16 tile: the tile's 256 values in tile raster order, +0.0 outside the image;
    for stride = 128 .. 1: v[i] = v[i] + v[i + stride] for i < stride.  Returns (tiles_y, tiles_x) float64."""
    h, w = values.shape
    ty, tx = -(-h // TILE), -(-w // TILE)
    padded = np.zeros((ty * TILE, tx * TILE), f64)
    padded[:h, :w] = values
    v = padded.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, TILE * TILE).copy()
    stride = 128
    with np.errstate(all="ignore"):
        while stride >= 1:
            v[:, :, :stride] = v[:, :, :stride] + v[:, :, stride:2 * stride]
            stride //= 2
    return v[:, :, 0].copy()


def pixels(state):
    """(se (h, w) float32, ay (h, w) float64) of the estimate."""
    s, q, k, n = state
    assert k >= 2
    with np.errstate(all="ignore"):
        d = q - (s * s) / f64(np.uint64(n))
        d = np.where(d < 0, f64(0), d)
        v = d * (f64(np.uint64(n)) / f64(np.uint64(k - 1)))
        se = np.sqrt(v.astype(np.float32))
        ay = np.abs(s)
    return se, ay


def host_stats(tiles, k, n):
    """RlErrorStats as a dict from (tiles_y, tiles_x, 2) pairs: every sum sequential in f64 in tile raster order."""
    ty, tx = tiles.shape[:2]
    pairs = tiles.reshape(-1, 2)
    sum_se, sum_y = f64(0), f64(0)
    with np.errstate(all="ignore"):
        for t_se, t_y in pairs:
            sum_se = sum_se + t_se
            sum_y = sum_y + t_y
        m = sum_y / f64(len(pairs))
        worst, at = None, 0
        for i, (t_se, t_y) in enumerate(pairs):
            rel = t_se / (t_y if t_y > m else m)
            if i == 0 or rel > worst:
                worst, at = rel, i
        relative = sum_se / sum_y
    return {"observations": k, "paths": n, "tiles_x": tx, "tiles_y": ty, "worst_tile_x": at % tx, "worst_tile_y": at // tx,
            "sum_y": float(sum_y), "sum_se": float(sum_se), "relative_error": float(relative), "worst_tile_error": float(worst)}


def tile_rel(tiles):
    """The per-tile rel of host_stats, (tiles_y, tiles_x) float64."""
    pairs = tiles.reshape(-1, 2)
    sum_y = f64(0)
    with np.errstate(all="ignore"):
        for t_y in pairs[:, 1]:
            sum_y = sum_y + t_y
        m = sum_y / f64(len(pairs))
        return (pairs[:, 0] / np.where(pairs[:, 1] > m, pairs[:, 1], m)).reshape(tiles.shape[:2])


def estimate(state):
    """rl_error_unit_estimate: (stats dict, se (h, w) float32, tiles (tiles_y, tiles_x, 2) float64)."""
    se, ay = pixels(state)
    tiles = np.stack([tile_tree(se.astype(f64)), tile_tree(ay)], axis=2)
    return host_stats(tiles, state[2], state[3]), se, tiles
