"""The films, importance sets and path counts the adaptive sampler's tests share (tests/test_adaptive.py, test_adaptive_abi.py,
test_gpu_adaptive.py).  Everything is made from fixed seeds; nothing is built at import."""
import numpy as np

import _adaptive_oracle as AO

# 4 x 3 tiles with a bottom row 4 pixels high; last cells 0.5 wide; one whole tile; the smallest film; 120 x 68 tiles
FILMS = [(64, 36), (33, 17), (16, 16), (2, 2), (1920, 1080)]
SMALL_FILMS = [(64, 36), (33, 17)]
UNIFORM_SHARE = 0.25
N_MAX = (1 << 32) - 1
IMPORTANCE = ("null", "equal", "one_hot_partial", "random", "invalid_entries", "all_zero")


def importance(name, w, h):
    """The importance set `name` for a w x h film: None or tiles_y * tiles_x doubles."""
    tx, ty = AO.tiles_of(w, h)
    n = tx * ty
    if name == "null":
        return None
    if name == "equal":
        return np.full(n, 3.0)
    if name == "one_hot_partial":        # everything on the last tile, which is partial on every film but 16 x 16
        g = np.zeros(n)
        g[-1] = 7.5
        return g
    if name == "random":
        return np.random.default_rng(w * 10007 + h).random(n) * 10.0 ** np.random.default_rng(h).integers(-3, 3, n)
    if name == "invalid_entries":        # NaN, infinite and negative entries count as 0; what is left is valid
        g = np.random.default_rng(w + h).random(n) + 0.5
        for k, bad in enumerate((np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e300)):   # (1e300: valid, and it dwarfs the rest)
            g[(k * 5) % n] = bad
        if not (np.isfinite(g) & (g > 0)).any():
            g[n - 1] = 1.0
        return g
    if name == "all_zero":
        return np.zeros(n)
    raise KeyError(name)


def overflowing(w, h):
    """Finite entries whose sequential sum G overflows, or None for a film of one tile.  (Entries of 1e300 alone overflow only
    from 1.8e8 tiles on; on these films they are part of "invalid_entries" as valid, very large values, and here two of 1e308 do it.)"""
    tx, ty = AO.tiles_of(w, h)
    n = tx * ty
    if n < 2:
        return None
    g = np.full(n, 1e300)
    g[0] = g[n - 1] = 1e308
    return g


def accepts(w, h, g, share, n):
    return AO.plan(w, h, g, share, n)[0] == AO.PLAN_OK


def smallest_n(w, h, g, share):
    """An n the plan accepts whose predecessor it refuses (every tile gets a sample at n, one gets none at n - 1), found by
    bisection between a refused and an accepted count."""
    lo, hi = 0, 1            # lo refused (0 paths is no plan), hi to be accepted
    while not accepts(w, h, g, share, hi):
        lo, hi = hi, hi * 2
        assert hi <= N_MAX
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepts(w, h, g, share, mid):
            hi = mid
        else:
            lo = mid
    return hi
