"""Shapes, bucket counts, observation schedules and edge states for the robust film (rl_robust_unit_*), shared by
tests/test_robust.py, tests/test_robust_abi.py and tests/test_gpu_robust.py.  Test-only."""
import zlib

import numpy as np

NEXT = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF

# the kernels' edges: one pixel (the observe kernel's tail alone); odd pixel counts (its pair path and the tail; the device's planes
# are then padded to an even stride); 16 x 9 and 64 x 36, the shapes of the real plot buffers; 144 = 2.25 waves of the resolve kernel
SHAPES = [(1, 1), (3, 1), (17, 5), (16, 9), (64, 36)]
# More pixels than one pass of either grid covers, so both grid-stride loops iterate: rl_robust_unit_observe launches at most
# 8 x CUs workgroups of RL_BLOCK = 256 lanes with two pixels each, 1,048,576 pixels on the 256 CUs of an MI355X; the resolve
# launches at most 8 x CUs x 4 one-wave workgroups, 524,288 pixels.  1031 x 1021 = 1,052,651 pixels, an odd count.
GRID_STRIDE_SHAPE = (1031, 1021)
assert GRID_STRIDE_SHAPE[0] * GRID_STRIDE_SHAPE[1] > 256 * 8 * 256 * 2 and GRID_STRIDE_SHAPE[0] * GRID_STRIDE_SHAPE[1] % 2 == 1
BUCKETS = [3, 4, 15, 32]
# (gain, max_trim)
PARAMS = [(0.0, NO_LIMIT), (1.0, NO_LIMIT), (float("inf"), NO_LIMIT), (1.0, 0), (1.0, 1), (float("inf"), 1), (2.5, NO_LIMIT)]
SCHEDULES = ("next", "scrambled", "unequal")


def _rng(*what):
    return np.random.default_rng(zlib.crc32(" ".join(str(x) for x in what).encode()))


def noisy(rng, w, h, n_paths):
    """A plot buffer like a render's: per pixel a Poisson number of hits (mean 0.002 n_paths, capped) of exponential size, the
    three components alike but not equal."""
    hits = rng.poisson(min(0.002 * n_paths, 50.0), size=(h, w, 1))
    return (hits * rng.exponential(1.0, size=(h, w, 3))).astype(np.float32)


def schedule(name, w, h, m):
    """[(xyz (h, w, 3) float32, n_paths, bucket)]: `next` 2 M + 1 observations in turn (RL_ROBUST_NEXT), so the round robin wraps
    twice; `scrambled` explicit buckets in a shuffled order, every bucket twice; `unequal` path counts from 1 to beyond 2^33."""
    rng = _rng(name, w, h, m)
    if name == "next":
        return [(noisy(rng, w, h, 4096), 4096, NEXT) for _ in range(2 * m + 1)]
    if name == "scrambled":
        order = rng.permutation(np.repeat(np.arange(m), 2))
        return [(noisy(rng, w, h, 2048), 2048, int(j)) for j in order]
    if name == "unequal":
        counts = [1, 7, 4096, 3, 100000, (1 << 33) + 1]
        out = []
        for i in range(m + 2):
            n = counts[i % len(counts)]
            out.append((noisy(rng, w, h, n), n, NEXT if i % 2 else i % m))
        # (the explicit buckets are the even i, so with NEXT's turns every bucket of every M here is filled; checked below)
        out += [(noisy(rng, w, h, 16), 16, j) for j in range(m)]
        return out
    raise KeyError(name)


def edge_state(w, h, m, seed=0):
    """An uploaded state (sums (M, 3, h, w), n, k) whose pixels run through the resolve's edges, pixel p taking edge p % 12 on top of
    a noisy film: 0 plain noise; 1 all buckets equal; 2 one bucket x 1000; 3 exact ties in Y with distinct X (all Y equal but one);
    4 a NaN key; 5 a +inf key; 6 a negative key; 7 all zero; 8 a -inf key; 9 two outliers; 10 every Y zero but X not; 11 ties at
    zero and a -0.0.  The n[j] are unequal and all > 0."""
    rng = _rng("edge", w, h, m, seed)
    p = h * w
    n = [int(x) for x in rng.integers(1, 5000, size=m)]
    n[0] = (1 << 33) + 1
    base = rng.poisson(20.0, size=(m, 1, p)) * rng.exponential(1.0, size=(m, 3, p)) + 1.0
    sums = base * np.asarray(n, np.float64)[:, None, None]
    for q in range(p):
        edge, j = q % 12, int(rng.integers(0, m))
        if edge == 1:
            sums[:, :, q] = np.asarray(n, np.float64)[:, None] * np.asarray([0.5, 0.25, 2.0])[None, :]
            if q % 24 == 1:                       # power-of-two path counts: the means are exactly equal
                sums[:, :, q] = 3.0
        elif edge == 2:
            sums[j, :, q] *= 1000.0
        elif edge == 3:
            sums[:, 1, q] = np.asarray(n, np.float64) * 0.75
            sums[j, 1, q] *= 3.0
        elif edge == 4:
            sums[j, 1, q] = np.nan
        elif edge == 5:
            sums[j, 1, q] = np.inf
        elif edge == 6:
            sums[j, 1, q] = -sums[j, 1, q]
        elif edge == 7:
            sums[:, :, q] = 0.0
        elif edge == 8:
            sums[j, 1, q] = -np.inf
        elif edge == 9:
            sums[j, :, q] *= 400.0
            sums[(j + 1) % m, :, q] *= 900.0
        elif edge == 10:
            sums[:, 1, q] = 0.0
        elif edge == 11:
            sums[:, 1, q] = 0.0
            sums[j, 1, q] = -0.0
            sums[(j + 1) % m, 1, q] = 5.0 * n[(j + 1) % m]
    return sums.reshape(m, 3, h, w), n, 2 * m + 3


for _m in BUCKETS:
    assert {j if j != NEXT else None for _, _, j in schedule("unequal", 1, 1, _m)} >= set(range(_m))
