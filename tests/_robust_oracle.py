"""The robust film (rl_robust_unit_*) on the CPU, in the order include/robigo_luculenta.h states: the device's results are held to
these bit for bit.  A state is (sums (M, 3, h, w) float64, n: list of M ints, k).  resolve is vector code over the pixels whose every
operation is one IEEE f64 operation per pixel and whose sums run bucket by bucket in the stated order (no np.sum, whose pairwise
order differs); resolve_pixel is the same contract as a plain loop over one pixel, and tests/test_robust.py holds the two to each
other.  numpy only, but for gain_figures at the end, which renders with the CPU oracle.  Test-only."""
import math

import numpy as np

NEXT = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF
MAX_BUCKETS = 32


def new_state(w, h, m):
    return np.zeros((m, 3, h, w), np.float64), [0] * m, 0


def observe(state, xyz, n_paths, bucket=NEXT):
    """One plot buffer (h, w, 3) float32 added to a bucket: S[j][c] = S[j][c] + (double)p[c]; n[j] += n_paths; k += 1."""
    sums, n, k = state
    m = len(n)
    j = k % m if bucket == NEXT else bucket
    assert 0 <= j < m and n_paths > 0
    sums, n = sums.copy(), list(n)
    with np.errstate(all="ignore"):
        sums[j] = sums[j] + np.asarray(xyz, np.float32).astype(np.float64).transpose(2, 0, 1)
    n[j] += n_paths
    return sums, n, k + 1


def _cmax(m, max_trim):
    return min(max_trim, (m - 1) // 2)


def resolve(state, gain=1.0, max_trim=NO_LIMIT):
    """(film (h, w, 3) float32, trim (h, w) uint8, stats dict)."""
    sums, n, k = state
    m, _, h, w = sums.shape
    assert all(x > 0 for x in n) and gain >= 0
    p = h * w
    at = np.arange(p)
    gain, md, total = np.float64(gain), np.float64(m), np.float64(sum(n))
    cmax = _cmax(m, max_trim)
    with np.errstate(all="ignore"):
        mean = np.empty((m, 3, p), np.float64)
        for j in range(m):
            mean[j] = sums[j].reshape(3, p) / np.float64(n[j])
        key = mean[:, 1, :]
        bad = (~np.isfinite(key) | (key < 0)).any(axis=0)
        perm = np.empty((m, p), np.int64)
        for j in range(m):
            rank = np.zeros(p, np.int64)
            for i in range(m):
                rank += (key[i] < key[j]) | ((key[i] == key[j]) & (i < j))
            perm[np.where(bad, j, rank), at] = j
        t, wsum = np.zeros(p), np.zeros(p)
        for r in range(m):
            kr = key[perm[r], at]
            t = t + kr
            wsum = wsum + np.float64(2 * r - m + 1) * kr
        untrimmable = bad | ~(t > 0)
        g = wsum / (md * t)
        v = ((gain * g) * md) * np.float64(0.5)
        inside = (v >= 0) & (v < np.float64(cmax))
        c = np.where(inside, np.floor(np.where(inside, v, 0.0)), np.where(v >= np.float64(cmax), cmax, 0)).astype(np.int64)
        c = np.where(untrimmable, 0, c)
        film = np.empty((p, 3), np.float32)
        for comp in range(3):
            a = np.zeros(p)
            for r in range(m):
                a = np.where((r >= c) & (r < m - c), a + mean[perm[r], comp, at], a)
            film[:, comp] = ((a / (m - 2 * c).astype(np.float64)) * total).astype(np.float32)
    stats = {"observations": k, "paths": sum(n), "buckets": m, "largest_trim": int(c.max()), "trimmed_pixels": int((c > 0).sum()),
             "trimmed_buckets": int(2 * c.sum()), "untrimmable_pixels": int(untrimmable.sum())}
    return film.reshape(h, w, 3), c.astype(np.uint8).reshape(h, w), stats


# ---- the plain film against the robust one, on the CPU (tools/robust_gain.py, tests/golden/robust_gain.json) -----------------------

GAIN = dict(w=64, h=36, buckets=15, gain=1.0, seed=1, stream=0, ref_stream=1, ref_factor=16, firefly_factor=4.0)
# (scene: 1 the glass-stress scene, 0 the demo scene; batches; paths per batch), the smallest first: tests/test_robust.py re-derives it
GAIN_CONFIGS = [(1, 15, 1024), (1, 60, 8192), (0, 60, 8192), (1, 240, 8192), (0, 240, 8192)]


def gain_figures(objs, cam, batches, n, cfg=GAIN, threads=16):
    """The film of `batches` batches of n paths of cfg["stream"], batch b into bucket b % M, as the plain f64 sum of the batch films
    and as resolve()'s, both per path against the mean of ref_factor times as many paths of cfg["ref_stream"]: for each the relative
    mean squared error of Y, sum (Y - Yref)^2 / sum Yref^2, and the pixels whose Y exceeds firefly_factor * Yref; and the histogram of
    the trim c.  The CPU oracle's photons and plot (the only import beyond numpy, made here)."""
    import _oracle as O
    w, h, m = cfg["w"], cfg["h"], cfg["buckets"]
    scene = O.Scene(np.ascontiguousarray(objs), cam)
    total = batches * n
    ref = O.plot(w, h, scene.render(w, h, cfg["seed"], cfg["ref_stream"], 0, cfg["ref_factor"] * total, threads=threads)[0])
    ref_y = ref.astype(np.float64)[:, 1] / (cfg["ref_factor"] * total)
    state, plain = new_state(w, h, m), np.zeros((h * w, 3), np.float64)
    for b in range(batches):
        film = O.plot(w, h, scene.render(w, h, cfg["seed"], cfg["stream"], b * n, n, threads=threads)[0])
        state = observe(state, film.reshape(h, w, 3), n)
        plain += film
    robust, trim, stats = resolve(state, cfg["gain"])
    out = {"batches": batches, "paths_per_batch": n, "stats": stats,
           "trim_histogram": [int(x) for x in np.bincount(trim.reshape(-1), minlength=(m - 1) // 2 + 1)]}
    for name, film in (("plain", plain), ("robust", robust.reshape(-1, 3).astype(np.float64))):
        y = film[:, 1] / total
        out[name] = {"rel_mse_y": float(((y - ref_y) ** 2).sum() / (ref_y ** 2).sum()),
                     "firefly_pixels": int((y > cfg["firefly_factor"] * ref_y).sum())}
    return out


def resolve_pixel(s, n, gain=1.0, max_trim=NO_LIMIT):
    """One pixel, step by step as the header numbers them: s is (M, 3) float64 sums.  Returns ((X, Y, Z) float32, c, untrimmable)."""
    m = len(n)
    f = np.float64
    with np.errstate(all="ignore"):
        mean = [[f(s[j][c]) / f(n[j]) for c in range(3)] for j in range(m)]                                   # 1
        key = [mean[j][1] for j in range(m)]                                                                  # 2
        rank = [sum(1 for i in range(m) if key[i] < key[j] or (key[i] == key[j] and i < j)) for j in range(m)]  # 3
        untrimmable = any((not math.isfinite(x)) or x < 0 for x in key)                                       # 4
        c = 0
        if untrimmable:
            order = list(range(m))
        else:
            order = [0] * m
            for j in range(m):
                order[rank[j]] = j
            t, w = f(0.0), f(0.0)                                                                             # 5
            for r in range(m):
                t = t + key[order[r]]
                w = w + f(2 * r - m + 1) * key[order[r]]
            if not t > 0:
                untrimmable = True
            else:
                g = w / (f(m) * t)
                v = ((f(gain) * g) * f(m)) * f(0.5)
                cmax = _cmax(m, max_trim)
                c = 0 if not v >= 0 else (cmax if v >= f(cmax) else int(math.floor(v)))
        out = []
        for comp in range(3):                                                                                 # 6
            a = f(0.0)
            for r in range(c, m - c):
                a = a + mean[order[r]][comp]
            out.append(np.float32((a / f(m - 2 * c)) * f(sum(n))))                                            # 7
    return tuple(out), c, untrimmable
