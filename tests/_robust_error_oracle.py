"""rl_robust_unit_estimate on the CPU, in the order include/robigo_luculenta.h states: the standard error of the trimmed film from
the M bucket means of Y (the winsorized sum of squares over h (h - 1), Tukey and McLaughlin 1963), per pixel and per 16 x 16 tile.
A state is _robust_oracle's (sums (M, 3, h, w) float64, n: list of M ints, k).  pixels is vector code over the pixels whose every
operation is one IEEE f64 operation per pixel and whose sums run rank by rank in the stated order; estimate_pixel is the same contract
as a plain loop over one pixel, and tests/test_robust_error.py holds the two to each other.  The tile tree and the host statistics
are _error_oracle's.  numpy only, but for gain_figures at the end, which renders with the CPU oracle.  Test-only."""
import math

import numpy as np

import _error_oracle as EO
import _robust_oracle as RO

NO_LIMIT = 0xFFFFFFFF
f64 = np.float64


def cmax_of(m, max_trim):
    """At least two buckets are kept: for odd M at full trim one less than the resolve's cap."""
    return min(max_trim, (m - 2) // 2)


def pixels(state, gain=1.0, max_trim=NO_LIMIT):
    """Per pixel, flat over h * w: dict of se float32; ay, var, f float64; c int64; untrimmable bool."""
    sums, n, k = state
    m, _, h, w = sums.shape
    assert all(x > 0 for x in n) and gain >= 0
    p = h * w
    at = np.arange(p)
    gain, md, total = f64(gain), f64(m), f64(sum(n))
    cmax = cmax_of(m, max_trim)
    with np.errstate(all="ignore"):
        key = np.empty((m, p), f64)
        for j in range(m):
            key[j] = sums[j, 1].reshape(p) / f64(n[j])
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
            wsum = wsum + f64(2 * r - m + 1) * kr
        untrimmable = bad | ~(t > 0)
        g = wsum / (md * t)
        v = ((gain * g) * md) * f64(0.5)
        inside = (v >= 0) & (v < f64(cmax))
        c = np.where(inside, np.floor(np.where(inside, v, 0.0)), np.where(v >= f64(cmax), cmax, 0)).astype(np.int64)
        c = np.where(untrimmable, 0, c)
        kept = m - 2 * c
        lo, hi = key[perm[c, at], at], key[perm[m - c - 1, at], at]
        a = np.zeros(p)
        for r in range(m):
            a = np.where((r >= c) & (r < m - c), a + key[perm[r], at], a)
        cd = c.astype(f64)
        b = cd * lo + a
        b = b + cd * hi
        mw = b / md
        d = np.zeros(p)
        for r in range(m):
            e = key[perm[r], at] - mw
            d = np.where((r >= c) & (r < m - c), d + e * e, d)
        el = lo - mw
        d = d + cd * (el * el)
        eh = hi - mw
        d = d + cd * (eh * eh)
        var = d / (kept * (kept - 1)).astype(f64)
        f = (a / kept.astype(f64)) * total
        vv = (var * total) * total
        se = np.sqrt(vv.astype(np.float32))
        ay = np.abs(f)
    return {"se": se, "ay": ay, "var": var, "f": f, "c": c, "untrimmable": untrimmable}


def estimate(state, gain=1.0, max_trim=NO_LIMIT):
    """rl_robust_unit_estimate: (stats dict, se (h, w) float32, tiles (tiles_y, tiles_x, 2) float64, trim (h, w) uint8 with bit 7
    set for an untrimmable pixel)."""
    sums, n, k = state
    h, w = sums.shape[2:]
    px = pixels(state, gain, max_trim)
    se = px["se"].reshape(h, w)
    tiles = np.stack([EO.tile_tree(se.astype(f64)), EO.tile_tree(px["ay"].reshape(h, w))], axis=2)
    trim = (px["c"] | np.where(px["untrimmable"], 0x80, 0)).astype(np.uint8).reshape(h, w)
    return EO.host_stats(tiles, k, sum(n)), se, tiles, trim


def estimate_pixel(s, n, gain=1.0, max_trim=NO_LIMIT):
    """One pixel, step by step as the header numbers them: s is the M Y sums.  Returns (se float32, ay, var, f, c, untrimmable)."""
    m = len(n)
    with np.errstate(all="ignore"):
        key = [f64(s[j]) / f64(n[j]) for j in range(m)]                                                       # 1
        rank = [sum(1 for i in range(m) if key[i] < key[j] or (key[i] == key[j] and i < j)) for j in range(m)]
        untrimmable = any((not math.isfinite(x)) or x < 0 for x in key)
        c = 0
        if untrimmable:
            order = list(range(m))
        else:
            order = [0] * m
            for j in range(m):
                order[rank[j]] = j
            t, w = f64(0.0), f64(0.0)
            for r in range(m):
                t = t + key[order[r]]
                w = w + f64(2 * r - m + 1) * key[order[r]]
            if not t > 0:
                untrimmable = True
            else:
                g = w / (f64(m) * t)
                v = ((f64(gain) * g) * f64(m)) * f64(0.5)
                cmax = cmax_of(m, max_trim)
                c = 0 if not v >= 0 else (cmax if v >= f64(cmax) else int(math.floor(v)))
        kept = m - 2 * c
        lo, hi = key[order[c]], key[order[m - c - 1]]                                                         # 2
        a = f64(0.0)
        for r in range(c, m - c):
            a = a + key[order[r]]
        b = f64(c) * lo + a                                                                                   # 3
        b = b + f64(c) * hi
        mw = b / f64(m)
        d = f64(0.0)                                                                                          # 4
        for r in range(c, m - c):
            e = key[order[r]] - mw
            d = d + e * e
        el = lo - mw
        d = d + f64(c) * (el * el)
        eh = hi - mw
        d = d + f64(c) * (eh * eh)
        var = d / f64(kept * (kept - 1))                                                                      # 5
        total = f64(sum(n))                                                                                   # 6
        f = (a / f64(kept)) * total
        vv = (var * total) * total
        se = np.sqrt(np.float32(vv))
        ay = abs(f)
    return se, ay, var, f, c, untrimmable


# ---- the plain noise estimate against the robust one, on the CPU (tools/robust_error_gain.py, tests/golden/robust_error_gain.json) --

GAIN = dict(RO.GAIN, uniform_share=0.25)
# (scene: 1 the glass-stress scene, 0 the demo scene; batches; paths per batch), the smallest first: tests/test_robust_error.py
# re-derives it
GAIN_CONFIGS = [(1, 15, 1024), (1, 60, 8192), (0, 60, 8192), (1, 240, 8192), (0, 240, 8192)]


def gain_figures(objs, cam, batches, n, cfg=GAIN, threads=16):
    """`batches` batches of n paths of cfg["stream"], each shown to the plain error oracle and to bucket b % M of the robust state:
    relative_error of both estimates on these buffers; the firefly pixels (_robust_oracle.gain_figures' definition and reference: the
    plain Y per path above firefly_factor times that of ref_factor times as many paths of ref_stream); and the share of the next
    adaptive batch of n paths that _adaptive_oracle's plan gives to the tiles that hold a firefly pixel, with each estimate's t_se
    as the importance."""
    import _adaptive_oracle as AO
    import _oracle as O
    w, h, m = cfg["w"], cfg["h"], cfg["buckets"]
    scene = O.Scene(np.ascontiguousarray(objs), cam)
    total = batches * n
    ref = O.plot(w, h, scene.render(w, h, cfg["seed"], cfg["ref_stream"], 0, cfg["ref_factor"] * total, threads=threads)[0])
    ref_y = ref.astype(f64)[:, 1] / (cfg["ref_factor"] * total)
    robust, plain_error, plain = RO.new_state(w, h, m), EO.new_state(w, h), np.zeros((h * w, 3), f64)
    for b in range(batches):
        film = O.plot(w, h, scene.render(w, h, cfg["seed"], cfg["stream"], b * n, n, threads=threads)[0]).reshape(h, w, 3)
        robust = RO.observe(robust, film, n)
        plain_error = EO.observe(plain_error, film, n)
        plain += film.reshape(-1, 3)
    fireflies = (plain[:, 1] / total > cfg["firefly_factor"] * ref_y).reshape(h, w)
    ty, tx = -(-h // EO.TILE), -(-w // EO.TILE)
    padded = np.zeros((ty * EO.TILE, tx * EO.TILE), bool)
    padded[:h, :w] = fireflies
    firefly_tiles = padded.reshape(ty, EO.TILE, tx, EO.TILE).any(axis=(1, 3))
    out = {"batches": batches, "paths_per_batch": n, "firefly_pixels": int(fireflies.sum()), "firefly_tiles": int(firefly_tiles.sum()),
           "tiles": int(ty * tx)}
    plain_stats, _, plain_tiles = EO.estimate(plain_error)
    robust_stats, _, robust_tiles, trim = estimate(robust, cfg["gain"])
    out["trimmed_pixels"] = int(((trim & 0x7F) > 0).sum())
    for name, stats, tiles in (("plain", plain_stats, plain_tiles), ("robust", robust_stats, robust_tiles)):
        status, counts, _, _ = AO.plan(w, h, tiles[:, :, 0].reshape(-1), cfg["uniform_share"], n)
        share = None                                       # (a plan the rule refuses gives no share)
        if status == AO.PLAN_OK:
            counts = counts.astype(np.int64).reshape(ty, tx)
            share = float(counts[firefly_tiles].sum() / counts.sum())
        out[name] = {"relative_error": stats["relative_error"], "worst_tile_error": stats["worst_tile_error"], "firefly_tile_share": share}
    return out
