"""The adaptive sampler's rules restated in numpy (include/robigo_luculenta.h, "adaptive sampling"): the plan -- cells, shares,
floor plus largest remainder, weights, in f64 in the header's order -- and the screen position of a sample in f32; and the ctypes
view of tests/adaptive_host, the g++ compile of the library's own plan rule and per-sample header.  Test-only; nothing is built at
import."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "adaptive_host", "_build", "librl_adaptive_host.so")
TILE = 16
PLAN_OK, PLAN_OVERFLOW, PLAN_EMPTY_TILE, PLAN_REMAINDER = range(4)
CAMERA_DTYPE = np.dtype([("ray", [("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")]),
                         ("x", "<f4"), ("y", "<f4"), ("reserved0", "<u4"), ("reserved1", "<u4")])
PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])
_lib = None


def tiles_of(w, h):
    return -(-w // TILE), -(-h // TILE)


def axis_cells(size):
    """(lo, hi) of every tile column of an axis of `size` pixels, f64: [max(0, 16 i - 0.5), min(size - 1, 16 i + 15.5)]."""
    i = np.arange(-(-size // TILE), dtype=np.float64)
    return np.maximum(0.0, 16.0 * i - 0.5), np.minimum(np.float64(size) - 1.0, 16.0 * i + 15.5)


def cells(w, h):
    """(tiles, 4) f64 {x_lo, x_hi, y_lo, y_hi} in raster order, and the areas."""
    tx, ty = tiles_of(w, h)
    xl, xh = axis_cells(w)
    yl, yh = axis_cells(h)
    c = np.zeros((ty, tx, 4))
    c[:, :, 0], c[:, :, 1], c[:, :, 2], c[:, :, 3] = xl[None, :], xh[None, :], yl[:, None], yh[:, None]
    c = c.reshape(-1, 4)
    return c, (c[:, 1] - c[:, 0]) * (c[:, 3] - c[:, 2])


def shares(w, h, importance, uniform_share):
    """(q_t, G, status): the header's shares, f64 in its order."""
    _, a = cells(w, h)
    area = (np.float64(w) - 1.0) * (np.float64(h) - 1.0)
    qa = a / area
    if importance is None:
        return qa, np.float64(0), PLAN_OK
    g = np.asarray(importance, dtype=np.float64).reshape(-1)
    assert len(g) == len(a)
    with np.errstate(all="ignore"):
        g = np.where((g > 0) & (g < np.inf), g, 0.0)
        total = np.float64(0)
        for v in g:                       # the sequential sum in raster order
            total = total + v
    if not total < np.inf:
        return None, total, PLAN_OVERFLOW
    if total == 0:
        return qa, total, PLAN_OK
    u = np.float64(uniform_share)
    return u * qa + (np.float64(1.0) - u) * (g / total), total, PLAN_OK


def plan(w, h, importance, uniform_share, n):
    """(status, counts uint32, weights float32, G): rl_adaptive_unit_plan's rule."""
    q, total, status = shares(w, h, importance, uniform_share)
    if status != PLAN_OK:
        return status, None, None, total
    _, a = cells(w, h)
    area = (np.float64(w) - 1.0) * (np.float64(h) - 1.0)
    e = np.float64(n) * q
    f = np.floor(e)
    c = f.astype(np.uint64)
    rest = e - f
    given = int(c.sum())
    if given > n or n - given > len(c):
        return PLAN_REMAINDER, None, None, total
    order = np.argsort(-rest, kind="stable")          # the largest remainder first, ties to the lower tile index
    c[order[:n - given]] += np.uint64(1)
    if (c == 0).any():
        return PLAN_EMPTY_TILE, None, None, total
    weights = ((np.float64(n) * a) / (area * c.astype(np.float64))).astype(np.float32)
    return PLAN_OK, c.astype(np.uint32), weights, total


def offsets(counts):
    off = np.zeros(len(counts) + 1, np.uint64)
    off[1:] = np.cumsum(counts.astype(np.uint64))
    return off.astype(np.uint32)


def tile_of(counts, j):
    """The tile of samples j (array): the t with off[t] <= j < off[t + 1]."""
    off = np.zeros(len(counts) + 1, np.uint64)
    off[1:] = np.cumsum(counts.astype(np.uint64))
    return (np.searchsorted(off, np.asarray(j, dtype=np.uint64), side="right") - 1).astype(np.uint32)


def closed01(word):
    """rl_get_unit of an RNG word (rl_rng.h), f32."""
    f = np.float32
    return (np.asarray(word, np.uint32) >> np.uint32(8)).astype(f) * f(5.9604644775390625e-8) * (f(16777216.0) / f(16777215.0))


def screen(lo, hi, u, m1):
    """The header's position arithmetic, f32 in its order: (px, x) with px = lo + (hi - lo) * u, x = (px / m1 - 0.5) * 2."""
    f = np.float32
    lo, hi, u = np.asarray(lo, f), np.asarray(hi, f), np.asarray(u, f)
    p = lo + (hi - lo) * u
    return p, (p / f(m1) - f(0.5)) * f(2.0)


def positions(w, h, cell, u, v):
    """(px, py, x, y) of samples in cells `cell` ((n, 4), any float type) with unit draws u, v."""
    f = np.float32
    c = np.asarray(cell).astype(f)
    px, x = screen(c[:, 0], c[:, 1], u, f(w) - f(1.0))
    py, y = screen(c[:, 2], c[:, 3], v, f(h) - f(1.0))
    return px, py, x, y / (f(w) / f(h))


def whole_film_tolerances(size, cam):
    """On a square film of one cell ([0, size - 1]^2, size <= 16) a sample must agree with rl_scene_camera_rays' for the same path,
    which takes x = u * 2 - 1.  (tol_xy, tol_direction), from the two formulas:
      the reference: 2u - 1 rounds once, onto a grid of 2^-24 below 1: 2^-25.
      the plan's: p = (m1 - 0) * u rounds by half an ulp of m1 = size - 1; p / m1 carries that over m1 and rounds by 2^-25 (a
      quotient <= 1); minus 0.5 rounds by at most 2^-26 (exact from 0.25 up); times 2 doubles all three.  y / aspect is y / 1.
    The ray: the origin depends on the lens and the camera time alone and is equal bit for bit.  The direction is the unit vector
    of v = focus - lens with focus = (x zoom, sd, -y zoom) F / sd and lens.y = 0, so |v| >= F and a change of (dx, dy) moves v / |v|
    by at most zoom * |(dx, dy)| / sd; zoom <= 1 + |chromatic_abberation| (|wavelength - 580| <= 200).  Each chain rounds some 30
    times on values no larger than the vector itself (two normalisations, a quotient, a difference, two quaternion products): 32
    half-ulps of 1 for each of the two."""
    m1 = float(size - 1)
    half_ulp_m1 = 2.0 ** (math.floor(math.log2(m1)) - 24)
    tol_xy = 2.0 * (half_ulp_m1 / m1 + 2.0 ** -25 + 2.0 ** -26) + 2.0 ** -25
    sd = 1.0 / math.tan(float(cam.fov_over_pi) * math.pi * 0.5)
    zoom = 1.0 + abs(float(cam.chromatic_abberation))
    return tol_xy, zoom * math.sqrt(2.0) * tol_xy / sd + 2 * 32 * 2.0 ** -25


# ---- tests/adaptive_host --------------------------------------------------------------------------------------------------------

def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "adaptive_host")], check=True)
        L = C.CDLL(SO)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.adaptive_scene_create.restype = vp
        L.adaptive_scene_create.argtypes = [vp, u32, vp]
        L.adaptive_scene_destroy.argtypes = [vp]
        L.adaptive_plan.restype = C.c_int
        L.adaptive_plan.argtypes = [u32, u32, vp, C.c_double, u64, vp, vp, vp, vp]
        L.adaptive_samples.argtypes = [vp, u32, u32, vp, vp, vp, u32, u64, u32, u64, u32, u32, vp]
        L.adaptive_render.argtypes = [vp, vp, u64, u32, u64, u32, u32, vp, vp]
        _lib = L
    return _lib


def host_plan(w, h, importance, uniform_share, n):
    """The library's own rule, compiled for the host: (status, counts, weights, cells (tiles, 4) float32, G)."""
    tx, ty = tiles_of(w, h)
    counts, weights, cell = np.zeros(tx * ty, np.uint32), np.zeros(tx * ty, np.float32), np.zeros((tx * ty, 4), np.float32)
    g = np.ascontiguousarray(importance, dtype=np.float64).reshape(-1) if importance is not None else None
    total = C.c_double(0)
    status = lib().adaptive_plan(w, h, g.ctypes.data if g is not None else None, uniform_share, n, counts.ctypes.data, weights.ctypes.data,
                                 cell.ctypes.data, C.byref(total))
    return status, counts, weights, cell, total.value


class HostScene:
    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs)
        self.h = lib().adaptive_scene_create(self.objs.ctypes.data, len(self.objs), C.byref(cam))
        assert self.h

    def __del__(self):
        try:
            lib().adaptive_scene_destroy(self.h)
        except Exception:
            pass

    def samples(self, w, h, counts, weights, seed, stream, first_path, first_sample, n):
        """rl_adaptive_unit_samples on the CPU for the plan (counts, weights) of a w x h film."""
        cell = cells(w, h)[0].astype(np.float32)
        off = offsets(counts)
        weights = np.ascontiguousarray(weights, np.float32)
        out = np.zeros(n, CAMERA_DTYPE)
        lib().adaptive_samples(self.h, w, h, off.ctypes.data, np.ascontiguousarray(cell).ctypes.data, weights.ctypes.data, len(counts), seed, stream,
                               first_path, first_sample, n, out.ctypes.data)
        return out

    def render(self, samples, seed, stream, first_path, first_sample=0, threads=16):
        """(photons, values): what rl_plot_unit_render_adaptive splats for `samples` (samples first_sample .. of a plan) -- x, y,
        f32(value * w_t), wavelength -- and the unweighted values, which are rl_scene_render_rays' for the same rays.  The host compile
        of the kernel's per-path header, which tests/test_host_mirror.py holds to the CPU oracle; threaded (the calls release the GIL)."""
        from concurrent.futures import ThreadPoolExecutor
        samples = np.ascontiguousarray(samples, CAMERA_DTYPE)
        n = len(samples)
        photons, values = np.zeros(n, PHOTON_DTYPE), np.zeros(n, np.float32)
        step = max(1, -(-n // (4 * threads)))

        def work(lo):
            k = min(step, n - lo)
            lib().adaptive_render(self.h, samples[lo:].ctypes.data, seed, stream, first_path, first_sample + lo, k, photons[lo:].ctypes.data,
                                  values[lo:].ctypes.data)

        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(work, range(0, n, step)))
        return photons, values


# ---- uniform against adaptive, on the CPU ------------------------------------------------------------------------------------------

GAIN = dict(w=64, h=36, n=1 << 16, warmup=4, budgets=(8, 16, 32), seed=1, stream=0, share=0.25, n_ref=1 << 23, ref_stream=1)
GAIN_TEST_BUDGET = 16       # the budget tests/test_gpu_adaptive.py runs on the device


def gain_metrics(state, total_xyz, paths, ref_mean):
    """relative_error and worst_tile_error of the error oracle's estimate, and the mean squared error of the XYZ mean against ref_mean."""
    import _error_oracle as EO
    stats = EO.estimate(state)[0]
    mse = float(((total_xyz / paths - ref_mean) ** 2).mean())
    return {"relative_error": float(stats["relative_error"]), "worst_tile_error": float(stats["worst_tile_error"]), "mse": mse}


def cpu_gain(objs, cam, adaptive_sampling, ref_mean, cfg=GAIN):
    """render_adaptive_to_error(target 0) restated on the CPU: batches of cfg["n"] paths, the uniform plan until the error oracle has
    cfg["warmup"] observations, then re-planned from its tile map before every batch (or never: the uniform sampler through the same
    code); the film of a batch is the oracle's plot of its weighted photons.  {budget: gain_metrics} at cfg["budgets"]."""
    import _error_oracle as EO
    import _oracle as O
    w, h, n = cfg["w"], cfg["h"], cfg["n"]
    host = HostScene(np.ascontiguousarray(objs), cam)
    state, total, out = EO.new_state(w, h), np.zeros((h * w, 3), np.float64), {}
    status, counts, weights, _ = plan(w, h, None, cfg["share"], n)
    for batch in range(max(cfg["budgets"])):
        first = batch * n
        samples = host.samples(w, h, counts, weights, cfg["seed"], cfg["stream"], first, 0, n)
        photons = host.render(samples, cfg["seed"], cfg["stream"], first)[0]
        film = O.plot(w, h, photons)
        state = EO.observe(state, film.reshape(h, w, 3), n)
        total += film
        if batch + 1 in cfg["budgets"]:
            out[batch + 1] = gain_metrics(state, total, (batch + 1) * n, ref_mean)
        if adaptive_sampling and batch + 1 >= max(2, cfg["warmup"]):
            tiles = EO.estimate(state)[2]
            status, counts, weights, _ = plan(w, h, tiles[:, :, 0].reshape(-1), cfg["share"], n)
            assert status == PLAN_OK
    return out


def cpu_reference_mean(objs, cam, cfg=GAIN):
    """The XYZ mean per path of cfg["n_ref"] uniform paths of another stream, from the CPU oracle: (h * w, 3) float64."""
    import _oracle as O
    photons, _ = O.Scene(np.ascontiguousarray(objs).view(O.OBJECT_DTYPE), O.RlCameraDesc.from_buffer_copy(bytes(cam))).render(
        cfg["w"], cfg["h"], cfg["seed"], cfg["ref_stream"], 0, cfg["n_ref"], threads=16)
    return O.plot(cfg["w"], cfg["h"], photons).astype(np.float64) / cfg["n_ref"]
