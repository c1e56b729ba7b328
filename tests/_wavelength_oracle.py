"""Wavelength importance sampling restated in numpy (include/robigo_luculenta.h, "wavelength importance sampling"): the table -- f64
in the header's order -- and what a path makes of it in f32; and the ctypes view of tests/wavelength_host, the g++ compile of the
library's own rule and per-path header.  Test-only; nothing is built at import."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "wavelength_host", "_build", "librl_wavelength_host.so")
M = 256
TABLE_FLOATS = 2 * M + 1
OK, OVERFLOW, NOT_INCREASING = range(3)
PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])
_lib = None


def cie_importance():
    """x-bar + y-bar + z-bar at the observer's 81 nodes, from the golden copy of the reference's table: f64 sums of the f32 values."""
    with open(os.path.join(HERE, "golden", "cie1931_xyz.json")) as f:
        d = json.load(f)
    x, y, z = (np.asarray(d[k], dtype=np.float32).astype(np.float64) for k in "XYZ")
    return (x + y) + z


def one_hot(n_nodes, k):
    g = np.zeros(n_nodes)
    g[k] = 1.0
    return g


def table(importance, n_nodes, uniform_share):
    """(status, Q float32[257], W float32[256]): the header's rule."""
    n, u = int(n_nodes), np.float64(uniform_share)
    nm1 = np.float64(n - 1)
    guided = False
    if importance is not None:
        g = np.asarray(importance, dtype=np.float64).reshape(-1)
        assert len(g) == n
        with np.errstate(all="ignore"):
            g = np.where((g > 0) & (g < np.inf), g, 0.0)
            m = (g[:-1] + g[1:]) * 0.5
            total = np.add.accumulate(m)[-1]          # the sequential sum from +0.0
        if not total < np.inf:
            return OVERFLOW, None, None
        guided = total > 0
    if guided:
        d = u / nm1 + (np.float64(1.0) - u) * (m / total)
    else:
        d = np.full(n - 1, np.float64(1.0) / nm1)
    c = np.concatenate([[0.0], np.add.accumulate(d)])
    t = (np.arange(M + 1, dtype=np.float64) / np.float64(M)) * c[n - 1]
    j = np.searchsorted(c[:n - 1], t, side="right") - 1          # the largest j <= n - 2 with C_j <= T_i
    with np.errstate(all="ignore"):       # (a share that underflows leaves segments of no width: 0 / 0 where T_i meets one)
        lam = 380.0 + (np.float64(400.0) / nm1) * (j.astype(np.float64) + (t - c[j]) / d[j])
    q = lam.astype(np.float32)
    q[0], q[M] = 380.0, 780.0
    if not (q[1:] > q[:-1]).all():
        return NOT_INCREASING, None, None
    w = (((q[1:].astype(np.float64) - q[:-1].astype(np.float64)) * np.float64(M)) / 400.0).astype(np.float32)
    return OK, q, w


def packed(q, w):
    """The table as the device and the host compile read it: the quantiles, then the weights."""
    return np.ascontiguousarray(np.concatenate([q, w]).astype(np.float32))


def draw(q, w0):
    """The wavelength of paths whose block 0 begins with the words w0: f32 in the header's order."""
    f32 = np.float32
    v = np.asarray(w0, np.uint32) >> np.uint32(8)
    i = (v >> np.uint32(16)).astype(np.int64)
    f = (v & np.uint32(0xffff)).astype(f32) * f32(2.0 ** -16)
    return q[i] + (q[i + 1] - q[i]) * f


def bin_of(q, lam):
    """The largest i <= M - 1 with Q[i] <= lambda."""
    return (np.searchsorted(q[:M], lam, side="right") - 1).astype(np.uint32)


# ---- tests/wavelength_host ------------------------------------------------------------------------------------------------------

def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "wavelength_host")], check=True)
        L = C.CDLL(SO)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.wavelength_scene_create.restype = vp
        L.wavelength_scene_create.argtypes = [vp, u32, vp]
        L.wavelength_scene_destroy.argtypes = [vp]
        L.wavelength_table.restype = C.c_int
        L.wavelength_table.argtypes = [vp, u32, C.c_double, vp]
        L.wavelength_cie_importance.argtypes = [vp]
        L.wavelength_draws.argtypes = [vp, vp, u64, vp, vp, vp]
        L.wavelength_camera.argtypes = [vp, u32, u32, vp, u64, u32, u64, u64, vp, vp]
        L.wavelength_render.argtypes = [vp, u32, u32, vp, u64, u32, u64, u64, vp, vp, vp]
        _lib = L
    return _lib


def host_table(importance, n_nodes, uniform_share):
    """The library's own rule, compiled for the host: (status, Q, W)."""
    out = np.zeros(TABLE_FLOATS, np.float32)
    g = np.ascontiguousarray(importance, dtype=np.float64).reshape(-1) if importance is not None else None
    status = lib().wavelength_table(g.ctypes.data if g is not None else None, n_nodes, uniform_share, out.ctypes.data)
    return status, out[:M + 1].copy(), out[M + 1:].copy()


def host_cie_importance():
    out = np.zeros(81, np.float64)
    lib().wavelength_cie_importance(out.ctypes.data)
    return out


def host_draws(tab, w0):
    """(wavelength, bin_of(wavelength), weight) of the words w0 by the host compile of the per-path header."""
    w0 = np.ascontiguousarray(w0, np.uint32)
    lam, b, w = np.zeros(len(w0), np.float32), np.zeros(len(w0), np.uint32), np.zeros(len(w0), np.float32)
    lib().wavelength_draws(tab.ctypes.data, w0.ctypes.data, len(w0), lam.ctypes.data, b.ctypes.data, w.ctypes.data)
    return lam, b, w


class HostScene:
    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs)
        self.h = lib().wavelength_scene_create(self.objs.ctypes.data, len(self.objs), C.byref(cam))
        assert self.h

    def __del__(self):
        try:
            lib().wavelength_scene_destroy(self.h)
        except Exception:
            pass

    def camera(self, w, h, tab, seed, stream, first, n):
        """(rays (n, 8) {origin, wavelength, direction, ior}, xy (n, 2)) of the paths' camera half; tab None: rl_begin_path."""
        rays, xy = np.zeros((n, 8), np.float32), np.zeros((n, 2), np.float32)
        lib().wavelength_camera(self.h, w, h, tab.ctypes.data if tab is not None else None, seed, stream, first, n, rays.ctypes.data, xy.ctypes.data)
        return rays, xy

    def render(self, w, h, tab, seed, stream, first, n, threads=8):
        """(photons, segments, unweighted values) of paths first .. first + n - 1 of a trace unit with the table `tab` (None: without)."""
        from concurrent.futures import ThreadPoolExecutor
        photons, values = np.zeros(n, PHOTON_DTYPE), np.zeros(n, np.float32)
        step = max(1, -(-n // (4 * threads)))
        t = tab.ctypes.data if tab is not None else None

        def work(lo):
            k = min(step, n - lo)
            segs = C.c_uint64(0)
            lib().wavelength_render(self.h, w, h, t, seed, stream, first + lo, k, photons[lo:].ctypes.data, C.byref(segs), values[lo:].ctypes.data)
            return segs.value

        with ThreadPoolExecutor(threads) as pool:
            segments = sum(pool.map(work, range(0, n, step)))
        return photons, segments, values


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------------

def case_table(name):
    """(importance or None, n_nodes, uniform_share) of a named table."""
    if name == "cie-0.1":
        return cie_importance(), 81, 0.1
    if name == "one-hot-1e-3":
        return one_hot(81, 40), 81, 1.0e-3
    if name == "null":
        return None, 81, 1.0
    raise KeyError(name)


def case_packed(name):
    status, q, w = table(*case_table(name))
    assert status == OK
    return packed(q, w)


# ---- uniform against importance sampling, on the CPU --------------------------------------------------------------------------------

GAIN = dict(w=64, h=36, n=1 << 16, budgets=(8, 16, 32), seed=1, stream=0, share=0.1, n_ref=1 << 23, ref_stream=1)
GAIN_TEST_BUDGET = 16       # the budget tests/test_gpu_wavelength.py runs on the device


def cpu_gain(objs, cam, tab, ref_mean, cfg=GAIN):
    """Batches of cfg["n"] paths through the host compile, with the table `tab` or (None) the uniform draw, each batch's film (the
    oracle's plot of its photons) observed by the error oracle: {budget: {component: metrics}} at cfg["budgets"], the metrics being
    relative_error and worst_tile_error of the component's estimate and the MSE of its mean against ref_mean."""
    import _error_oracle as EO
    import _oracle as O
    w, h, n = cfg["w"], cfg["h"], cfg["n"]
    host = HostScene(np.ascontiguousarray(objs), cam)
    states = [EO.new_state(w, h) for _ in range(3)]
    total, out = np.zeros((h * w, 3), np.float64), {}
    for batch in range(max(cfg["budgets"])):
        photons = host.render(w, h, tab, cfg["seed"], cfg["stream"], batch * n, n)[0]
        film = O.plot(w, h, photons.view(O.PHOTON_DTYPE)).reshape(h, w, 3)
        for k in range(3):      # the error oracle reads a film's Y: each component in turn takes its place
            only = np.zeros_like(film)
            only[:, :, 1] = film[:, :, k]
            states[k] = EO.observe(states[k], only, n)
        total += film.reshape(-1, 3)
        if batch + 1 in cfg["budgets"]:
            mean = total / ((batch + 1) * n)
            out[batch + 1] = {}
            for k, name in enumerate("XYZ"):
                stats = EO.estimate(states[k])[0]
                out[batch + 1][name] = {"relative_error": float(stats["relative_error"]), "worst_tile_error": float(stats["worst_tile_error"]),
                                        "mse": float(((mean[:, k] - ref_mean[:, k]) ** 2).mean())}
    return out
