"""TraceUnit::render_ray (trace_unit.rs:81-132; oracle/rl_oracle.cpp: render_ray) restated in Python on pieces the CPU oracle
exports, for rays no camera makes: oracle_scene_intersect for every segment, oracle_material_bounce with block 2 + b for bounce b,
oracle_black_body for a light, oracle_rng_block and oracle_math_f32 (exp) for the roulette.  The f32 steps between them are done
in numpy float32, in the reference's order: the origin offset by 1e-5 * direction, the continue chance times 0.96, and
`unit * 0.85 > continue_chance * (1 - exp(intensity * -20))`.  Like rl_scene_render_rays it returns value 0 with no segment for a
non-finite wavelength (RL_PATH_END_INVALID) and ends a path after max_segments segments (RL_PATH_END_LIMIT).  Test-only."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _oracle as O

NONE = 0xffffffff
VOID, EMITTER, ROULETTE, LIMIT, INVALID = range(5)
MAX_SEGMENTS = 4096
RESULT_DTYPE = np.dtype([("value", "<f4"), ("segments", "<u4"), ("object", "<u4"), ("end", "<u4")])   # RlPathResult
BLACK_BODY = 0

f32 = np.float32
_HALF_OPEN = f32(5.9604644775390625e-8)
_CLOSED = f32(16777216.0) / f32(16777215.0)


def _unit(word):
    """rl_get_unit (rl_rng.h): closed [0, 1] from the top 24 bits of a draw."""
    return f32(int(word) >> 8) * _HALF_OPEN * _CLOSED


class PathOracle:
    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs).view(O.OBJECT_DTYPE)
        self.scene = O.Scene(self.objs, O.RlCameraDesc.from_buffer_copy(bytes(cam)))

    def render_ray(self, origin, direction, wavelength, seed, stream, path, max_segments=0):
        """(value, segments, object, end) of one ray as path `path` of (seed, stream)."""
        L = O.lib()
        wl = f32(wavelength)
        if not np.isfinite(wl):
            return f32(0), 0, NONE, INVALID
        limit = max_segments or MAX_SEGMENTS
        o = np.array(origin, dtype=np.float32)
        d = np.array(direction, dtype=np.float32)
        intensity, cc = f32(1), f32(1)
        isect = np.zeros(10, np.float32)
        in7, out7 = np.zeros(7, np.float32), np.zeros(7, np.float32)
        words = np.zeros(4, np.uint32)
        x, y = np.zeros(1, np.float32), np.zeros(1, np.float32)
        segments = 0
        while True:
            segments += 1
            idx = L.oracle_scene_intersect(self.scene.h, O.ptr(o), O.ptr(d), O.ptr(isect))
            if idx < 0:
                return f32(0), segments, NONE, VOID
            ob = self.objs[idx]
            kind, m = int(ob["material_kind"]), ob["m"]
            if kind == BLACK_BODY:
                return intensity * f32(L.oracle_black_body(f32(m[0]), f32(m[1]), wl, None)), segments, idx, EMITTER
            in7[0:3], in7[3:6], in7[6] = o, d, wl
            block = 2 + segments - 1
            L.oracle_material_bounce(kind, f32(m[0]), f32(m[1]), f32(m[2]), O.ptr(in7), O.ptr(isect), seed, stream, path, block,
                                     O.ptr(out7))
            d = out7[3:6].copy()
            intensity = intensity * out7[6]
            o = (out7[0:3] + d * f32(1e-5)).astype(np.float32)
            cc = cc * f32(0.96)
            L.oracle_rng_block(seed, stream, path, block, O.ptr(words))
            x[0] = intensity * f32(-20.0)
            L.oracle_math_f32(3, O.ptr(x), O.ptr(y), 1)   # rl_expf
            if _unit(words[2]) * f32(0.85) > cc * (f32(1) - y[0]):
                return f32(0), segments, NONE, ROULETTE
            if segments >= limit:
                return f32(0), segments, NONE, LIMIT

    def render_rays(self, origins, directions, wavelengths, seed, stream, first=0, max_segments=0, threads=16):
        """RESULT_DTYPE records for rays i = 0 .. n-1 as paths first + i (a thread pool: the oracle's calls release the GIL)."""
        n = len(origins)
        out = np.zeros(n, dtype=RESULT_DTYPE)
        wavelengths = np.broadcast_to(np.asarray(wavelengths, dtype=np.float32), (n,))

        def work(lo, hi):
            for i in range(lo, hi):
                out[i] = self.render_ray(origins[i], directions[i], wavelengths[i], seed, stream, first + i, max_segments)

        step = max(1, (n + 63) // 64)
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda lo: work(lo, min(n, lo + step)), range(0, n, step)))
        return out
