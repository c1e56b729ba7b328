"""One turn of TraceUnit::render_ray's loop (trace_unit.rs:92-126) in Python on the pieces the CPU oracle exports, built as
tests/_path_oracle.py builds the whole loop: state in, state and hit out.  oracle_scene_intersect for the segment,
oracle_material_bounce with block 2 + segments, oracle_black_body for a light, oracle_rng_block and oracle_math_f32 (exp) for the
roulette; the f32 steps between them in numpy float32 in the reference's order.  The records are RlPathState and RlRayHit of
include/robigo_luculenta.h.  Test-only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _oracle as O
from _path_oracle import BLACK_BODY, EMITTER, INVALID, NONE, ROULETTE, VOID, _unit, f32

LIVE = 0xffffffff
NO_ROULETTE = 1
STATE_DTYPE = np.dtype([("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("intensity", "<f4"),
                        ("continue_chance", "<f4"), ("segments", "<u4"), ("end", "<u4"), ("value", "<f4"), ("path_index", "<u8"),
                        ("object", "<u4"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("distance", "<f4"), ("object", "<u4"),
                      ("reserved", "<u4")])
assert STATE_DTYPE.itemsize == 64 and HIT_DTYPE.itemsize == 48


def begin(rays, first=0):
    """rl_scene_begin_paths: SPECTRAL_RAY records (origin, wavelength, direction) as states of paths first .. first + n - 1."""
    s = np.zeros(len(rays), dtype=STATE_DTYPE)
    s["origin"], s["wavelength"], s["direction"] = rays["origin"], rays["wavelength"], rays["direction"]
    s["intensity"] = s["continue_chance"] = 1.0
    s["end"] = np.where(np.isfinite(rays["wavelength"]), LIVE, INVALID)
    s["path_index"] = np.uint64(first) + np.arange(len(rays), dtype=np.uint64)
    s["object"] = NONE
    return s


def roulette_ends(seed, stream, path, block, intensity, continue_chance):
    """trace_unit.rs:122-125 for a bounce that drew `block`: `unit * 0.85 > continue_chance * (1 - exp(intensity * -20))`, on the
    intensity and the continue chance after the bounce."""
    L = O.lib()
    words = np.zeros(4, np.uint32)
    x, y = np.zeros(1, np.float32), np.zeros(1, np.float32)
    L.oracle_rng_block(int(seed), int(stream), int(path), int(block), O.ptr(words))
    x[0] = f32(intensity) * f32(-20.0)
    L.oracle_math_f32(3, O.ptr(x), O.ptr(y), 1)   # rl_expf
    return bool(_unit(words[2]) * f32(0.85) > f32(continue_chance) * (f32(1) - y[0]))


class StepOracle:
    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs).view(O.OBJECT_DTYPE)
        self.scene = O.Scene(self.objs, O.RlCameraDesc.from_buffer_copy(bytes(cam)))

    def step_one(self, state, hit, seed, stream, flags=0):
        """Steps the 0-d record views `state` (and `hit`, or None) in place; a state that is not live is left alone."""
        if int(state["end"]) != LIVE:
            return
        L = O.lib()
        o = np.array(state["origin"], dtype=np.float32)
        d = np.array(state["direction"], dtype=np.float32)
        wl = f32(state["wavelength"])
        isect = np.zeros(10, np.float32)
        idx = L.oracle_scene_intersect(self.scene.h, O.ptr(o), O.ptr(d), O.ptr(isect))
        block = (2 + int(state["segments"])) & 0xffffffff          # 32-bit sums, as RlPathState::segments says: they wrap
        state["segments"] = (int(state["segments"]) + 1) & 0xffffffff
        state["value"], state["object"], state["reserved"] = f32(0), NONE, 0
        if hit is not None:
            hit["position"], hit["normal"], hit["tangent"] = (isect[0:3], isect[3:6], isect[6:9]) if idx >= 0 else (0, 0, 0)
            hit["distance"] = isect[9] if idx >= 0 else f32(0)
            hit["object"], hit["reserved"] = (idx if idx >= 0 else NONE), 0
        if idx < 0:
            state["end"] = VOID
            return
        ob = self.objs[idx]
        kind, m = int(ob["material_kind"]), ob["m"]
        if kind == BLACK_BODY:
            state["value"] = f32(state["intensity"]) * f32(L.oracle_black_body(f32(m[0]), f32(m[1]), wl, None))
            state["object"], state["end"] = idx, EMITTER
            return
        in7, out7 = np.zeros(7, np.float32), np.zeros(7, np.float32)
        in7[0:3], in7[3:6], in7[6] = o, d, wl
        path = int(state["path_index"])
        L.oracle_material_bounce(kind, f32(m[0]), f32(m[1]), f32(m[2]), O.ptr(in7), O.ptr(isect), seed, stream, path, block, O.ptr(out7))
        nd = out7[3:6].copy()
        intensity = f32(state["intensity"]) * out7[6]
        cc = f32(state["continue_chance"]) * f32(0.96)
        state["direction"] = nd
        state["origin"] = (out7[0:3] + nd * f32(1e-5)).astype(np.float32)
        state["intensity"], state["continue_chance"] = intensity, cc
        if not (flags & NO_ROULETTE) and roulette_ends(seed, stream, path, block, intensity, cc):
            state["end"] = ROULETTE

    def step(self, states, seed, stream, flags=0, hits=None, threads=16):
        """rl_scene_step_paths on an (n,) STATE_DTYPE array (and an (n,) HIT_DTYPE array or None), in place (a thread pool: the
        oracle's calls release the GIL)."""
        n = len(states)

        def work(lo, hi):
            for i in range(lo, hi):
                self.step_one(states[i:i + 1].reshape(()), None if hits is None else hits[i:i + 1].reshape(()), seed, stream, flags)

        chunk = max(1, (n + 63) // 64)
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda lo: work(lo, min(n, lo + chunk)), range(0, n, chunk)))
        return states

    def run(self, rays, seed, stream, first=0, max_steps=4096):
        """begin, then step until nothing is live: (final states, steps taken)."""
        s = begin(rays, first)
        steps = 0
        while (s["end"] == LIVE).any() and steps < max_steps:
            live = np.flatnonzero(s["end"] == LIVE)
            sub = s[live]
            self.step(sub, seed, stream)
            s[live] = sub
            steps += 1
        return s, steps
