"""rl_scene_light_paths in numpy float32, restated from the contract in include/robigo_luculenta.h ("The sample") on the pieces the
CPU oracle exports: oracle_rng_blocks for the Philox words, oracle_math_f32 for sin and cos, oracle_black_body for the emitted
intensity, and the oracle's Scene::intersect for the shadow ray.  numpy's float32 +, *, /, sqrt are correctly rounded and never
contracted, as the device's are.  rotate_towards and normalise are restated from vector3.rs:56-83.

Occlusion.  "Some object has a hit with distance < t_max and < 1e12" is decided from the oracle's nearest hit (oracle_scene_intersect:
the flat scan of scene.rs:39-60 in C++), which is the same predicate as the linear scan over oracle_intersect_object that
tests/test_gpu_occlusion.py uses -- `occluded_linear` below is that scan, and tests/test_light_abi.py holds the two against each
other -- at one library call per ray instead of one per (ray, object).  Test-only."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _oracle as O

f32 = np.float32
NONE, LIVE, ROULETTE = 0xffffffff, 0xffffffff, 2
BLACK_BODY, GREY, COLOURED = 0, 1, 2
SPHERE, CIRCLE = 0, 2
SKIPPED, BACKFACING, OCCLUDED, VISIBLE = range(4)
OFFSET = f32(0.00001)
SHORTEN = f32(0.9990234375)
SAMPLE_DTYPE = np.dtype([("direction", "<f4", 3), ("distance", "<f4"), ("value", "<f4"), ("weight", "<f4"), ("emitter", "<u4"),
                         ("status", "<u4")])
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])
assert SAMPLE_DTYPE.itemsize == 32


def emitters(objs):
    """The object indices of the sampleable emitters of an OBJECT_DTYPE description, in scan order."""
    r = objs["f"][:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        bounded = np.isfinite(r) & (r > 0)
        n = objs["v0"].astype(f32)
        n2 = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        unit = np.abs(n2 - f32(1)) <= f32(2.0 ** -20)
    kind = objs["surface_kind"]
    ok = (objs["material_kind"] == BLACK_BODY) & bounded & ((kind == SPHERE) | ((kind == CIRCLE) & unit))
    return np.flatnonzero(ok).astype(np.uint32)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _normalise(v):
    """vector3.rs:56-67: v / |v|, v itself where |v| == 0."""
    m = np.sqrt(_dot(v, v))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = v / m[:, None]
    return np.where((m == 0)[:, None], v, u).astype(f32)


def _rotate_towards(v, n):
    """vector3.rs:69-83."""
    up = np.zeros_like(n)
    up[:, 2] = 1
    a1 = _normalise(_cross(up, n))
    a2 = _normalise(_cross(a1, n))
    with np.errstate(invalid="ignore", over="ignore"):
        out = (a1 * v[:, 0:1] + a2 * v[:, 1:2]) + n * v[:, 2:3]
    mirrored = v.copy()
    mirrored[:, 2] = -v[:, 2]
    out = np.where((n[:, 2] < f32(-0.9999))[:, None], mirrored, out)
    return np.where((n[:, 2] > f32(0.9999))[:, None], v, out).astype(f32)


def draw(objs, states, hits, seed, stream):
    """The sampling half for (n,) states and hits: (samples as the call writes them when no ray is blocked, the RAY_DTYPE shadow
    rays -- all zero where none is cast)."""
    objs = np.ascontiguousarray(objs).view(O.OBJECT_DTYPE)
    n = len(states)
    out, rays = np.zeros(n, SAMPLE_DTYPE), np.zeros(n, RAY_DTYPE)
    out["emitter"] = NONE
    em = emitters(objs)
    obj = hits["object"].astype(np.int64)
    inside = obj < len(objs)
    material = np.full(n, 99, np.int64)
    material[inside] = objs["material_kind"][obj[inside]]
    sampled = (((states["end"] == LIVE) | (states["end"] == ROULETTE)) & (states["segments"] >= 1) & inside &
               ((material == GREY) | (material == COLOURED)) & (len(em) > 0))
    rows = np.flatnonzero(sampled)
    if not len(rows):
        return out, rays
    st, ht = states[rows], hits[rows]
    w = np.zeros((len(rows), 4), np.uint32)
    paths = np.ascontiguousarray(st["path_index"], dtype=np.uint64)
    blocks = (st["segments"].astype(np.uint64) + np.uint64(0x80000000)).astype(np.uint32)   # (a 32-bit sum)
    O.lib().oracle_rng_blocks(int(seed), int(stream), O.ptr(paths), O.ptr(np.ascontiguousarray(blocks)), O.ptr(w), len(rows))
    k = ((w[:, 2].astype(np.uint64) * np.uint64(len(em))) >> np.uint64(32)).astype(np.int64)
    half = (w[:, 0] >> 8).astype(f32) * f32(5.9604644775390625e-8)           # rand 0.3.11: 24 bits in [0, 1)
    u = half * (f32(16777216.0) / f32(16777215.0))                           # Closed01
    phi = (w[:, 1] >> 8).astype(f32) * f32(5.9604644775390625e-8) * f32(3.14159274101257324) * f32(2)
    cos_phi, sin_phi = O.math_f32("cos", phi), O.math_f32("sin", phi)
    e = objs[em[k]]
    radius = e["f"][:, 0].astype(f32)
    circle = e["surface_kind"] == CIRCLE
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        # a sphere (c, R)
        z = f32(1) - f32(2) * u
        r = np.sqrt(np.maximum(f32(0), f32(1) - z * z))
        nl_s = np.stack([r * cos_phi, r * sin_phi, z], axis=1)
        q_s = e["v0"] + nl_s * radius[:, None]
        area_s = f32(4) * radius * radius
        # a circle (n, p, R)
        r = radius * np.sqrt(u)
        flat = np.stack([r * cos_phi, r * sin_phi, np.zeros_like(r)], axis=1)
        nl_c = e["v0"].astype(f32)
        q_c = e["v1"] + _rotate_towards(flat, nl_c)
        area_c = radius * radius
        nl = np.where(circle[:, None], nl_c, nl_s).astype(f32)
        q = np.where(circle[:, None], q_c, q_s).astype(f32)
        area4 = np.where(circle, area_c, area_s).astype(f32)
        # the vertex
        x, normal = ht["position"].astype(f32), ht["normal"].astype(f32)
        facing = np.where((_dot(st["direction"].astype(f32), normal) >= 0)[:, None], normal, -normal)
        v = q - x
        d2 = _dot(v, v)
        usable = (d2 > 0) & np.isfinite(d2)
        distance = np.sqrt(d2)
        direction = _normalise(v)
        cos_s = _dot(facing, direction)
        along = _dot(nl, direction)
        cos_l = np.where(circle, np.abs(along), -along)
        front = usable & (cos_s > 0) & (cos_l > 0) & np.isfinite(cos_s) & np.isfinite(cos_l)
        emitted = np.zeros(len(rows), f32)
        L = O.lib()
        for j in np.flatnonzero(front):
            emitted[j] = L.oracle_black_body(f32(e["m"][j, 0]), f32(e["m"][j, 1]), f32(st["wavelength"][j]), None)
        weight = (emitted * ((cos_s * cos_l) / d2)) * (area4 * f32(len(em)))
        origin = x + direction * OFFSET
        t_max = (distance - OFFSET) * SHORTEN
        value = st["intensity"].astype(f32) * weight
    o = out[rows]
    o["emitter"] = em[k]
    o["status"] = np.where(front, VISIBLE, BACKFACING)
    o["direction"] = np.where(usable[:, None], direction, 0)
    o["distance"] = np.where(usable, distance, 0)
    o["weight"] = np.where(front, weight, 0)
    o["value"] = np.where(front, value, 0)
    out[rows] = o
    ry = rays[rows]
    ry["origin"] = np.where(front[:, None], origin, 0)
    ry["direction"] = np.where(front[:, None], direction, 0)
    ry["t_max"] = np.where(front, t_max, 0)
    rays[rows] = ry
    return out, rays


class Occluder:
    """rl_scene_occluded for rays with unit directions on the CPU oracle's scene."""

    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs).view(O.OBJECT_DTYPE)
        self.scene = O.Scene(self.objs, O.RlCameraDesc.from_buffer_copy(bytes(cam)))

    def occluded(self, rays, threads=16):
        """1 where the nearest hit of Scene::intersect (itself below 1e12) lies below t_max; a t_max that is NaN, zero or negative
        never blocks."""
        n = len(rays)
        out = np.zeros(n, np.uint8)
        L, h = O.lib(), self.scene.h
        o = np.ascontiguousarray(rays["origin"], dtype=np.float32)
        d = np.ascontiguousarray(rays["direction"], dtype=np.float32)
        t = rays["t_max"]
        todo = np.flatnonzero(t > 0)

        def work(part):
            isect = np.zeros(10, np.float32)
            for i in part:
                idx = L.oracle_scene_intersect(h, O.ptr(o[i]), O.ptr(d[i]), O.ptr(isect))
                out[i] = 1 if idx >= 0 and isect[9] < t[i] else 0

        if len(todo):
            with ThreadPoolExecutor(threads) as pool:
                list(pool.map(work, np.array_split(todo, max(1, min(threads * 4, len(todo))))))
        return out

    def occluded_linear(self, rays):
        """The same by the linear scan over oracle_intersect_object with the `< t_max`, `< 1e12` filter."""
        out = np.zeros(len(rays), np.uint8)
        for i, ray in enumerate(rays):
            if not ray["t_max"] > 0:
                continue
            for index in range(len(self.objs)):
                hit = self.scene.intersect_object(index, ray["origin"], ray["direction"])
                if hit is not None and hit[9] < ray["t_max"] and hit[9] < f32(1e12):
                    out[i] = 1
                    break
        return out


def light_paths(occluder, states, hits, seed, stream, list=None, n_list=None, samples=None):
    """rl_scene_light_paths: samples (n,) SAMPLE_DTYPE (made zeroed when None) with the records of the listed states written."""
    n = len(states)
    if samples is None:
        samples = np.zeros(n, SAMPLE_DTYPE)
    if list is None:
        named = np.arange(n if n_list is None else n_list)
    else:
        named = np.asarray(list, dtype=np.uint32)[:n_list].astype(np.int64)
        named = named[named < n]
    drawn, rays = draw(occluder.objs, states[named], hits[named], seed, stream)
    blocked = occluder.occluded(rays).astype(bool) & (drawn["status"] == VISIBLE)
    drawn["status"][blocked] = OCCLUDED
    drawn["value"][blocked] = 0
    samples[named] = drawn
    return samples
