"""rl_scene_light_paths* at the boundary, without a GPU: the record, the entry points and their argument checks in the documented
order, the emitters of a description, the host compile of the sampling function (rl_debug_light_sample) against the numpy
restatement (tests/_light_oracle.py) bit for bit, the estimator's mean against the path's own emitter hits on the CPU oracle, and
the compiled kernels' resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
import _light_oracle as LO
import _oracle as O
import _random_scene as RS
import _rng_width as RW
import _step_oracle as S
from _boundary import _err, _FakeScene
from _cases import bounce_directions, vertex_states
from _compare import assert_means_agree
from _device_build import kernels, variant_of_name  # noqa: F401  (kernels is a fixture)
from _scenes import _with_lights, closed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
ENTRY_POINTS = ("rl_scene_light_paths", "rl_scene_light_paths_device")
W, H = 320, 180


def test_the_record_is_as_specified():
    assert C.sizeof(_lib.RlLightSample) == R.LIGHT_SAMPLE_DTYPE.itemsize == LO.SAMPLE_DTYPE.itemsize == 32
    offsets = {"direction": 0, "distance": 12, "value": 16, "weight": 20, "emitter": 24, "status": 28}
    for name, off in offsets.items():
        assert getattr(_lib.RlLightSample, name).offset == off == R.LIGHT_SAMPLE_DTYPE.fields[name][1], name
    assert (R.RL_LIGHT_SKIPPED, R.RL_LIGHT_BACKFACING, R.RL_LIGHT_OCCLUDED, R.RL_LIGHT_VISIBLE) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    for k, name in enumerate(("RL_LIGHT_SKIPPED", "RL_LIGHT_BACKFACING", "RL_LIGHT_OCCLUDED", "RL_LIGHT_VISIBLE")):
        assert re.search(r"\b%s = %d\b" % (name, k), header), name
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    for name in ENTRY_POINTS + ("rl_scene_emitters",):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust), name
    for name in ("rl_debug_light_launches", "rl_debug_light_sample", "rl_debug_scene_emitters"):
        assert hasattr(_lib.lib, name) and name in _lib.DEBUG_SIGNATURES, name
    assert len(R.light_launches()) == 6 and _lib.lib.rl_debug_light_launches(None) == RL_E_INVALID
    assert "block 2^31 + s" in open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "rl_rng.h")).read()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_bad_arguments_are_invalid_in_the_documented_order_with_no_device(name):
    fn = getattr(_lib.lib, name)
    st, hits, sm = np.zeros(4, R.PATH_STATE_DTYPE), np.zeros(4, R.HIT_DTYPE), np.full(4 * 8, 0xAAAAAAAA, np.uint32)
    lst = np.arange(4, dtype=np.uint32)
    sp, hp, mp, lp = (a.ctypes.data_as(C.c_void_p) for a in (st, hits, sm, lst))
    fake = _FakeScene().ptr
    LDS = R.FETCH_LDS
    for scene in (None, fake):
        assert fn(scene, 7, 1, 0, sp, 4, lp, 4, hp, mp) == RL_E_INVALID and b"fetch" in _err()
        assert fn(scene, -1, 1, 0, None, 4, None, 5, None, None) == RL_E_INVALID and b"fetch" in _err()
        for args in ((None, 4, lp, 4, hp, mp), (sp, 4, lp, 4, None, mp), (sp, 4, lp, 4, hp, None), (None, 0, lp, 1, None, None)):
            assert fn(scene, LDS, 1, 0, *args) == RL_E_INVALID and b"buffer" in _err(), args
    assert fn(None, LDS, 1, 0, sp, 4, lp, 4, hp, mp) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, LDS, 1, 0, None, 0, None, 0, None, None) == RL_E_INVALID and b"scene" in _err()
    assert fn(fake, LDS, 1, 0, sp, 4, None, 5, hp, mp) == RL_E_INVALID and b"identity list" in _err()
    # the documented order: fetch, buffers, scene, identity list
    assert fn(None, 7, 1, 0, None, 4, None, 5, None, None) == RL_E_INVALID and b"fetch" in _err()
    assert fn(None, LDS, 1, 0, None, 4, None, 5, hp, mp) == RL_E_INVALID and b"buffer" in _err()
    assert fn(None, LDS, 1, 0, sp, 4, None, 5, hp, mp) == RL_E_INVALID and b"scene" in _err()
    # an empty list does nothing, whatever else is given
    for args in ((sp, 4, lp, 0, hp, mp), (None, 0, None, 0, None, None), (sp, 0, None, 0, None, mp)):
        for fetch in (LDS, R.FETCH_GLOBAL):
            assert fn(fake, fetch, 1, 0, *args) == 0, args
    assert (sm == 0xAAAAAAAA).all() and st.tobytes() == bytes(st.nbytes) and hits.tobytes() == bytes(hits.nbytes) and (lst == np.arange(4)).all()


def test_emitters_of_a_description():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    want = [i for i, o in enumerate(objs) if o["material_kind"] == 0 and o["surface_kind"] in (0, 2)]   # black body on a sphere or a circle
    assert len(want) == 3 and [int(objs["surface_kind"][i]) for i in want] == [0, 2, 2]                  # the sun and the two sky discs
    assert R.description_emitters(objs).tolist() == want == LO.emitters(objs.view(O.OBJECT_DTYPE)).tolist()
    # the capacity protocol
    n, out = C.c_uint32(77), np.full(4, 0xAAAAAAAA, np.uint32)
    op = objs.ctypes.data_as(C.c_void_p)
    fn = _lib.lib.rl_debug_scene_emitters
    assert fn(op, len(objs), out.ctypes.data_as(C.c_void_p), 2, C.byref(n)) == RL_E_INVALID and n.value == 3 and b"too small" in _err()
    assert fn(op, len(objs), None, 0, C.byref(n)) == RL_E_INVALID and n.value == 3 and (out == 0xAAAAAAAA).all()
    assert fn(op, len(objs), out.ctypes.data_as(C.c_void_p), 3, C.byref(n)) == 0 and out[:3].tolist() == want and out[3] == 0xAAAAAAAA
    assert fn(op, len(objs), out.ctypes.data_as(C.c_void_p), 3, None) == RL_E_INVALID
    assert _lib.lib.rl_scene_emitters(None, None, 0, C.byref(n)) == RL_E_INVALID and b"scene" in _err()
    # what is not sampleable: a plane, a paraboloid, radii that are zero, negative or not finite, a disc whose normal is not a unit vector
    odd = np.zeros(9, R.OBJECT_DTYPE)
    odd["v0"] = (0, 0, 1)
    odd["m"] = (5000.0, 1.0, 0.0)
    odd["surface_kind"] = [1, 0, 0, 0, 0, 2, 2, 3, 2]
    odd["f"][:, 0] = [0, 0.0, -1.0, np.inf, np.nan, 2.0, 2.0, 2.0, 0.0]
    odd["v0"][5] = (0, 0, 1.001)
    odd["v0"][6] = (0, 0, np.float32(1 + 2.0 ** -22))
    assert R.description_emitters(odd).tolist() == [6] == LO.emitters(odd.view(O.OBJECT_DTYPE)).tolist()
    odd["material_kind"] = 1
    assert R.description_emitters(odd).tolist() == []
    assert fn(odd.ctypes.data_as(C.c_void_p), 9, None, 0, C.byref(n)) == 0 and n.value == 0


def _camera_rays(objs, cam, n, seed, stream, first):
    import _mirror as M
    ms = M.Scene(objs, cam)
    dump = M.lib().mirror_dump_rays
    dump.restype = C.c_uint64
    dump.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    rays6 = np.zeros((n, 6), np.float32)
    for i in range(n):
        assert dump(ms.h, W, H, seed, stream, first + i, 1, rays6[i].ctypes.data, 1) == 1
    rays = np.zeros(n, R.SPECTRAL_RAY_DTYPE)
    rays["origin"], rays["direction"] = rays6[:, :3], rays6[:, 3:]
    rays["wavelength"] = np.random.default_rng(seed).uniform(380.0, 780.0, n).astype(np.float32)
    return rays


# path indices whose block 0x80000001 under (seed 11, stream 2) has all-zero / all-one top 24 bits in word 0: u = 0 and u = 1
EDGE_SEED, EDGE_STREAM = 11, 2


def _edge_paths():
    """Searches the first 2^25 path indices for u = 0 and u = 1 at segments = 1 (each has probability 2^-24 per index)."""
    found = {}
    step = 1 << 21
    w = np.zeros((step, 4), np.uint32)
    blocks = np.full(step, 0x80000001, np.uint32)
    for lo in range(0, 1 << 27, step):
        paths = np.arange(lo, lo + step, dtype=np.uint64)
        O.lib().oracle_rng_blocks(EDGE_SEED, EDGE_STREAM, O.ptr(paths), O.ptr(blocks), O.ptr(w), step)
        top = w[:, 0] >> 8
        for want in (0, 0xffffff):
            hit = np.flatnonzero(top == want)
            if len(hit) and want not in found:
                found[want] = int(paths[hit[0]])
        if len(found) == 2:
            break
    return found


@pytest.mark.parametrize("name", ["demo", "random"])
def test_host_compile_of_the_sampling_function_is_the_oracle_bit_for_bit(name):
    rng = np.random.default_rng(len(name))
    if name == "demo":
        objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    else:
        objs, cam = RS.random_scene(3, n_spheres=150, n_prisms=4, n_circles=4)
        objs = _with_lights(objs.view(R.OBJECT_DTYPE), rng)
    objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)
    seed, stream, first, n = EDGE_SEED, EDGE_STREAM, 4000, 1200
    so = S.StepOracle(objs, cam)
    states = S.begin(_camera_rays(objs.view(O.OBJECT_DTYPE), cam, n, seed, stream, first), first)
    hits = np.zeros(n, S.HIT_DTYPE)
    all_states, all_hits = [], []
    for step in range(3):
        so.step(states, seed, stream, hits=hits)
        all_states.append(states.copy())
        all_hits.append(hits.copy())
    st, ht = np.concatenate(all_states), np.concatenate(all_hits)
    # vertices a camera path of this scene may not reach: anywhere among the objects, facing anywhere, on every diffuse object
    m = 1500
    diffuse = np.flatnonzero((objs["material_kind"] == 1) | (objs["material_kind"] == 2))
    f_st, f_ht = np.zeros(m, S.STATE_DTYPE), np.zeros(m, S.HIT_DTYPE)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    f_ht["position"], f_ht["normal"], f_ht["object"] = rng.normal(0, 15, (m, 3)), unit(rng.normal(size=(m, 3))), rng.choice(diffuse, m)
    f_st["direction"], f_st["wavelength"], f_st["intensity"] = unit(rng.normal(size=(m, 3))), rng.uniform(380, 780, m), rng.uniform(0.05, 1, m)
    f_st["segments"], f_st["path_index"] = rng.integers(1, 9, m), rng.integers(0, 1 << 62, m, dtype=np.uint64)
    f_st["end"] = np.where(rng.random(m) < 0.5, S.LIVE, 2)
    st, ht = np.concatenate([st, f_st]), np.concatenate([ht, f_ht])
    # a vertex lying on the emitter: the hit moved onto the point the sample will draw (d2 == 0), and one next to it
    base, _ = LO.draw(objs, st, ht, seed, stream)
    some = np.flatnonzero(base["status"] != LO.SKIPPED)[-40:]
    assert len(some) == 40
    on = ht[some].copy()
    on["position"] = (ht["position"][some] + base["direction"][some] * base["distance"][some][:, None]).astype(np.float32)
    st, ht = np.concatenate([st, st[some]]), np.concatenate([ht, on])
    # u = 0 and u = 1: states whose path index draws them, at every sampled vertex kind
    edges = _edge_paths()
    assert sorted(edges) == [0, 0xffffff], edges
    for path in edges.values():
        e_st, e_ht = st[some].copy(), ht[some].copy()
        e_st["path_index"], e_st["segments"] = path, 1
        st, ht = np.concatenate([st, e_st]), np.concatenate([ht, e_ht])
    # hit records a step never writes: a miss, an object out of range, NaN positions and normals
    w_st, w_ht = st[some].copy(), ht[some].copy()
    w_ht["object"][:10] = 0xffffffff
    w_ht["object"][10:20] = len(objs)
    w_ht["position"][20:30] = np.nan
    w_ht["normal"][30:40] = (np.inf, 0, 0)
    st, ht = np.concatenate([st, w_st]), np.concatenate([ht, w_ht])
    # path indices over all 64 bits (neighbours that share one word and differ in the other, words that are float NaN, -0 and
    # infinity patterns) and `segments` at the edges of 32 bits: the block is (2^31 + segments) mod 2^32 (tests/_rng_width.py)
    mixed = RW.mixed_path_indices(320)
    p_st, p_ht = st[some][np.arange(320) % 40].copy(), ht[some][np.arange(320) % 40].copy()
    p_st["path_index"] = mixed
    edges = np.array([s for s in RW.SEGMENT_EDGES if s >= 1], np.uint32)
    s_st, s_ht = st[some][np.arange(8 * len(edges)) % 40].copy(), ht[some][np.arange(8 * len(edges)) % 40].copy()
    s_st["segments"] = edges[np.arange(len(s_st)) % len(edges)]
    b_st, b_ht = p_st.copy(), p_ht.copy()
    b_st["segments"] = edges[np.arange(len(b_st)) % len(edges)]
    assert set(RW.SPECIAL_PATHS) <= set(mixed.tolist()) and (mixed >> np.uint64(32) != 0).mean() > 0.9
    st, ht = np.concatenate([st, p_st, s_st, b_st]), np.concatenate([ht, p_ht, s_ht, b_ht])
    assert len(st) > 5700

    want, want_rays = LO.draw(objs, st, ht, seed, stream)
    got, got_rays = R.light_sample_host(objs, st.view(R.PATH_STATE_DTYPE), ht.view(R.HIT_DTYPE), seed, stream)
    bad = [i for i in range(len(st)) if got[i].tobytes() != want[i].tobytes() or got_rays[i].tobytes() != want_rays[i].tobytes()]
    assert not bad, (name, len(bad), bad[:5], got[bad[0]], want[bad[0]], got_rays[bad[0]], want_rays[bad[0]])
    # the classes are not vacuous, and the edge cases are what they claim to be
    status = want["status"]
    for s in (LO.SKIPPED, LO.BACKFACING, LO.VISIBLE):
        assert (status == s).sum() >= 40, (name, s, np.bincount(status, minlength=4))
    zero_d = (status == LO.BACKFACING) & (want["distance"] == 0)
    assert zero_d.any() and (want["direction"][zero_d] == 0).all()
    em = LO.emitters(objs.view(O.OBJECT_DTYPE))
    kinds = set(int(objs["surface_kind"][e]) for e in np.unique(want["emitter"][status != LO.SKIPPED]))
    assert kinds == {0, 2}, kinds
    assert set(np.unique(want["emitter"][status != LO.SKIPPED]).tolist()) <= set(em.tolist())
    if name == "random":
        steep = [int(e) for e in em if objs["surface_kind"][e] == 2 and abs(objs["v0"][e][2]) > 0.9999]
        assert len(steep) >= 2 and all((want["emitter"][status == LO.VISIBLE] == e).any() for e in steep), steep
    skipped = want[status == LO.SKIPPED]
    assert (skipped["emitter"] == 0xffffffff).all() and not skipped["direction"].any() and not skipped["weight"].any()
    assert np.isfinite(want["weight"]).all() and (want["weight"][status == LO.VISIBLE] >= 0).all()


def test_nearest_hit_occlusion_is_the_linear_scan():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    objs = objs.view(O.OBJECT_DTYPE)
    seed, stream, first, n = 5, 1, 0, 150
    so = S.StepOracle(objs, cam)
    states, hits = S.begin(_camera_rays(objs, cam, n, seed, stream, first), first), np.zeros(n, S.HIT_DTYPE)
    so.step(states, seed, stream, hits=hits)
    so.step(states, seed, stream, hits=hits)
    _, rays = LO.draw(objs, states, hits, seed, stream)
    rays = rays[rays["t_max"] > 0]
    occ = LO.Occluder(objs, cam)
    fast = occ.occluded(rays)
    assert fast.tolist() == occ.occluded_linear(rays).tolist() and 0 < fast.sum() < len(rays)


@pytest.mark.parametrize("occluder", [True, False])
def test_the_sample_estimates_what_the_next_segment_finds_on_the_cpu_oracle(occluder):
    """The mean of `value` over states at one vertex against the mean of what those states carry after one more segment that ends
    on one of the two lights: both estimate the light the vertex reflects towards the path.  On the oracle alone."""
    objs, cam = closed_scene(occluder)
    n, seed, stream = 1 << 13, 17, 3
    st, ht = vertex_states(n)
    occ = LO.Occluder(objs, cam)
    light = LO.light_paths(occ, st, ht, seed, stream)
    assert set(np.unique(light["status"])) >= ({LO.BACKFACING, LO.VISIBLE} | ({LO.OCCLUDED} if occluder else set()))
    # the path's own next segment: the diffuse bounce, then Scene::intersect, counting ends on the lights
    d = bounce_directions(st, seed, stream)
    o = (ht["position"] + d * np.float32(1e-5)).astype(np.float32)
    value = np.zeros(n)
    isect = np.zeros(10, np.float32)
    L = O.lib()
    lights = set(LO.emitters(objs.view(O.OBJECT_DTYPE)).tolist())
    assert lights == {1, 2}
    for i in range(n):
        idx = L.oracle_scene_intersect(occ.scene.h, O.ptr(o[i]), O.ptr(d[i]), O.ptr(isect))
        if idx in lights:
            value[i] = st["intensity"][i] * L.oracle_black_body(float(objs["m"][idx][0]), float(objs["m"][idx][1]), float(st["wavelength"][i]), None)
    assert_means_agree(light["value"], value, "occluder %s" % occluder)


def test_light_kernels_compile_without_scratch_and_within_the_register_bound(kernels):
    light = {n: k for n, k in kernels.items() if "rl_light_kernel" in n}
    assert sorted(variant_of_name(n, "rl_light_kernel") for n in light) == [(s, c) for s in "012" for c in "01"]
    steps = {variant_of_name(n, "rl_step_kernel"): k for n, k in kernels.items() if "rl_step_kernel" in n}
    for name, k in light.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)
        v = variant_of_name(name, "rl_light_kernel")
        assert k["sgpr_spill_count"] <= steps[v]["sgpr_spill_count"], (name, k["sgpr_spill_count"], steps[v]["sgpr_spill_count"])
        if v[0] == "2":
            assert k["sgpr_spill_count"] == 0, (name, k)
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_light.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
