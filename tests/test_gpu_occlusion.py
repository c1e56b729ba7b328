"""Scene.occluded on the device (rl_scene_occluded / rl_scene_occluded_device) against its definition: one byte per ray, 1 where
Scene::intersect reports an object nearer than t_max.  Bit for bit against the CPU oracle over every scene, ray set and t_max case of
tests/test_gpu_query.py (tests/_scenes.py, tests/_cases.py) plus shadow rays and short rays (whose bound the kernel's scan starts from), both fetch modes and every
kernel variant; against rl_scene_intersect_device at scale; batch sizes with guard bytes behind the output; pageable memory refused;
concurrent callers; a call made while a render is open."""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import _boundary as B
import _occlusion_cases as OC
import _oracle as O
import _query_rays as QR
from _boundary import _ocam
from _cases import _ray_records, blocked, oracle_hits, ray_sets, t_max_cases
from _compare import assert_same_bytes
from _scenes import SCENES, _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE = R.RL_OBJECT_NONE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
BOTH_OUTCOMES = ("demo", "demo-2500", "random-6000")   # the shadow and short sets must hold >= 5 % of each answer there
_ran = set()   # occlusion variants seen by test_scene_occlusion_bit_exact (test_every_occlusion_variant_ran reads it)


def bounded_sets(objs, cam_o, cam_d, first_hits, rng, oscene=None):
    """{kind: (origins, directions, t_max)}: the shadow and the short set from the camera rays' first hits.  With the CPU oracle's
    scene, a quarter of the shadow rays aim at emitter points the oracle says they see."""
    oracle = None if oscene is None else (lambda o, d: oracle_hits(oscene, o, d))
    return {"shadow": OC.shadow_rays(objs, cam_d, first_hits, rng, oracle), "short": OC.short_rays(cam_d, first_hits, rng)}


@pytest.mark.parametrize("name", SCENES)
def test_scene_occlusion_bit_exact(name):
    objs, cam = _scene(name)
    scene, oscene = R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    big = len(objs) > 2000
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sets = ray_sets(scene, objs, cam, rng, 1024 if big else 4096)
    assert set(sets) >= {"camera", "bounce", "uniform", "non_unit", "degenerate"}, sorted(sets)   # (and "tangent" where a sphere has a radius)
    cyl = int((objs["surface_kind"] == 4).sum() >= 40)
    cam_o, cam_d = sets["camera"]
    cases = {}   # kind: (origins, directions, [t_max per case], [the oracle's answer per case])
    for kind, (o, d) in sets.items():
        want = oracle_hits(oscene, o, d)
        t_cases = [np.float32(np.inf), t_max_cases(want, rng)]
        cases[kind] = (o, d, t_cases, [blocked(want, t) for t in t_cases])
    for kind, (o, d, t) in bounded_sets(objs, cam_o, cam_d, oracle_hits(oscene, cam_o, cam_d), rng, oscene).items():
        answer = blocked(oracle_hits(oscene, o, d), t)
        if name in BOTH_OUTCOMES:   # (the oracle's answer alone: both classes are there whatever the GPU says)
            share = float(answer.mean())
            print("%s %s: %d rays, %.1f %% blocked" % (name, kind, len(answer), 100.0 * share))
            assert len(answer) >= 256 and 0.05 <= share <= 0.95, (name, kind, len(answer), share)
        cases[kind] = (o, d, [t], [answer])
    for kind, (o, d, t_cases, answers) in cases.items():
        for fetch in FETCHES:
            for t, answer in zip(t_cases, answers):
                before = R.occlusion_launches()
                got = scene.occluded(o, d, t, fetch=fetch)
                if len(o):
                    v = B._variant_of(R.occlusion_launches, before)
                    assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (name, fetch, v)
                    _ran.add(v)
                assert_same_bytes(got, answer, "%s %s fetch %d t_max %s" % (name, kind, fetch, "inf" if np.ndim(t) == 0 else "per ray"))


def test_every_occlusion_variant_ran():
    """Whole scene, tables only and nothing staged, each with and without the prisms' second bound, as the query kernel's test has
    it.  Fills in what the scene tests left out."""
    for name in ("demo", "many-prisms", "demo-2500", "tables-prisms"):
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        o, d = QR.camera_rays(cam, 1920, 1080, np.random.default_rng(1), 256)
        for fetch in FETCHES:
            before = R.occlusion_launches()
            scene.occluded(o, d, fetch=fetch)
            _ran.add(B._variant_of(R.occlusion_launches, before))
    assert _ran == set(range(6)), sorted(_ran)


GUARD = 64


def _device_occluded(scene, rays, fetch):
    """The device form into a buffer of n + 64 bytes of 0xAA: every byte of [0, n) is written with 0 or 1, the guard stays."""
    n = len(rays)
    db, ob = QR.DeviceBuffer(rays.nbytes), QR.DeviceBuffer(n + GUARD)
    db.upload(rays)
    out = np.full(n + GUARD, 0xAA, np.uint8)
    ob.upload(out)
    if n:
        scene.occluded_device(db, ob, fetch=fetch)
    else:
        assert R.lib.rl_scene_occluded_device(scene.handle, fetch, C.c_void_p(db.data_ptr()), 0, C.c_void_p(ob.data_ptr())) == 0
    ob.download(out)
    assert (out[n:] == 0xAA).all(), "bytes behind n_rays = %d were written: %r" % (n, out[n:])
    assert (out[:n] <= 1).all()
    return out[:n].copy()


def _device_objects(scene, rays, fetch):
    db, hb = QR.DeviceBuffer(rays.nbytes), QR.DeviceBuffer(len(rays) * 48)
    db.upload(rays)
    hits = np.zeros(len(rays), dtype=R.HIT_DTYPE)
    scene.intersect_device(db, hb, fetch=fetch)
    hb.download(hits)
    return hits


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return objs, cam, R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))


@pytest.mark.parametrize("name", ["demo", "random-20000"])
def test_device_against_device_at_scale(name):
    """2^22 camera, shadow and short rays: occluded_device equals intersect_device's object != NONE, byte for byte."""
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    n = 1 << 22
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    cam_o, cam_d = QR.camera_rays(cam, 1920, 1080, rng, n)
    first = _device_objects(scene, _ray_records(cam_o, cam_d), R.FETCH_LDS)
    assert (first["object"] != NONE).any()
    sets = {"camera": (cam_o, cam_d, np.float32(np.inf))}
    for kind, (o, d, t) in bounded_sets(objs, cam_o, cam_d, first, rng).items():
        pad = rng.integers(0, len(o), n - len(o))   # (misses dropped: filled up to 2^22 with repeats)
        sets[kind] = (np.concatenate([o, o[pad]]), np.concatenate([d, d[pad]]), np.concatenate([t, t[pad]]))
    for kind, (o, d, t) in sets.items():
        rays = _ray_records(o, d, t)
        assert len(rays) == n
        for fetch in FETCHES:
            want = (_device_objects(scene, rays, fetch)["object"] != NONE).astype(np.uint8)
            got = _device_occluded(scene, rays, fetch)
            print("%s %s fetch %d: %.1f %% blocked" % (name, kind, fetch, 100.0 * want.mean()))
            assert_same_bytes(got, want, "%s %s fetch %d, 2^22 rays" % (name, kind, fetch))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, (1 << 20) + 4097])
def test_batch_sizes_host_and_device_forms_agree(demo, n):
    """Host form (staged in chunks of 2^20 rays: the last size spans two) and device form give the same bytes, the 64 guard bytes
    behind the device output stay 0xAA, and a subsample equals the oracle.  Short rays for every other size, so both answers occur."""
    objs, cam, scene, oscene = demo
    rng = np.random.default_rng(n)
    o, d = QR.camera_rays(cam, 1920, 1080, rng, n)
    t = np.where(np.arange(n) % 2 == 0, np.float32(np.inf), np.float32(15.0)).astype(np.float32)
    for fetch in FETCHES:
        host = scene.occluded(o, d, t, fetch=fetch)
        assert host.dtype == np.uint8 and len(host) == n
        dev = _device_occluded(scene, _ray_records(o, d, t), fetch)
        assert_same_bytes(dev, host, "device vs host form, n=%d fetch %d" % (n, fetch))
        pick = rng.choice(n, min(n, 4096), replace=False) if n else np.zeros(0, np.int64)
        assert_same_bytes(host[pick], blocked(oracle_hits(oscene, o[pick], d[pick]), t[pick]), "n=%d fetch %d" % (n, fetch))
    assert R.lib.rl_scene_occluded_device(scene.handle, 0, None, 0, None) == 0
    assert R.lib.rl_scene_occluded(scene.handle, 0, None, 0, None) == 0


def test_device_form_refuses_host_memory(demo):
    objs, cam, scene, oscene = demo
    rays, out = np.zeros(64, R.RAY_DTYPE), np.full(64, 0xAA, np.uint8)
    rc = R.lib.rl_scene_occluded_device(scene.handle, 0, rays.ctypes.data_as(C.c_void_p), 64, out.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"device memory" in R.lib.rl_last_error()
    assert (out == 0xAA).all()


def test_four_threads_query_one_scene_concurrently(demo):
    objs, cam, scene, oscene = demo
    sets, wants = [], []
    for k in range(4):
        rng = np.random.default_rng(100 + k)
        o, d = QR.camera_rays(cam, 1920, 1080, rng, 3000 + 1000 * k)
        so, sd, st = OC.short_rays(d, oracle_hits(oscene, o, d), rng)
        sets.append((so, sd, st))
        wants.append(blocked(oracle_hits(oscene, so, sd), st))
    errors, barrier = [], threading.Barrier(4)

    def worker(k):
        try:
            barrier.wait()
            for rep in range(20):
                o, d, t = sets[k]
                got = scene.occluded(o, d, t, fetch=FETCHES[(k + rep) % 2]) if rep % 2 else _device_occluded(scene, _ray_records(o, d, t), FETCHES[k % 2])
                assert got.tobytes() == wants[k].tobytes(), (k, rep)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


def test_occlusion_between_render_begin_and_end(demo):
    """A call issued while a render is open on the device completes with the right bytes, and the render's photons are those of a
    render made alone."""
    objs, cam, scene, oscene = demo
    W, H, N = 320, 180, 1 << 16
    alone = R.TraceUnit(0, W, H, n_photons=N)
    alone.render(scene, seed=5, stream=0, first_path_index=0)
    want_photons, want_stats = alone.mapped_photons.tobytes(), alone.stats()[:2]
    rng = np.random.default_rng(9)
    o, d = QR.camera_rays(cam, 1920, 1080, rng, 8192)
    so, sd, st = OC.shadow_rays(objs, d, oracle_hits(oscene, o, d), rng)
    want = blocked(oracle_hits(oscene, so, sd), st)
    for fetch in FETCHES:
        t = R.TraceUnit(0, W, H, n_photons=N)
        R.check(R.lib.rl_trace_unit_render_begin(t.handle, scene.handle, 5, 0, 0))
        got = scene.occluded(so, sd, st, fetch=fetch)
        R.check(R.lib.rl_trace_unit_render_end(t.handle))
        assert_same_bytes(got, want, "occlusion during an open render, fetch %d" % fetch)
        assert t.mapped_photons.tobytes() == want_photons and t.stats()[:2] == want_stats
