"""Scene.intersect on the device (rl_scene_intersect / rl_scene_intersect_device) against the CPU oracle's Scene::intersect,
bit for bit: the object index and the raw bits of position, normal, tangent and distance of every ray, over the built-in, glass,
random, many-prism, degenerate and third-level scenes, camera-like, bounce-like, random, non-unit, tangent, degenerate and far rays,
every t_max case, both fetch modes, every query variant, the host and device paths, concurrent callers and a query made while a
render is open."""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import _boundary as B
import _oracle as O
import _query_rays as QR
from _boundary import _ocam
from _cases import _filter, _ray_records, oracle_hits, ray_sets, t_max_cases
from _compare import assert_same
from _scenes import SCENES, _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE = R.RL_OBJECT_NONE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
_ran = set()   # query variants seen by test_scene_queries_bit_exact (test_every_query_variant_ran reads it)


@pytest.mark.parametrize("name", SCENES)
def test_scene_queries_bit_exact(name):
    objs, cam = _scene(name)
    scene, oscene = R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    big = len(objs) > 2000
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sets = ray_sets(scene, objs, cam, rng, 1024 if big else 4096)
    cyl = int((objs["surface_kind"] == 4).sum() >= 40)
    for kind, (o, d) in sets.items():
        want = oracle_hits(oscene, o, d)
        if kind == "camera":
            assert (want["object"] != NONE).any(), name   # (the camera looks at something)
        t_max = t_max_cases(want, rng)
        want_t = _filter(want, t_max)
        for fetch in FETCHES:
            before = R.query_launches()
            got = scene.intersect(o, d, fetch=fetch)
            v = B._variant_of(R.query_launches, before)
            assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (name, fetch, v)
            _ran.add(v)
            assert_same(got, want, "%s %s fetch %d t_max inf" % (name, kind, fetch))
            assert_same(scene.intersect(o, d, t_max, fetch=fetch), want_t, "%s %s fetch %d t_max cases" % (name, kind, fetch))


def test_every_query_variant_ran():
    """Whole scene, tables only and nothing staged, each with and without the prisms' second bound (the third cull level rides
    in the tables-only and nothing-staged variants: demo-2500, random-6000 / 20000).  Fills in what the scene tests left out."""
    for name in ("demo", "many-prisms", "demo-2500", "tables-prisms"):
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        o, d = QR.camera_rays(cam, 1920, 1080, np.random.default_rng(1), 256)
        for fetch in FETCHES:
            before = R.query_launches()
            scene.intersect(o, d, fetch=fetch)
            _ran.add(B._variant_of(R.query_launches, before))
    assert _ran == set(range(6)), sorted(_ran)


def _device_query(scene, rays, fetch):
    db, hb = QR.DeviceBuffer(rays.nbytes), QR.DeviceBuffer(len(rays) * 48)
    db.upload(rays)
    hits = np.zeros(len(rays), dtype=R.HIT_DTYPE)
    hits["object"] = 12345   # poison: every record must be written
    hb.upload(hits)
    scene.intersect_device(db, hb, fetch=fetch)
    hb.download(hits)
    return hits


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return objs, cam, R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, (1 << 20) + 4097])
def test_batch_sizes_host_and_device_paths_agree(demo, n):
    """Host path (staged through device buffers in chunks of 2^20 rays: the last size spans two) and device path give the same
    bytes; a random subsample of the large batch and every ray of the small ones equal the oracle."""
    objs, cam, scene, oscene = demo
    rng = np.random.default_rng(n)
    o, d = QR.camera_rays(cam, 1920, 1080, rng, n)
    for fetch in FETCHES:
        host = scene.intersect(o, d, fetch=fetch)
        assert len(host) == n
        dev = _device_query(scene, _ray_records(o, d), fetch)
        assert_same(dev, host, "device vs host path, n=%d fetch %d" % (n, fetch))
        pick = rng.choice(n, min(n, 4096), replace=False) if n else np.zeros(0, np.int64)
        assert_same(host[pick], oracle_hits(oscene, o[pick], d[pick]), "n=%d fetch %d" % (n, fetch))
    assert R.lib.rl_scene_intersect_device(scene.handle, 0, None, 0, None) == 0


def test_device_path_refuses_host_memory(demo):
    objs, cam, scene, oscene = demo
    rays, hits = np.zeros(64, R.RAY_DTYPE), np.zeros(64, R.HIT_DTYPE)
    rc = R.lib.rl_scene_intersect_device(scene.handle, 0, rays.ctypes.data_as(C.c_void_p), 64, hits.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"device memory" in R.lib.rl_last_error()


def test_four_threads_query_one_scene_concurrently(demo):
    objs, cam, scene, oscene = demo
    sets = [QR.camera_rays(cam, 1920, 1080, np.random.default_rng(100 + k), 3000 + 1000 * k) for k in range(4)]
    wants = [oracle_hits(oscene, o, d) for o, d in sets]
    errors, barrier = [], threading.Barrier(4)

    def worker(k):
        try:
            barrier.wait()
            for rep in range(20):
                o, d = sets[k]
                got = scene.intersect(o, d, fetch=FETCHES[(k + rep) % 2]) if rep % 2 else _device_query(scene, _ray_records(o, d), FETCHES[k % 2])
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


def test_query_between_render_begin_and_end(demo):
    """A query issued while a render is open on the device (rl_trace_unit_render_begin ... _end) returns correct hits -- it waits
    for the open launch to drain, which that launch does by itself once its calls are complete (include/robigo_luculenta.h) -- and
    the render's photons still equal the oracle's."""
    objs, cam, scene, oscene = demo
    W, H, N = 320, 180, 1 << 16
    want_photons, segs = oscene.render(W, H, 5, 0, 0, N, threads=8)
    o, d = QR.camera_rays(cam, 1920, 1080, np.random.default_rng(9), 8192)
    want = oracle_hits(oscene, o, d)
    for fetch in FETCHES:
        t = R.TraceUnit(0, W, H, n_photons=N)
        R.check(R.lib.rl_trace_unit_render_begin(t.handle, scene.handle, 5, 0, 0))
        got = scene.intersect(o, d, fetch=fetch)
        R.check(R.lib.rl_trace_unit_render_end(t.handle))
        assert_same(got, want, "query during an open render, fetch %d" % fetch)
        assert t.mapped_photons.tobytes() == want_photons.tobytes() and t.stats()[:2] == (N, segs)
