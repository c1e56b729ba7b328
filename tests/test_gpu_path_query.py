"""Scene.camera_rays / Scene.render_rays on the device (rl_scene_camera_rays*, rl_scene_render_rays*), bit for bit: camera rays fed
back reproduce the oracle's render and the device's own rl_trace_unit_render (photon values, x, y, wavelength, segment counts);
rays no camera makes -- uniform, bounce-like, non-unit, tangent, degenerate, with odd and non-finite wavelengths -- match the
Python restatement of render_ray (tests/_path_oracle.py) in every field of RlPathResult; plus the segment limit, batch splits,
the host and device paths, every path-kernel variant, concurrent callers and a call made while a render is open."""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import _boundary as B
import _oracle as O
import _path_oracle as P
import _query_rays as QR
from _boundary import _ocam
from _cases import _wavelengths, ray_sets
from _compare import assert_consistent, assert_same
from _scenes import _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE = R.RL_OBJECT_NONE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
# scene -> the least share of paths that must carry a value: about half the share the oracle's render gives (~10 % on the built-in
# scene), so that a kernel which zeroed most emitter hits would fail here even before the bit-for-bit comparison
IDENTITY_SCENES = {"demo": 0.05, "glass": 0.05, "random-seed-1": 0.3, "random-seed-2": 0.4, "many-prisms": 0.4, "demo-2500": 0.05,
                   "random-6000": 0.1}


@pytest.mark.parametrize("name", sorted(IDENTITY_SCENES))
def test_camera_rays_fed_back_reproduce_the_renderer(name):
    objs, cam = _scene(name)
    scene, oscene = R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    big = len(objs) > 2000
    n, seed, stream, first = (8192 if big else 65536), 3 + len(name), 1, 1000
    want, segs = oscene.render(W, H, seed, stream, first, n, threads=16)
    cyl = int((objs["surface_kind"] == 4).sum() >= 40)
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    assert samples["x"].tobytes() == want["x"].tobytes() and samples["y"].tobytes() == want["y"].tobytes()
    assert samples["ray"]["wavelength"].tobytes() == want["wavelength"].tobytes()
    assert (samples["ray"]["reserved"] == 0).all() and (samples["reserved0"] == 0).all() and (samples["reserved1"] == 0).all()
    for fetch in FETCHES:
        before = R.path_launches()
        res = scene.render_spectral_rays(samples["ray"], seed, stream, first, fetch=fetch)
        v = B._variant_of(R.path_launches, before)
        assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (name, fetch, v)
        assert res["value"].tobytes() == want["probability"].tobytes(), (name, fetch)
        assert int(res["segments"].sum(dtype=np.uint64)) == segs, (name, fetch)
        assert_consistent(res)
        share = float((res["value"] != 0).mean())
        assert share >= IDENTITY_SCENES[name], (name, share)
    if name == "demo":   # ... and the device's own renderer gives the same bytes for those paths
        t = R.TraceUnit(0, W, H, n_photons=n)
        t.render(scene, seed, stream, first)
        got = t.mapped_photons
        assert got["probability"].tobytes() == res["value"].tobytes() and t.stats()[:2] == (n, segs)


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_path_oracle_on_device_camera_rays(name):
    """The Python restatement, fed the device's camera rays, reproduces the oracle's render: its yardstick is the reference's."""
    objs, cam = _scene(name)
    oscene = O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    n, seed, stream, first = 2048, 21, 3, 77
    want, segs = oscene.render(W, H, seed, stream, first, n, threads=16)
    samples = R.Scene(objs, cam).camera_rays(W, H, seed, stream, first, n)
    r = samples["ray"]
    got = P.PathOracle(objs, cam).render_rays(r["origin"], r["direction"], r["wavelength"], seed, stream, first)
    assert got["value"].tobytes() == want["probability"].tobytes()
    assert int(got["segments"].sum()) == segs


@pytest.mark.parametrize("name", ["demo", "glass", "random-seed-1"])
def test_arbitrary_rays_match_the_path_oracle(name):
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    po = P.PathOracle(objs, cam)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    sets = ray_sets(scene, objs, cam, rng, 1024)
    seed, stream = 5, 2
    for kind, (o, d) in sets.items():
        wl = _wavelengths(rng, len(o))
        first = int(rng.integers(0, 1 << 40))
        want = po.render_rays(o, d, wl, seed, stream, first).view(R.PATH_RESULT_DTYPE)
        invalid = ~np.isfinite(wl)
        assert (want["end"][invalid] == R.RL_PATH_END_INVALID).all() and (want["segments"][invalid] == 0).all()
        assert (want["end"][~invalid] != R.RL_PATH_END_INVALID).all()
        for fetch in FETCHES:
            got = scene.render_rays(o, d, wl, seed, stream, first, fetch=fetch)
            assert_same(got, want, "%s %s fetch %d" % (name, kind, fetch))


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_segment_limit(name):
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    po = P.PathOracle(objs, cam)
    n, seed, stream, first = 2048, 8, 0, 0
    r = scene.camera_rays(W, H, seed, stream, first, n)["ray"]
    for ms in (1, 2, 3, 7):
        want = po.render_rays(r["origin"], r["direction"], r["wavelength"], seed, stream, first, max_segments=ms).view(R.PATH_RESULT_DTYPE)
        got = scene.render_spectral_rays(r, seed, stream, first, max_segments=ms)
        assert_same(got, want, "%s max_segments %d" % (name, ms))
        assert (got["end"] == R.RL_PATH_END_LIMIT).any() and (got["segments"] <= ms).all()
        assert (got["value"][got["end"] == R.RL_PATH_END_LIMIT] == 0).all()
    r = scene.camera_rays(W, H, seed, stream, first, 1 << 16)["ray"]
    default = scene.render_spectral_rays(r, seed, stream, first, max_segments=0)
    assert default.tobytes() == scene.render_spectral_rays(r, seed, stream, first, max_segments=65536).tobytes()
    assert (default["end"] != R.RL_PATH_END_LIMIT).all()


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return objs, cam, R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))


def test_split_batches_give_the_same_bytes(demo):
    objs, cam, scene, oscene = demo
    n, seed, stream, first = 50000, 4, 1, 123
    r = scene.camera_rays(W, H, seed, stream, first, n)["ray"]
    whole = scene.render_spectral_rays(r, seed, stream, first)
    for k in (1, 64, 12345, 49999):
        a = scene.render_spectral_rays(r[:k], seed, stream, first)
        b = scene.render_spectral_rays(r[k:], seed, stream, first + k)
        assert np.concatenate([a, b]).tobytes() == whole.tobytes(), k
        ca = scene.camera_rays(W, H, seed, stream, first, k)
        cb = scene.camera_rays(W, H, seed, stream, first + k, n - k)
        assert np.concatenate([ca["ray"], cb["ray"]]).tobytes() == r.tobytes(), k


def _device_paths(scene, rays, seed, stream, first, fetch):
    db, rb = QR.DeviceBuffer(rays.nbytes), QR.DeviceBuffer(len(rays) * 16)
    db.upload(rays)
    res = np.zeros(len(rays), dtype=R.PATH_RESULT_DTYPE)
    res["end"] = 12345   # poison: every record must be written
    rb.upload(res)
    scene.render_rays_device(db, rb, seed, stream, first, fetch=fetch)
    rb.download(res)
    return res


def _device_camera(scene, n, seed, stream, first):
    sb = QR.DeviceBuffer(n * 48)
    samples = np.zeros(n, dtype=R.CAMERA_SAMPLE_DTYPE)
    samples["x"] = 12345.0
    sb.upload(samples)
    scene.camera_rays_device(W, H, seed, stream, first, sb)
    sb.download(samples)
    return samples


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, (1 << 20) + 4097])
def test_batch_sizes_host_and_device_paths_agree(demo, n):
    """Host path (staged in chunks of 2^20 records: the last size spans two) and device path give the same bytes; a subsample of
    the large batch and every path of the small ones equal the oracle's render."""
    objs, cam, scene, oscene = demo
    seed, stream, first = 9, 0, 5
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    assert _device_camera(scene, n, seed, stream, first).tobytes() == samples.tobytes()
    r = samples["ray"]
    pick = np.random.default_rng(n).choice(n, min(n, 2048), replace=False) if n else np.zeros(0, np.int64)
    want = np.zeros(len(pick), dtype=O.PHOTON_DTYPE)
    for j, i in enumerate(pick):
        want[j:j + 1] = oscene.render(W, H, seed, stream, first + int(i), 1)[0]
    for fetch in FETCHES:
        host = scene.render_spectral_rays(r, seed, stream, first, fetch=fetch)
        assert len(host) == n
        assert_same(_device_paths(scene, np.ascontiguousarray(r), seed, stream, first, fetch), host, "device vs host, n=%d" % n)
        assert host["value"][pick].tobytes() == want["probability"].tobytes(), (n, fetch)
    assert R.lib.rl_scene_render_rays_device(scene.handle, 0, 1, 0, 0, 0, None, 0, None) == 0
    assert R.lib.rl_scene_camera_rays_device(scene.handle, W, H, 1, 0, 0, 0, None) == 0


def test_device_paths_refuse_host_memory(demo):
    objs, cam, scene, oscene = demo
    rays, res = np.zeros(64, R.SPECTRAL_RAY_DTYPE), np.zeros(64, R.PATH_RESULT_DTYPE)
    rc = R.lib.rl_scene_render_rays_device(scene.handle, 0, 1, 0, 0, 0, rays.ctypes.data_as(C.c_void_p), 64, res.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"device memory" in R.lib.rl_last_error()
    s = np.zeros(64, R.CAMERA_SAMPLE_DTYPE)
    rc = R.lib.rl_scene_camera_rays_device(scene.handle, W, H, 1, 0, 0, 64, s.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b"device memory" in R.lib.rl_last_error()


def test_every_path_variant_ran():
    """Whole scene, tables only and nothing staged, each with and without the prisms' second bound; fills in what the other tests
    left out, and each call runs exactly one variant.  Asserts on its own launches only."""
    ran = set()
    for name in ("demo", "many-prisms", "demo-2500", "tables-prisms"):
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        r = scene.camera_rays(W, H, 1, 0, 0, 256)["ray"]
        for fetch in FETCHES:
            before = R.path_launches()
            scene.render_spectral_rays(r, 1, 0, 0, fetch=fetch)
            ran.add(B._variant_of(R.path_launches, before))
    assert ran == set(range(6)), sorted(ran)


def test_four_threads_render_rays_on_one_scene(demo):
    objs, cam, scene, oscene = demo
    jobs = []
    for k in range(4):
        n, first = 3000 + 1000 * k, 10000 * k
        want, _ = oscene.render(W, H, 6, k, first, n, threads=4)
        jobs.append((k, first, scene.camera_rays(W, H, 6, k, first, n)["ray"], want))
    errors, barrier = [], threading.Barrier(4)

    def worker(k, first, r, want):
        try:
            barrier.wait()
            for rep in range(10):
                fetch = FETCHES[(k + rep) % 2]
                got = scene.render_spectral_rays(r, 6, k, first, fetch=fetch) if rep % 2 else \
                    _device_paths(scene, np.ascontiguousarray(r), 6, k, first, fetch)
                assert got["value"].tobytes() == want["probability"].tobytes(), (k, rep)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


def test_render_rays_between_render_begin_and_end(demo):
    objs, cam, scene, oscene = demo
    N = 1 << 16
    want_photons, segs = oscene.render(W, H, 5, 0, 0, N, threads=16)
    want, _ = oscene.render(W, H, 7, 1, 0, 8192, threads=16)
    r = scene.camera_rays(W, H, 7, 1, 0, 8192)["ray"]
    for fetch in FETCHES:
        t = R.TraceUnit(0, W, H, n_photons=N)
        R.check(R.lib.rl_trace_unit_render_begin(t.handle, scene.handle, 5, 0, 0))
        got = scene.render_spectral_rays(r, 7, 1, 0, fetch=fetch)
        R.check(R.lib.rl_trace_unit_render_end(t.handle))
        assert got["value"].tobytes() == want["probability"].tobytes(), fetch
        assert t.mapped_photons.tobytes() == want_photons.tobytes() and t.stats()[:2] == (N, segs)
