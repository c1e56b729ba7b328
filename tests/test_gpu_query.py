"""Scene.intersect on the device (rl_scene_intersect / rl_scene_intersect_device) against the CPU oracle's Scene::intersect,
bit for bit: the object index and the raw bits of position, normal, tangent and distance of every ray, over the built-in, glass,
random, many-prism, degenerate and third-level scenes, camera-like, bounce-like, random, non-unit, tangent and degenerate rays,
every t_max case, both fetch modes, every query variant, the host and device paths, concurrent callers and a query made while a
render is open."""
import ctypes as C
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _boundary as B
import _oracle as O
import _query_rays as QR
import _random_scene as RS
from _boundary import _ocam

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE = R.RL_OBJECT_NONE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)


def oracle_hits(oscene, origins, directions, t_max=None):
    """HIT_DTYPE records of the oracle's Scene::intersect for every ray (per-ray calls on a thread pool: ctypes releases the
    GIL), restricted to distance < t_max when t_max is given."""
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(directions, dtype=np.float32)
    n = len(o)
    out10 = np.zeros((n, 10), dtype=np.float32)
    idx = np.zeros(n, dtype=np.int64)
    fn, h = O.lib().oracle_scene_intersect, oscene.h
    po, pd, pv = o.ctypes.data, d.ctypes.data, out10.ctypes.data

    def work(lo, hi):
        for i in range(lo, hi):
            idx[i] = fn(h, po + 12 * i, pd + 12 * i, pv + 40 * i)

    step = max(1, (n + 63) // 64)
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(lambda lo: work(lo, min(n, lo + step)), range(0, n, step)))
    hits = np.zeros(n, dtype=R.HIT_DTYPE)
    hit = idx >= 0
    if t_max is not None:
        hit &= out10[:, 9] < np.broadcast_to(np.asarray(t_max, np.float32), (n,))
    hits["object"] = np.where(hit, idx, NONE).astype(np.uint32)
    hits["position"][hit], hits["normal"][hit], hits["tangent"][hit] = out10[hit, 0:3], out10[hit, 3:6], out10[hit, 6:9]
    hits["distance"][hit] = out10[hit, 9]
    return hits


def assert_same(got, want, what):
    if got.tobytes() != want.tobytes():
        rows = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: %d of %d rays differ, first %d: got %r want %r" % (what, len(rows), len(got), rows[0], got[rows[0]],
                                                                                       want[rows[0]]))


def t_max_cases(want, rng):
    """Per ray: +inf, random in (0, 2 distance), exactly the distance (a miss), nextafter(distance, inf) (a hit), 0, -1, NaN."""
    n = len(want)
    dist = np.where(want["object"] != NONE, want["distance"], np.float32(50.0)).astype(np.float32)
    case = np.arange(n) % 7
    t = np.full(n, np.inf, dtype=np.float32)
    t[case == 1] = (dist * rng.uniform(0, 2, n).astype(np.float32))[case == 1]
    t[case == 2] = dist[case == 2]
    t[case == 3] = np.nextafter(dist, np.float32(np.inf))[case == 3]
    t[case == 4], t[case == 5], t[case == 6] = 0.0, -1.0, np.nan
    return t


def ray_sets(scene, objs, cam, rng, n):
    """{kind: (origins, directions)}: camera-like, bounce-like (from the camera rays' hits), uniform origins within 4x the scene's
    bounding radius, non-unit directions (|d| in [0.25, 4]), rays tangent to spheres and degenerate rays."""
    sets = {}
    o, d = QR.camera_rays(cam, 1920, 1080, rng, n)
    sets["camera"] = (o, d)
    sets["bounce"] = QR.bounce_rays(o, d, scene.intersect(o, d), rng)
    centres = np.concatenate([objs["v0"][objs["surface_kind"] == 0], objs["v1"][objs["surface_kind"] != 0]])
    finite = np.isfinite(centres).all(axis=1) & (np.abs(centres).max(axis=1) < 1e4)
    radius = float(np.linalg.norm(centres[finite], axis=1).max()) if finite.any() else 10.0
    u = QR.uniform_directions(rng, n)
    sets["uniform"] = ((u * (4.0 * radius * rng.random((n, 1)) ** (1 / 3))).astype(np.float32), QR.uniform_directions(rng, n))
    o2 = (rng.normal(0, radius, (n, 3))).astype(np.float32)
    sets["non_unit"] = (o2, (QR.uniform_directions(rng, n) * rng.uniform(0.25, 4.0, (n, 1))).astype(np.float32))
    sph = objs[(objs["surface_kind"] == 0) & np.isfinite(objs["f"][:, 0]) & (objs["f"][:, 0] > 0)]
    if len(sph):
        k = rng.integers(0, len(sph), n // 4)
        c, r = sph["v0"][k].astype(np.float64), sph["f"][k, 0].astype(np.float64)
        a = QR.uniform_directions(rng, len(k)).astype(np.float64)
        b = np.cross(a, QR.uniform_directions(rng, len(k)))
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        # the line origin + s a passes at distance r from the centre: tangent (up to rounding, which either grazes or misses)
        sets["tangent"] = ((c + r[:, None] * b - 3.0 * r[:, None] * a).astype(np.float32), a.astype(np.float32))
    bad = np.array([np.nan, np.inf, -np.inf, 0.0], np.float32)
    dg_o = np.repeat(o[:1], 48, axis=0).copy()
    dg_d = np.repeat(d[:1], 48, axis=0).copy()
    for j in range(48):
        comp, val = j % 3, bad[(j // 3) % 4]
        if j < 12:
            dg_d[j] = 0.0                       # zero direction
        elif j < 30:
            dg_d[j, comp] = val                 # NaN / inf in the direction
        else:
            dg_o[j, comp] = val                 # ... in the origin
    sets["degenerate"] = (dg_o, dg_d)
    return sets


def _scene(name):
    if name == "demo":
        return R.builtin_scene_desc(R.SCENE_DEMO)
    if name == "demo-2500":
        return R.builtin_scene_desc(R.SCENE_DEMO, 2500)
    if name == "glass":
        return R.builtin_scene_desc(R.SCENE_GLASS_STRESS)
    if name.startswith("random-seed-"):
        seed = int(name.rsplit("-", 1)[1])
        return RS.random_scene(seed, n_spheres=[40, 300, 700][seed % 3], n_prisms=6 + seed % 5)
    if name == "many-prisms":
        return RS.random_scene(22, n_spheres=60, n_prisms=70)
    if name == "tables-prisms":
        return RS.random_scene(77, n_spheres=3000, n_prisms=48, n_planes=2, n_circles=3, n_parabs=1)
    if name == "random-6000":
        return RS.random_scene(41, n_spheres=6000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1)
    if name == "random-20000":
        return RS.random_scene(35, n_spheres=20000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1)
    if name.startswith("degenerate-"):   # the sphere layouts of test_gpu_parity.py, 57 spheres
        layout = name.split("-", 1)[1]
        objs0, cam = R.builtin_scene_desc(R.SCENE_DEMO)
        proto, rest = objs0[objs0["surface_kind"] == 0][:1], objs0[objs0["surface_kind"] != 0]
        rng = np.random.default_rng(7)
        n = 57
        o = np.repeat(proto, n)
        o["v0"] = rng.normal(0, 8, (n, 3)).astype(np.float32)
        o["v0"][:, 1] = np.abs(o["v0"][:, 1])
        o["f"][:, 0] = rng.uniform(0.1, 1.0, n).astype(np.float32)
        if layout == "same":
            o["v0"] = np.array([1.0, 2.0, 3.0], np.float32)
        elif layout == "line":
            o["v0"] = np.stack([np.linspace(-20, 20, n), np.ones(n), np.ones(n)], 1).astype(np.float32)
        elif layout == "zero_radius":
            o["f"][:, 0] = 0.0
        elif layout == "huge_spread":
            o["v0"] = (rng.normal(0, 1, (n, 3)) * np.exp(rng.uniform(-5, 12, (n, 1)))).astype(np.float32)
            o["f"][:, 0] = np.exp(rng.uniform(-8, 3, n)).astype(np.float32)
        elif layout == "infinite":
            o["f"][0, 0] = np.inf
        return np.concatenate([rest, o]), cam
    raise KeyError(name)


SCENES = ["demo", "demo-2500", "glass", "random-seed-1", "random-seed-2", "random-seed-3", "many-prisms", "tables-prisms",
          "degenerate-same", "degenerate-line", "degenerate-zero_radius", "degenerate-huge_spread", "degenerate-infinite",
          "random-6000", "random-20000"]
_ran = set()   # query variants seen by test_scene_queries_bit_exact (test_every_query_variant_ran reads it)


def _variant_of(before):
    return B._variant_of(R.query_launches, before)


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
            v = _variant_of(before)
            assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (name, fetch, v)
            _ran.add(v)
            assert_same(got, want, "%s %s fetch %d t_max inf" % (name, kind, fetch))
            assert_same(scene.intersect(o, d, t_max, fetch=fetch), want_t, "%s %s fetch %d t_max cases" % (name, kind, fetch))


def _filter(want, t_max):
    out = want.copy()
    miss = (want["object"] == NONE) | ~(want["distance"] < t_max)
    out[miss] = np.zeros(1, dtype=R.HIT_DTYPE)
    out["object"][miss] = NONE
    return out


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
            _ran.add(_variant_of(before))
    assert _ran == set(range(6)), sorted(_ran)


def _rays(o, d, t_max=np.inf):
    rays = np.zeros(len(o), dtype=R.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["t_max"] = o, d, t_max
    return rays


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
        dev = _device_query(scene, _rays(o, d), fetch)
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
                got = scene.intersect(o, d, fetch=FETCHES[(k + rep) % 2]) if rep % 2 else _device_query(scene, _rays(o, d), FETCHES[k % 2])
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
