"""Scene.begin_paths / Scene.step_paths on the device (rl_scene_begin_paths*, rl_scene_step_paths*), bit for bit and through the C
ABI: begun and stepped until nothing is live they give rl_scene_render_rays' results, with and without compaction and shuffling
between steps; every field of every state and every hit equals the Python restatement of one loop turn (tests/_step_oracle.py)
after each of the first steps; hits equal rl_scene_intersect's; RL_STEP_NO_ROULETTE; states that are not live are untouched;
invalid wavelengths; batch sizes, splits, host and device forms, fetch modes and every kernel variant; concurrent callers and a
step made while a render is open."""
import ctypes as C
import threading

import numpy as np
import pytest

import _oracle as O
import _query_rays as QR
import _step_oracle as S
from _cases import _results
from _compare import assert_same
from _device_arrays import _Device, _begin_device, _poison_hits
from _scenes import _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE, LIVE = R.RL_OBJECT_NONE, R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
# the scenes of test_gpu_path_query.py's IDENTITY_SCENES: the whole scene staged (demo, glass, random-seed-*, many-prisms), tables only
# with a third cull level (demo-2500, random-6000), prisms with the second bound (many-prisms)
IDENTITY_SCENES = ("demo", "glass", "random-seed-1", "random-seed-2", "many-prisms", "demo-2500", "random-6000")
BUDGET = R.RL_PATH_MAX_SEGMENTS


def _identity_case(name):
    objs, cam = _scene(name)
    n, seed, stream, first = (8192 if len(objs) > 2000 else 65536), 3 + len(name), 1, 1000
    return objs, cam, n, seed, stream, first


def _step_device(scene, sb, seed, stream, fetch=R.FETCH_LDS, flags=0, hb=None):
    R.check(R.lib.rl_scene_step_paths_device(scene.handle, fetch, seed, stream, flags, C.c_void_p(sb.buf.data_ptr()), len(sb.host),
                                             C.c_void_p(hb.buf.data_ptr()) if hb is not None else None))


def _run_uncompacted(scene, rays, seed, stream, first, fetch):
    """begin_paths, then step_paths on the whole batch until nothing is live (at most BUDGET steps): (final states, steps)."""
    sb = _begin_device(scene, rays, first)
    steps = 0
    while steps < BUDGET and (sb.get()["end"] == LIVE).any():
        _step_device(scene, sb, seed, stream, fetch)
        steps += 1
    return sb.get().copy(), steps


@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_identity_uncompacted(name):
    objs, cam, n, seed, stream, first = _identity_case(name)
    scene = R.Scene(objs, cam)
    rays = np.ascontiguousarray(scene.camera_rays(W, H, seed, stream, first, n)["ray"])
    want = scene.render_spectral_rays(rays, seed, stream, first)
    assert (want["end"] != R.RL_PATH_END_LIMIT).all()   # a path the budget cut short fails here instead of dropping out
    assert (want["value"] != 0).mean() >= 0.05
    begun = scene.begin_paths(rays, first)
    assert_same(_begin_device(scene, rays, first).get(), begun, "%s begin: device vs host" % name)
    assert begun.tobytes() == S.begin(rays, first).tobytes()
    for fetch in FETCHES:
        final, steps = _run_uncompacted(scene, rays, seed, stream, first, fetch)
        assert (final["end"] != LIVE).all(), (name, fetch, int((final["end"] == LIVE).sum()))
        assert steps == int(want["segments"].max()) <= BUDGET, (name, steps)
        assert_same(_results(final), want, "%s fetch %d" % (name, fetch))
        assert (final["path_index"] == first + np.arange(n)).all() and (final["reserved"] == 0).all()
        assert final["wavelength"].tobytes() == rays["wavelength"].tobytes()
    # the host form, stepped the same way
    st = begun.copy()
    for _ in range(steps):
        scene.step_paths(st, seed, stream)
    assert_same(st, final, "%s host form" % name)


@pytest.mark.parametrize("name", ["demo", "glass", "many-prisms", "random-6000"])
def test_identity_under_compaction_and_shuffling(name):
    objs, cam, n, seed, stream, first = _identity_case(name)
    scene = R.Scene(objs, cam)
    rays = np.ascontiguousarray(scene.camera_rays(W, H, seed, stream, first, n)["ray"])
    want = scene.render_spectral_rays(rays, seed, stream, first)
    plain, _ = _run_uncompacted(scene, rays, seed, stream, first, R.FETCH_LDS)
    rng = np.random.default_rng(len(name))
    final = np.zeros(n, R.PATH_STATE_DTYPE)
    final["end"] = 777
    cur = _begin_device(scene, rays, first).get().copy()
    steps = 0
    while len(cur) and steps <= BUDGET:
        done = cur["end"] != LIVE
        final[(cur["path_index"][done] - first).astype(np.int64)] = cur[done]
        live = cur[~done]
        if not len(live):
            cur = live
            break
        sb = _Device(live[rng.permutation(len(live))])   # only the live states, in a seeded random order, in fresh device memory
        _step_device(scene, sb, seed, stream, FETCHES[steps % 2])
        cur = sb.get().copy()
        steps += 1
    assert not len(cur) and (final["end"] != 777).all()
    assert_same(final, plain, "%s compacted vs uncompacted" % name)
    assert_same(_results(final), want, "%s compacted" % name)


def _mixed_states(name, rng):
    """A few thousand begun states on scene `name`: camera rays, rays that start just behind the surfaces they hit (inside glass),
    non-unit directions (x2 and x0.5: the exact scan), rays into the void and rays aimed at the lights."""
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    o, d = QR.camera_rays(cam, 1920, 1080, rng, 1024)
    bo, bd = QR.bounce_rays(o, d, scene.intersect(o, d), rng)
    far = (QR.uniform_directions(rng, 256) * np.float32(500.0)).astype(np.float32)
    lights = objs[(objs["material_kind"] == 0) & (objs["surface_kind"] == 0)]
    assert len(lights)
    lo = (rng.normal(0, 3, (256, 3))).astype(np.float32)
    lc = lights["v0"][rng.integers(0, len(lights), 256)]
    ld = (lc - lo) / np.linalg.norm(lc - lo, axis=1, keepdims=True)
    origins = np.concatenate([o, bo, o[:256], bo[:256], far, lo]).astype(np.float32)
    directions = np.concatenate([d, bd, d[:256] * np.float32(2.0), bd[:256] * np.float32(0.5), far / np.float32(500.0), ld]).astype(np.float32)
    rays = np.zeros(len(origins), R.SPECTRAL_RAY_DTYPE)
    rays["origin"], rays["direction"] = origins, directions
    rays["wavelength"] = rng.uniform(380.0, 780.0, len(rays)).astype(np.float32)
    return objs, cam, scene, rays


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_every_step_matches_the_step_oracle(name):
    rng = np.random.default_rng(len(name))
    objs, cam, scene, rays = _mixed_states(name, rng)
    assert 2000 <= len(rays) <= 8000
    seed, stream, first = 5, 2, int(rng.integers(0, 1 << 40))
    so = S.StepOracle(objs, cam)
    want = S.begin(rays, first)
    want_hits = _poison_hits(len(rays))
    got = {f: (_begin_device(scene, rays, first), _Device(_poison_hits(len(rays)))) for f in FETCHES}
    ends = set()
    for step in range(8):
        so.step(want, seed, stream, hits=want_hits)
        ends |= set(np.unique(want["end"]).tolist())
        for fetch, (sb, hb) in got.items():
            _step_device(scene, sb, seed, stream, fetch, hb=hb)
            assert_same(sb.get(), want, "%s step %d fetch %d: states" % (name, step, fetch))
            assert_same(hb.get(), want_hits, "%s step %d fetch %d: hits" % (name, step, fetch))
    assert ends >= {R.RL_PATH_END_VOID, R.RL_PATH_END_EMITTER, R.RL_PATH_END_ROULETTE, LIVE}, ends
    assert (want["segments"] == 8).any() and (want["value"] != 0).any()


@pytest.mark.parametrize("name", ["demo", "glass", "random-6000"])
def test_hits_are_scene_intersect_and_null_hits_change_nothing(name):
    rng = np.random.default_rng(7)
    if name == "random-6000":
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        rays = np.ascontiguousarray(scene.camera_rays(W, H, 2, 0, 0, 4096)["ray"])
    else:
        objs, cam, scene, rays = _mixed_states(name, rng)
    seed, stream, first = 12, 1, 99
    for fetch in FETCHES:
        st = scene.begin_paths(rays, first)
        for step in range(4):
            live = st["end"] == LIVE
            want = scene.intersect(st["origin"], st["direction"], fetch=fetch)
            hits = _poison_hits(len(st))
            without = scene.step_paths(st.copy(), seed, stream, fetch=fetch)
            scene.step_paths(st, seed, stream, fetch=fetch, hits=hits)
            assert_same(st, without, "%s step %d: NULL hits" % (name, step))
            assert_same(hits[live], want[live], "%s step %d fetch %d" % (name, step, fetch))
            assert hits[~live].tobytes() == _poison_hits(int((~live).sum())).tobytes()
            assert live.any()


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_no_roulette_flag(name):
    rng = np.random.default_rng(11)
    objs, cam, scene, rays = _mixed_states(name, rng)
    seed, stream, first = 31, 4, 1 << 33
    st = scene.begin_paths(rays, first)
    ended_by_roulette = 0
    for step in range(3):
        before = st.copy()
        plain = scene.step_paths(st.copy(), seed, stream)
        flagged = scene.step_paths(st.copy(), seed, stream, flags=R.RL_STEP_NO_ROULETTE)
        for f in R.PATH_STATE_DTYPE.names:
            if f != "end":
                assert flagged[f].tobytes() == plain[f].tobytes(), (name, step, f)
        differs = flagged["end"] != plain["end"]
        assert ((flagged["end"][differs] == LIVE) & (plain["end"][differs] == R.RL_PATH_END_ROULETTE)).all()
        assert not (flagged["end"] == R.RL_PATH_END_ROULETTE).any()
        # the reference's comparison, applied on the host to the flagged states that bounced, reproduces the flag-0 `end`
        bounced = np.flatnonzero((before["end"] == LIVE) & (flagged["end"] == LIVE))
        assert len(bounced) > 100
        for i in bounced:
            ends = S.roulette_ends(seed, stream, int(flagged["path_index"][i]), 2 + int(before["segments"][i]), flagged["intensity"][i],
                                   flagged["continue_chance"][i])
            assert ends == (plain["end"][i] == R.RL_PATH_END_ROULETTE), (name, step, int(i))
        ended_by_roulette += int(differs.sum())
        st = flagged   # goes on past the roulette
    assert ended_by_roulette > 0
    live = st["end"] == LIVE   # three bounces each, whatever the roulette said
    assert live.any() and (st["segments"][live] == 3).all()
    assert (st["continue_chance"][live] == np.float32(1) * np.float32(0.96) * np.float32(0.96) * np.float32(0.96)).all()


def test_states_that_are_not_live_are_untouched():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    n = 64 * 37 + 5
    rays = np.ascontiguousarray(scene.camera_rays(W, H, 3, 0, 0, n)["ray"])
    st = scene.begin_paths(rays, 0)
    ends = np.array([LIVE, R.RL_PATH_END_VOID, R.RL_PATH_END_EMITTER, R.RL_PATH_END_ROULETTE, R.RL_PATH_END_LIMIT, R.RL_PATH_END_INVALID,
                     7, 0xfffffffe], np.uint32)[np.arange(n) % 8]
    dead = ends != LIVE
    raw = st.view(np.uint8).reshape(n, 64)
    raw[dead] = 0xc3                     # a poison pattern over the whole record ...
    st["end"][dead] = ends[dead]         # ... but for the word that says it is not live
    before = st.copy()
    for fetch in FETCHES:
        host, hits = before.copy(), _poison_hits(n)
        scene.step_paths(host, 1, 0, fetch=fetch, hits=hits)
        sb, hb = _Device(before), _Device(_poison_hits(n))
        _step_device(scene, sb, 1, 0, fetch, hb=hb)
        for got, got_hits in ((host, hits), (sb.get(), hb.get())):
            assert got[dead].tobytes() == before[dead].tobytes()
            assert got_hits[dead].tobytes() == _poison_hits(int(dead.sum())).tobytes()
            assert (got["segments"][~dead] == 1).all() and (got_hits["reserved"][~dead] == 0).all()
        assert_same(sb.get(), host, "device vs host")


def test_invalid_wavelengths_are_never_stepped():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    n = 1000
    rays = np.ascontiguousarray(scene.camera_rays(W, H, 3, 0, 0, n)["ray"])
    bad = np.arange(n) % 5 == 0
    rays["wavelength"][bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(bad.sum())) % 3]
    st = scene.begin_paths(rays, 40)
    assert (st["end"][bad] == R.RL_PATH_END_INVALID).all() and (st["end"][~bad] == LIVE).all()
    assert (st["value"] == 0).all() and (st["segments"] == 0).all() and (st["object"] == NONE).all()
    assert_same(_begin_device(scene, rays, 40).get(), st, "begin: device vs host")
    begun = st.copy()
    hits = _poison_hits(n)
    for _ in range(3):
        scene.step_paths(st, 1, 0, hits=hits)
    assert st[bad].tobytes() == begun[bad].tobytes() and hits[bad].tobytes() == _poison_hits(int(bad.sum())).tobytes()
    want = scene.render_spectral_rays(rays, 1, 0, 40, max_segments=3)
    ended = st["end"] != LIVE
    assert_same(_results(st[ended]), want[ended], "three steps against max_segments = 3")
    assert (want["end"][~ended] == R.RL_PATH_END_LIMIT).all()


def _variants_since(before):
    return {i for i, (a, b) in enumerate(zip(R.step_launches(), before)) if a != b}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, (1 << 20) + 4097])
def test_batch_sizes_splits_forms_and_fetches_give_the_same_bytes(n):
    """Host form (staged in chunks of 2^20 records: the last size spans two) and device form, LDS and global fetch, whole and
    split batches, on the built-in scene, a tables-only scene and one with a third cull level: the same bytes."""
    ran = set()
    for name in ("demo", "demo-2500", "random-6000", "many-prisms", "tables-prisms"):
        if n > 65 and name in ("many-prisms", "tables-prisms"):
            continue
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        seed, stream, first = 9, 0, 5
        rays = np.ascontiguousarray(scene.camera_rays(W, H, seed, stream, first, n)["ray"])
        begun = scene.begin_paths(rays, first)
        assert len(begun) == n
        ref = ref_hits = None
        for fetch in FETCHES:
            before = R.step_launches()
            st, hits = begun.copy(), _poison_hits(n)
            sb, hb = _Device(begun), _Device(_poison_hits(n))
            for _ in range(2):
                scene.step_paths(st, seed, stream, fetch=fetch, hits=hits)
                if n:
                    _step_device(scene, sb, seed, stream, fetch, hb=hb)
            v = _variants_since(before)
            assert len(v) == (1 if n else 0), (name, fetch, v)
            ran |= v
            if ref is None:
                ref, ref_hits = st, hits
            assert_same(st, ref, "%s n=%d fetch %d" % (name, n, fetch))
            assert_same(hits, ref_hits, "%s n=%d fetch %d: hits" % (name, n, fetch))
            assert_same(sb.get(), ref, "%s n=%d fetch %d: device form" % (name, n, fetch))
            assert_same(hb.get(), ref_hits, "%s n=%d fetch %d: device form, hits" % (name, n, fetch))
        for k in sorted({1, 64, n // 3, n - 1} & set(range(1, n))):   # split batches, in another order
            a, b = begun[k:].copy(), begun[:k].copy()
            for _ in range(2):
                scene.step_paths(a, seed, stream)
                scene.step_paths(b, seed, stream, fetch=R.FETCH_GLOBAL)
            assert_same(np.concatenate([b, a]), ref, "%s n=%d split at %d" % (name, n, k))
        if n:
            assert (ref["segments"] >= 1).all() and (n < 63 or (ref["end"] != LIVE).any())
    if 0 < n <= 65:
        assert ran == set(range(6)), sorted(ran)   # every instantiation of the step kernel ran
    assert R.lib.rl_scene_step_paths_device(scene.handle, 0, 1, 0, 0, None, 0, None) == 0
    assert R.lib.rl_scene_begin_paths_device(scene.handle, 0, None, 0, None) == 0


def test_device_forms_refuse_host_memory():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    rays = np.zeros(64, R.SPECTRAL_RAY_DTYPE)
    raw = np.zeros(64 * 64 + 16, np.uint8)
    off = (-raw.ctypes.data) % 16   # (16-byte aligned: the check under test is the memory's kind)
    st = raw[off:off + 64 * 64].view(R.PATH_STATE_DTYPE)
    assert st.ctypes.data % 16 == 0 and len(st) == 64
    st["end"] = LIVE
    before = st.tobytes()
    hits = np.zeros(64, R.HIT_DTYPE)
    sp, hp, rp = st.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p)
    assert R.lib.rl_scene_step_paths_device(scene.handle, 0, 1, 0, 0, sp, 64, None) == -1 and b"device memory" in R.lib.rl_last_error()
    assert R.lib.rl_scene_begin_paths_device(scene.handle, 0, rp, 64, sp) == -1 and b"device memory" in R.lib.rl_last_error()
    sb = _Device(st)
    assert R.lib.rl_scene_step_paths_device(scene.handle, 0, 1, 0, 0, C.c_void_p(sb.buf.data_ptr()), 64, hp) == -1
    assert b"device memory" in R.lib.rl_last_error()
    assert R.lib.rl_scene_begin_paths_device(scene.handle, 0, rp, 64, C.c_void_p(sb.buf.data_ptr())) == -1
    assert b"device memory" in R.lib.rl_last_error()
    assert R.lib.rl_scene_step_paths_device(scene.handle, 0, 1, 0, 0, C.c_void_p(sb.buf.data_ptr() + 8), 63, None) == -1
    assert b"aligned" in R.lib.rl_last_error()
    assert st.tobytes() == before and sb.get().tobytes() == before


def test_four_threads_step_on_one_scene():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    jobs = []
    for k in range(4):
        n, first = 3000 + 1000 * k, 10000 * k
        rays = np.ascontiguousarray(scene.camera_rays(W, H, 6, k, first, n)["ray"])
        jobs.append((k, first, rays, scene.render_spectral_rays(rays, 6, k, first)))
    errors, barrier = [], threading.Barrier(4)

    def worker(k, first, rays, want):
        try:
            barrier.wait()
            for rep in range(3):
                fetch = FETCHES[(k + rep) % 2]
                if rep % 2:
                    st = scene.begin_paths(rays, first)
                    while (st["end"] == LIVE).any():
                        scene.step_paths(st, 6, k, fetch=fetch)
                else:
                    st, _ = _run_uncompacted(scene, rays, 6, k, first, fetch)
                assert _results(st).tobytes() == want.tobytes(), (k, rep)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


def test_step_between_render_begin_and_end():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    oscene = O.Scene(objs.view(O.OBJECT_DTYPE), O.RlCameraDesc.from_buffer_copy(bytes(cam)))
    N = 1 << 16
    want_photons, segs = oscene.render(W, H, 5, 0, 0, N, threads=16)
    rays = np.ascontiguousarray(scene.camera_rays(W, H, 7, 1, 0, 8192)["ray"])
    want = scene.step_paths(scene.begin_paths(rays, 0), 7, 1)
    for fetch in FETCHES:
        t = R.TraceUnit(0, W, H, n_photons=N)
        R.check(R.lib.rl_trace_unit_render_begin(t.handle, scene.handle, 5, 0, 0))
        got = scene.step_paths(scene.begin_paths(rays, 0), 7, 1, fetch=fetch)
        R.check(R.lib.rl_trace_unit_render_end(t.handle))
        assert_same(got, want, "fetch %d" % fetch)
        assert t.mapped_photons.tobytes() == want_photons.tobytes() and t.stats()[:2] == (N, segs)
