"""PlotUnit.plot_photons / PlotUnit.render_samples on the device (rl_plot_unit_plot_photons*, rl_plot_unit_render_samples*): a film
for photons and camera samples the caller supplies.  Films are compared as tests/test_gpu_parity.py compares one
(test_plot_fused_and_unfused_match_oracle): np.allclose(rtol=2e-5, atol=1e-6 max) against the CPU oracle's plot of the same photons
AND the per-pixel bound of tests/_image_cases.py (within (k - 1) 2^-24 S of the exact sum of a pixel's k terms, the oracle's bits for
k <= 2); results are compared byte for byte with rl_scene_render_rays."""
import ctypes as C
import threading

import numpy as np
import pytest

import _boundary as B
import _image_cases as IC
import _oracle as O
import _path_oracle as P
import _query_rays as QR
from _boundary import _ocam
from _cases import _photons_of, synthetic_photons
from _compare import assert_film
from _device_arrays import _upload
from _scenes import _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
# the least share of paths that must carry a value (tests/test_gpu_path_query.py: IDENTITY_SCENES)
IDENTITY_SCENES = {"demo": 0.05, "glass": 0.05, "random-seed-1": 0.3, "demo-2500": 0.05}
BATCH_SIZES = [0, 1, 63, 64, 65, (1 << 20) + 4097]


def _render_samples_device(plot, scene, samples, seed, stream, first, fetch=R.FETCH_LDS, max_segments=0, results=True):
    sb = _upload(samples)
    if not results:
        plot.render_samples_device(scene, sb, seed, stream, first, fetch=fetch, max_segments=max_segments)
        return None
    res = np.zeros(len(samples), dtype=R.PATH_RESULT_DTYPE)
    res["end"] = 12345   # poison: every record must be written
    rb = _upload(res)
    plot.render_samples_device(scene, sb, seed, stream, first, fetch=fetch, max_segments=max_segments, results=rb)
    rb.download(res)
    return res


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return objs, cam, R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))


# ---- 1. the renderer's own photons ------------------------------------------------------------------------------------------

def test_plot_of_the_renderers_own_photons(demo):
    objs, cam, scene, oscene = demo
    n = 1 << 18
    t = R.TraceUnit(0, W, H, n_photons=n)
    t.render(scene, seed=1, stream=0, first_path_index=0)
    photons = t.mapped_photons
    assert (photons["probability"] != 0).mean() >= 0.05
    host = R.PlotUnit(0, W, H)
    host.plot_photons(photons)
    want = assert_film(host.tristimulus_buffer, W, H, photons, "host form")
    assert np.count_nonzero(want) > 1000
    dev = R.PlotUnit(1, W, H)
    dev.plot_photons_device(_upload(photons))
    assert_film(dev.tristimulus_buffer, W, H, photons, "device form")
    unit = R.PlotUnit(2, W, H)
    unit.plot([t])
    assert_film(unit.tristimulus_buffer, W, H, photons, "PlotUnit.plot of the same trace unit")


# ---- 2. photons no renderer makes -------------------------------------------------------------------------------------------

FILM_SHAPES = [s for s in IC.SMALL_SHAPES if min(s) >= 2] + [(1, 17), (17, 1), (1, 4097), (4097, 1), (1919, 1079)]
@pytest.mark.parametrize("shape", FILM_SHAPES, ids=IC.shape_id)
def test_photons_no_renderer_makes(shape):
    w, h = shape
    photons = synthetic_photons(w, h, 5)
    host = R.PlotUnit(0, w, h)
    host.plot_photons(photons)
    want = assert_film(host.tristimulus_buffer, w, h, photons, "host %dx%d" % shape)
    assert np.count_nonzero(want)
    dev = R.PlotUnit(1, w, h)
    dev.plot_photons_device(_upload(photons))
    assert_film(dev.tristimulus_buffer, w, h, photons, "device %dx%d" % shape)


@pytest.mark.parametrize("shape", [(320, 180), (37, 101), (1, 17), (17, 1)], ids=IC.shape_id)
def test_photons_with_a_non_finite_position_are_skipped(shape):
    w, h = shape
    valid = synthetic_photons(w, h, 6, 4000)
    rng = np.random.default_rng(8)
    odd = synthetic_photons(w, h, 7, 300)
    odd["probability"] = 1.0
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    odd["x"][0::3] = bad[np.arange(len(odd["x"][0::3])) % 3]
    odd["y"][1::3] = bad[np.arange(len(odd["y"][1::3])) % 3]
    odd["x"][2::3], odd["y"][2::3] = np.nan, -np.inf
    assert not (np.isfinite(odd["x"]) & np.isfinite(odd["y"])).any()
    mixed = np.concatenate([valid, odd])
    mixed = mixed[rng.permutation(len(mixed))]
    for form in ("host", "device"):
        p, q = R.PlotUnit(0, w, h), R.PlotUnit(1, w, h)
        if form == "host":
            p.plot_photons(mixed)
            q.plot_photons(odd)
        else:
            p.plot_photons_device(_upload(mixed))
            q.plot_photons_device(_upload(odd))
        assert_film(p.tristimulus_buffer, w, h, valid, "%s, mixed" % form)
        assert q.tristimulus_buffer.tobytes() == bytes(w * h * 12)   # a cleared buffer stays all zero bits


# ---- 3. identity with the renderer ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(IDENTITY_SCENES))
def test_camera_samples_rendered_onto_a_film_reproduce_the_renderer(name):
    objs, cam = _scene(name)
    scene, oscene = R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    big = len(objs) > 2000
    n, seed, stream, first = (8192 if big else 65536), 3 + len(name), 1, 1000
    want_photons, segs = oscene.render(W, H, seed, stream, first, n, threads=16)
    assert (want_photons["probability"] != 0).mean() >= IDENTITY_SCENES[name]   # an all-black film cannot pass
    assert np.count_nonzero(O.plot(W, H, want_photons)) > 0
    cyl = int((objs["surface_kind"] == 4).sum() >= 40)
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    for fetch in FETCHES:
        rays = scene.render_spectral_rays(samples["ray"], seed, stream, first, fetch=fetch)
        p = R.PlotUnit(0, W, H)
        before = R.film_launches()
        res = p.render_samples(scene, samples, seed, stream, first, fetch=fetch)
        v = B._variant_of(R.film_launches, before)
        assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0) and (fetch != R.FETCH_LDS or v // 2 == (1 if big else 2)), (name, fetch, v)
        assert res.tobytes() == rays.tobytes(), (name, fetch)
        assert res["value"].tobytes() == want_photons["probability"].tobytes() and int(res["segments"].sum(dtype=np.uint64)) == segs
        assert_film(p.tristimulus_buffer, W, H, want_photons, "%s fetch %d" % (name, fetch))
        q = R.PlotUnit(1, W, H)
        before = R.film_launches()
        assert q.render_samples(scene, samples, seed, stream, first, fetch=fetch, results=False) is None
        assert B._variant_of(R.film_launches, before) == v
        assert_film(q.tristimulus_buffer, W, H, want_photons, "%s fetch %d, no results" % (name, fetch))


def test_every_film_variant_ran():
    """Whole scene, tables only and nothing staged, each with and without the prisms' second bound, each against the path kernel's
    results and the oracle's plot of them.  Asserts on its own launches only."""
    ran = set()
    for name in ("demo", "many-prisms", "demo-2500", "tables-prisms"):
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        n = 4096
        samples = scene.camera_rays(W, H, 1, 0, 0, n)
        for fetch in FETCHES:
            rays = scene.render_spectral_rays(samples["ray"], 1, 0, 0, fetch=fetch)
            assert (rays["value"] != 0).any()
            for results in (True, False):
                p = R.PlotUnit(0, W, H)
                before = R.film_launches()
                res = p.render_samples(scene, samples, 1, 0, 0, fetch=fetch, results=results)
                ran.add(B._variant_of(R.film_launches, before))
                assert res is None or res.tobytes() == rays.tobytes(), (name, fetch)
                assert_film(p.tristimulus_buffer, W, H, _photons_of(samples, rays), "%s fetch %d" % (name, fetch))
    assert ran == set(range(6)), sorted(ran)


# ---- 4. a camera of the caller's own ----------------------------------------------------------------------------------------

def orthographic_samples(cam, n, rng, aspect):
    """A parallel bundle from a plane at the built-in camera's position looking at the origin (no built-in camera makes one),
    screen positions on a regular grid plus jitter, random wavelengths."""
    pos, fwd, right, up, fov = QR.camera_frame(cam)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    gx = ((i % side) + rng.random(n)) / side * 2.0 - 1.0
    gy = ((i // side) + rng.random(n)) / side * 2.0 - 1.0
    half = float(np.linalg.norm(pos)) * np.tan(fov * 0.5)
    s = np.zeros(n, dtype=R.CAMERA_SAMPLE_DTYPE)
    s["ray"]["origin"] = (pos[None, :] + (gx * half)[:, None] * right[None, :] - (gy * half / aspect)[:, None] * up[None, :]).astype(np.float32)
    s["ray"]["direction"] = fwd.astype(np.float32)
    s["ray"]["wavelength"] = rng.uniform(380.0, 780.0, n).astype(np.float32)
    s["x"] = gx.astype(np.float32)
    s["y"] = (gy / aspect).astype(np.float32)
    s["reserved0"], s["reserved1"], s["ray"]["reserved"] = 0xdeadbeef, 7, 0xffffffff   # ignored
    return s


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_a_camera_of_the_callers_own(name):
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    rng = np.random.default_rng(len(name))
    n, seed, stream, first = 2048, 12, 4, 1 << 33
    s = orthographic_samples(cam, n, rng, np.float32(W) / np.float32(H))
    r = s["ray"]
    want = P.PathOracle(objs, cam).render_rays(r["origin"], r["direction"], r["wavelength"], seed, stream, first).view(R.PATH_RESULT_DTYPE)
    photons = _photons_of(s, want)
    assert (want["value"] != 0).sum() >= 20 and np.count_nonzero(O.plot(W, H, photons)) > 0
    for fetch in FETCHES:
        p = R.PlotUnit(0, W, H)
        got = p.render_samples(scene, s, seed, stream, first, fetch=fetch)
        assert got.tobytes() == want.tobytes(), (name, fetch)
        assert_film(p.tristimulus_buffer, W, H, photons, "%s own camera, fetch %d" % (name, fetch))
        p = R.PlotUnit(0, W, H)
        assert _render_samples_device(p, scene, s, seed, stream, first, fetch=fetch).tobytes() == want.tobytes()
        assert_film(p.tristimulus_buffer, W, H, photons, "%s own camera, device form, fetch %d" % (name, fetch))


def test_the_built_in_camera_mirrored(demo):
    objs, cam, scene, oscene = demo
    n, seed, stream, first = 65536, 2, 0, 500
    want_photons, _ = oscene.render(W, H, seed, stream, first, n, threads=16)
    mirrored = want_photons.copy()
    mirrored["x"] = -mirrored["x"]   # (not a flipped image: (x * 0.5 + 0.5) * (w - 1) does not mirror exactly in f32)
    assert (mirrored["probability"] != 0).mean() >= 0.05
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    samples["x"] = -samples["x"]
    p = R.PlotUnit(0, W, H)
    res = p.render_samples(scene, samples, seed, stream, first)
    assert res["value"].tobytes() == want_photons["probability"].tobytes()
    assert_film(p.tristimulus_buffer, W, H, mirrored, "mirrored")


# ---- 5. batch sizes and splits ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCH_SIZES)
def test_plot_photons_batch_sizes(n):
    """Host form (staged in chunks of 2^20 records: the last size spans two) and device form."""
    photons = synthetic_photons(W, H, 9, max(n, 8))[:n]
    for form in ("host", "device"):
        p = R.PlotUnit(0, W, H)
        if form == "host":
            p.plot_photons(photons)
        else:
            p.plot_photons_device(_upload(photons))
        assert_film(p.tristimulus_buffer, W, H, photons, "%s n=%d" % (form, n))
    u = R.PlotUnit(0, W, H)
    assert R.lib.rl_plot_unit_plot_photons(u.handle, None, 0) == 0 and R.lib.rl_plot_unit_plot_photons_device(u.handle, None, 0) == 0


@pytest.mark.parametrize("n", BATCH_SIZES)
def test_render_samples_batch_sizes(demo, n):
    objs, cam, scene, oscene = demo
    seed, stream, first = 9, 0, 5
    want_photons, _ = oscene.render(W, H, seed, stream, first, n, threads=16) if n else (np.zeros(0, O.PHOTON_DTYPE), 0)
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    rays = scene.render_spectral_rays(samples["ray"], seed, stream, first)
    assert rays["value"].tobytes() == want_photons["probability"].tobytes()
    for form in ("host", "device"):
        for results in (True, False):
            p = R.PlotUnit(0, W, H)
            if form == "host":
                res = p.render_samples(scene, samples, seed, stream, first, results=results)
            else:
                res = _render_samples_device(p, scene, samples, seed, stream, first, results=results)
            assert res is None or res.tobytes() == rays.tobytes(), (form, n)
            assert_film(p.tristimulus_buffer, W, H, want_photons, "%s n=%d results=%s" % (form, n, results))
    u = R.PlotUnit(0, W, H)
    assert R.lib.rl_plot_unit_render_samples(u.handle, scene.handle, 0, 1, 0, 0, 0, None, 0, None) == 0
    assert R.lib.rl_plot_unit_render_samples_device(u.handle, scene.handle, 0, 1, 0, 0, 0, None, 0, None) == 0


def test_split_batches_give_the_same_results_and_film(demo):
    objs, cam, scene, oscene = demo
    n, seed, stream, first = 50000, 4, 1, 123
    want_photons, _ = oscene.render(W, H, seed, stream, first, n, threads=16)
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    whole_unit = R.PlotUnit(0, W, H)
    whole = whole_unit.render_samples(scene, samples, seed, stream, first)
    assert_film(whole_unit.tristimulus_buffer, W, H, want_photons, "whole")
    for a, b in ((1, 64), (12345, 12346), (63, 49999)):
        p = R.PlotUnit(1, W, H)
        parts = [p.render_samples(scene, samples[lo:hi], seed, stream, first + lo) for lo, hi in ((0, a), (a, b), (b, n))]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), (a, b)
        assert_film(p.tristimulus_buffer, W, H, want_photons, "split at %d, %d" % (a, b))


# ---- 6. a plot unit like any other ------------------------------------------------------------------------------------------

def test_render_samples_adds_to_a_plot_and_the_gather_sees_it(demo):
    objs, cam, scene, oscene = demo
    n = 1 << 16
    a, _ = oscene.render(W, H, 1, 0, 0, n, threads=16)
    b, _ = oscene.render(W, H, 7, 1, 0, n, threads=16)
    t = R.TraceUnit(0, W, H, n_photons=n)
    t.render(scene, 1, 0, 0)
    p = R.PlotUnit(0, W, H)
    p.plot([t])
    samples = scene.camera_rays(W, H, 7, 1, 0, n)
    res = p.render_samples(scene, samples, 7, 1, 0)
    assert res["value"].tobytes() == b["probability"].tobytes()
    g = R.GatherUnit(W, H)
    g.accumulate(p)   # straight after it, no sync call: gathers both and clears
    both = np.concatenate([a, b])
    assert_film(g.tristimulus_buffer, W, H, both, "plot + render_samples, gathered")
    assert p.tristimulus_buffer.tobytes() == bytes(W * H * 12)
    p.render_samples(scene, samples, 7, 1, 0, results=False)   # and the cleared unit takes the next film
    assert_film(p.tristimulus_buffer, W, H, b, "after the gather's clear")


def test_render_samples_after_render_fused_begin_into_the_same_unit(demo):
    objs, cam, scene, oscene = demo
    n = 1 << 16
    a, _ = oscene.render(W, H, 5, 0, 0, n, threads=16)
    b, _ = oscene.render(W, H, 7, 1, 0, 8192, threads=16)
    samples = scene.camera_rays(W, H, 7, 1, 0, 8192)
    t = R.TraceUnit(0, W, H, n_photons=n)
    p = R.PlotUnit(0, W, H)
    t.render_fused_begin(scene, p, n, seed=5, stream=0, first_path_index=0)
    res = p.render_samples(scene, samples, 7, 1, 0)   # ends the begun render first
    assert res["value"].tobytes() == b["probability"].tobytes()
    assert_film(p.tristimulus_buffer, W, H, np.concatenate([a, b]), "fused_begin + render_samples")
    p.clear()
    t.render_fused_begin(scene, p, n, seed=5, stream=0, first_path_index=0)
    p.plot_photons(b)
    assert_film(p.tristimulus_buffer, W, H, np.concatenate([a, b]), "fused_begin + plot_photons")


def test_render_samples_between_render_begin_and_end(demo):
    objs, cam, scene, oscene = demo
    N = 1 << 16
    want_photons, segs = oscene.render(W, H, 5, 0, 0, N, threads=16)
    want, _ = oscene.render(W, H, 7, 1, 0, 8192, threads=16)
    samples = scene.camera_rays(W, H, 7, 1, 0, 8192)
    for fetch in FETCHES:
        t = R.TraceUnit(0, W, H, n_photons=N)
        p = R.PlotUnit(0, W, H)
        R.check(R.lib.rl_trace_unit_render_begin(t.handle, scene.handle, 5, 0, 0))
        got = p.render_samples(scene, samples, 7, 1, 0, fetch=fetch)
        p.plot_photons(want)
        R.check(R.lib.rl_trace_unit_render_end(t.handle))
        assert got["value"].tobytes() == want["probability"].tobytes(), fetch
        assert_film(p.tristimulus_buffer, W, H, np.concatenate([want, want]), "between begin and end, fetch %d" % fetch)
        assert t.mapped_photons.tobytes() == want_photons.tobytes() and t.stats()[:2] == (N, segs)


def test_four_threads_four_plot_units_one_scene(demo):
    objs, cam, scene, oscene = demo
    jobs = []
    for k in range(4):
        n, first = 3000 + 1000 * k, 10000 * k
        want, _ = oscene.render(W, H, 6, k, first, n, threads=4)
        jobs.append((k, first, scene.camera_rays(W, H, 6, k, first, n), want))
    errors, barrier = [], threading.Barrier(4)

    def worker(k, first, samples, want):
        try:
            barrier.wait()
            for rep in range(6):
                fetch = FETCHES[(k + rep) % 2]
                p = R.PlotUnit(k, W, H)
                if rep % 2:
                    got = p.render_samples(scene, samples, 6, k, first, fetch=fetch)
                else:
                    got = _render_samples_device(p, scene, samples, 6, k, first, fetch=fetch)
                assert got["value"].tobytes() == want["probability"].tobytes(), (k, rep)
                assert_film(p.tristimulus_buffer, W, H, want, "thread %d rep %d" % (k, rep))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(240)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors


# ---- 7. what the device forms refuse ----------------------------------------------------------------------------------------

def test_device_forms_refuse_host_memory(demo):
    objs, cam, scene, oscene = demo
    p = R.PlotUnit(0, W, H)
    photons = synthetic_photons(W, H, 1, 64)
    rc = R.lib.rl_plot_unit_plot_photons_device(p.handle, photons.ctypes.data_as(C.c_void_p), 64)
    assert rc == -1 and b"device memory" in R.lib.rl_last_error()
    samples, res = scene.camera_rays(W, H, 1, 0, 0, 64), np.zeros(64, R.PATH_RESULT_DTYPE)
    sb, rb = _upload(samples), _upload(res)
    sp, rp = samples.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    fn = R.lib.rl_plot_unit_render_samples_device
    assert fn(p.handle, scene.handle, 0, 1, 0, 0, 0, sp, 64, None) == -1 and b"device memory" in R.lib.rl_last_error()
    assert fn(p.handle, scene.handle, 0, 1, 0, 0, 0, C.c_void_p(sb.data_ptr()), 64, rp) == -1 and b"device memory" in R.lib.rl_last_error()
    assert fn(p.handle, scene.handle, 0, 1, 0, 0, 0, sp, 64, C.c_void_p(rb.data_ptr())) == -1 and b"device memory" in R.lib.rl_last_error()
    assert p.tristimulus_buffer.tobytes() == bytes(W * H * 12) and res.tobytes() == bytes(res.nbytes)


def test_a_unit_and_a_scene_on_different_devices_are_refused():
    if R.device_count() < 2:
        pytest.skip("needs two devices")
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam, device=0)
    p = R.PlotUnit(0, W, H, device=1)
    samples = scene.camera_rays(W, H, 1, 0, 0, 64)
    with pytest.raises(R.RlError) as e:
        p.render_samples(scene, samples, 1, 0, 0)
    assert e.value.code == -5 and "different devices" in str(e.value)
    assert p.tristimulus_buffer.tobytes() == bytes(W * H * 12)


# ---- 8. invalid and limited paths leave no mark -----------------------------------------------------------------------------

def test_invalid_and_limited_paths_leave_no_mark(demo):
    objs, cam, scene, oscene = demo
    n, seed, stream, first = 8192, 8, 0, 0
    samples = scene.camera_rays(W, H, seed, stream, first, n)
    full = scene.render_spectral_rays(samples["ray"], seed, stream, first)
    lit = np.flatnonzero(full["value"] != 0)
    assert len(lit) >= n // 20
    # every path that would have carried a value gets a non-finite wavelength, a non-finite position, or stays as it is
    odd = samples.copy()
    odd["ray"]["wavelength"][lit[0::3]] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(lit[0::3])) % 3]
    odd["x"][lit[1::3]] = np.nan
    odd["y"][lit[1::3][::2]] = np.inf
    rays = scene.render_spectral_rays(odd["ray"], seed, stream, first)
    assert (rays["end"][lit[0::3]] == R.RL_PATH_END_INVALID).all() and rays[lit[1::3]].tobytes() == full[lit[1::3]].tobytes()
    keep = np.ones(n, bool)
    keep[lit[0::3]] = keep[lit[1::3]] = False
    want_photons = _photons_of(samples, full)[keep]
    assert (want_photons["probability"] != 0).sum() >= len(lit) // 4
    for results in (True, False):
        p = R.PlotUnit(0, W, H)
        res = p.render_samples(scene, odd, seed, stream, first, results=results)
        assert res is None or res.tobytes() == rays.tobytes()
        assert_film(p.tristimulus_buffer, W, H, want_photons, "invalid wavelengths and positions, results=%s" % results)
    # one segment: only a camera ray that starts towards a light ends with a value
    limited = scene.render_spectral_rays(samples["ray"], seed, stream, first, max_segments=1)
    assert (limited["end"] == R.RL_PATH_END_LIMIT).sum() >= n // 2 and (limited["value"][limited["end"] == R.RL_PATH_END_LIMIT] == 0).all()
    p = R.PlotUnit(0, W, H)
    res = p.render_samples(scene, samples, seed, stream, first, max_segments=1)
    assert res.tobytes() == limited.tobytes()
    assert_film(p.tristimulus_buffer, W, H, _photons_of(samples, limited), "max_segments = 1")
    nowhere = samples[limited["end"] == R.RL_PATH_END_LIMIT]   # ... and rays that do not start on a light leave the film as it was
    p.clear()
    p.render_samples(scene, nowhere, seed, stream, first, max_segments=1, results=False)
    assert p.tristimulus_buffer.tobytes() == bytes(W * H * 12)
