"""PlotUnit.light_paths* and PlotUnit.render_samples_direct* on the device (rl_plot_unit_light_paths*,
rl_plot_unit_render_samples_direct*): the sample records against rl_scene_light_paths' byte for byte on all six variants; the film
against the CPU oracle's plot of the photons the numpy statement of the rule (tests/_light_film_oracle.py) builds from those
samples, by the film tests' bar (tests/_compare.py: assert_film: the tolerance and the per-pixel bound, the oracle's bits where a
component has at most two terms, which on the camera's own 320x180 film is nearly all of them -- tests/test_light_film_abi.py
measures what that catches), with rl_plot_unit_plot_photons' film of the same photons beside it, and the `sampled` bytes exactly;
the drop rule's corners on a scene
built for them; a hostile list into guarded buffers; every variant on poisoned LDS; the direct render against the loop of public
calls and rl_scene_render_rays; and the estimator's mean against the paths' own.  A GPU fault ends the run: nothing here provokes
one."""
import numpy as np
import pytest

import _guarded as G
import _image_cases as IC
import _lds_poison as LP
import _light_film_oracle as FO
import _oracle as O
import _query_rays as QR
from _boundary import _ocam
from _cases import _stepped_camera
from _compare import assert_film, assert_means_agree, assert_same
from _device_arrays import _Device, _Words, _prefilled, _slice_crossing_size
from _scenes import _lit_scene, _scene, closed_scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
SCENES = ["demo", "many-prisms", "demo-2500", "tables-prisms", "random-6000"]   # whole scene / tables / third level, with and without CYL
SAMPLE = R.LIGHT_SAMPLE_DTYPE
W, H = 320, 180      # the camera the paths are drawn for
# 16x9 and 64x36 are the contention cases for the atomics (a plot unit is free to be smaller than the camera's film); on the camera's
# own film almost every component collects one or two terms, and the device must then give the oracle's bits
FILMS = ((16, 9), (64, 36), (W, H))


def _some_bytes(n, rng):
    """`sampled` as a caller may hold it: zero, one, and other non-zero values."""
    return rng.choice(np.array([0, 0, 1, 1, 0xAA], np.uint8), n)


def _plot_of(w, h, photons):
    plot = R.PlotUnit(0, w, h)
    plot.plot_photons(photons)
    return plot.tristimulus_buffer


def assert_light_film(got, w, h, photons, what, beside=None):
    """The film tests' bar (tests/_compare.py: assert_film): `got` against the CPU oracle's plot of `photons`, which the numpy
    restatement reproduces bit for bit, by np.allclose(rtol=2e-5, atol=1e-6 max) AND the per-pixel bound against the exact sum,
    the oracle's bits where a component has at most two terms.  `beside` is a film of the same photons made on the device by
    other calls (rl_plot_unit_plot_photons, the loop of public calls), itself held to that bar where it is made: a second
    comparison, by the tolerance for a different order of the float atomics."""
    want = assert_film(got, w, h, photons, what)
    if beside is not None:
        scale = float(np.abs(beside).max())
        print("%s: max |got - device film| %.3e, image max %.3e" % (what, float(np.abs(got - beside).max()), scale))
        assert np.allclose(got, beside, rtol=2e-5, atol=1e-6 * scale), what
    return want


def _expected(scene, st, hits, camera, sampled, seed, stream, w, h, lst=None, n_list=None):
    """(rl_plot_unit_plot_photons' film of the photons, sampled bytes, samples, photons) the call must produce on a cleared film:
    the composition of today's public calls."""
    samples = scene.light_paths(st, hits, seed, stream, list=lst, n_list=n_list, samples=_prefilled(len(st)))
    photons, after = FO.film_photons(st, samples, scene.emitters(), camera, sampled, lst, n_list)
    film = _plot_of(w, h, photons)
    assert_film(film, w, h, photons, "plot_photons of the composition's %d photons" % len(photons))
    return film, after, samples, photons


def _call_device(scene, w, h, st, hits, camera, sampled, seed, stream, lst=None, n_list=None, fetch=R.FETCH_LDS, want_samples=True):
    """One device-form call onto a cleared film: (film, sampled bytes, samples, variant that ran)."""
    plot = R.PlotUnit(0, w, h)
    sb, hb, cb = _Device(st), _Device(hits), _Device(camera)
    yb = None if sampled is None else _Device(sampled)
    mb = _Device(_prefilled(len(st))) if want_samples else None
    lb = None if lst is None else _Words(lst)
    before = R.light_film_launches()
    plot.light_paths_device(scene, sb.buf, hb.buf, cb.buf, seed, stream, list=None if lb is None else lb.buf,
                            n_list=(len(st) if lst is None else len(lst)) if n_list is None else n_list, fetch=fetch,
                            sampled=None if yb is None else yb.buf, samples=None if mb is None else mb.buf)
    ran = [a - b for a, b in zip(R.light_film_launches(), before)]
    assert sum(ran) == 1, ran
    assert sb.get().tobytes() == st.tobytes() and hb.get().tobytes() == hits.tobytes() and cb.get().tobytes() == camera.tobytes()
    return plot.tristimulus_buffer, None if yb is None else yb.get().copy(), None if mb is None else mb.get().copy(), ran.index(1)


# ---- 1. the samples, bit for bit ---------------------------------------------------------------------------------------------

def test_samples_are_light_paths_in_every_byte_on_all_six_variants():
    ran = set()
    for name in SCENES:
        objs, cam = _lit_scene(name)
        scene = R.Scene(objs, cam)
        cyl = int((objs["surface_kind"] == 4).sum() >= 40)
        n, seed, stream, first = 4097, 7, 1, 1 << 34
        camera, st, hits = _stepped_camera(scene, n, seed, stream, first, 2)
        want = scene.light_paths(st, hits, seed, stream, samples=_prefilled(n))
        for fetch in FETCHES:
            what = "%s fetch %d" % (name, fetch)
            _, _, got, v = _call_device(scene, 16, 9, st, hits, camera, np.zeros(n, np.uint8), seed, stream, fetch=fetch)
            assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
            ran.add(v)
            assert_same(got, want, what)
        host = R.PlotUnit(0, 16, 9).light_paths(scene, st, hits, camera, seed, stream, samples=_prefilled(n))
        assert_same(host, want, name + ": host form")
    assert ran == set(range(6)), sorted(ran)


# ---- 2. the film against the composition -------------------------------------------------------------------------------------

def _composition(name, film_of_steps):
    """The film, the bytes and the samples of every form of the call against the composition, after one, two and three steps onto
    the film film_of_steps names."""
    objs, cam = _lit_scene(name)
    scene = R.Scene(objs, cam)
    n, seed, stream, first = 4097, 7, 1, 1 << 34      # (tests/test_light_film_abi.py: FILM_PATHS)
    rng = np.random.default_rng(n)
    for steps in (1, 2, 3):
        camera, st, hits = _stepped_camera(scene, n, seed, stream, first, steps)
        sampled = _some_bytes(n, rng)
        w, h = film_of_steps(steps)
        film, after, samples, photons = _expected(scene, st, hits, camera, sampled, seed, stream, w, h)
        if name == "demo":      # on the composition alone: both kinds of splat and the drop are present
            ending = (st["end"] == R.RL_PATH_END_EMITTER) & (st["value"] != 0)
            dropped = ending & (sampled != 0) & np.isin(st["object"], scene.emitters())
            assert (samples["status"] == R.RL_LIGHT_VISIBLE).sum() > 50 and dropped.sum() > 10 and (ending & ~dropped).sum() > 10
        if name == "demo" and steps == 1:
            # the film positions and wavelengths the CPU test of the bound measured its shares on are these
            drawn, _ = O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam)).render(W, H, seed, stream, first, n, threads=16)
            assert all(camera[a].tobytes() == drawn[a].tobytes() for a in "xy") and camera["ray"]["wavelength"].tobytes() == drawn["wavelength"].tobytes()
        if (w, h) == (W, H):
            k = IC.splat(w, h, photons)[1]
            few = float((k[k > 0] <= 2).mean()) if len(photons) else 1.0      # (random-6000 lights nothing after one step)
            print("%s steps %d: %d photons, %.1f %% of the non-empty components have k <= 2" % (name, steps, len(photons), 100 * few))
            assert (name != "demo" or len(photons) > 1000) and few > 0.9
        for fetch in FETCHES:
            what = "%s steps %d fetch %d" % (name, steps, fetch)
            got, got_bytes, got_samples, _ = _call_device(scene, w, h, st, hits, camera, sampled, seed, stream, fetch=fetch)
            assert_light_film(got, w, h, photons, what, film)
            assert got_bytes.tobytes() == after.tobytes(), what
            assert_same(got_samples, samples, what)
        # the host form, without a sample buffer, and with sampled = NULL
        plot = R.PlotUnit(0, w, h)
        mine = sampled.copy()
        assert plot.light_paths(scene, st, hits, camera, seed, stream, sampled=mine) is None
        assert_light_film(plot.tristimulus_buffer, w, h, photons, "%s steps %d: host form" % (name, steps), film)
        assert mine.tobytes() == after.tobytes()
        film0, none, _, photons0 = _expected(scene, st, hits, camera, None, seed, stream, w, h)
        got, got_bytes, _, _ = _call_device(scene, w, h, st, hits, camera, None, seed, stream, want_samples=False)
        assert none is None and got_bytes is None and len(photons0) >= len(photons)
        assert_light_film(got, w, h, photons0, "%s steps %d: sampled = NULL" % (name, steps), film0)


@pytest.mark.parametrize("name", SCENES)
def test_film_and_bytes_are_the_composition_after_one_two_and_three_steps(name):
    _composition(name, lambda steps: FILMS[steps % 2])


@pytest.mark.parametrize("name", SCENES)
def test_film_and_bytes_are_the_composition_on_the_cameras_own_film(name):
    """320x180: about 1.1 to 1.8 thousand photons (demo) on 57,600 pixels, so almost every component the call writes collects one
    or two terms and is held to the oracle's bits: one splat lost, doubled, misplaced or carrying the wrong field cannot hide."""
    _composition(name, lambda steps: FILMS[2])


@pytest.fixture(scope="module")
def demo_paths():
    """One reference shared by the size cases: 4033 demo paths after two steps."""
    scene = R.Scene(*_scene("demo"))
    seed, stream, first = 9, 0, 5
    return (scene, seed, stream) + _stepped_camera(scene, 4033, seed, stream, first, 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4033, "slice"])
def test_list_sizes_identity_and_permuted(demo_paths, n):
    scene, seed, stream, camera, st, hits = demo_paths
    rng = np.random.default_rng(17)
    w, h = 64, 36
    if n == "slice":
        # a list beyond the slice rule's threshold over the same 4033 states: every state once, in a shuffled order, the other
        # positions entries past the end of the state buffer
        n_list = _slice_crossing_size()
        lst = rng.integers(len(st), 1 << 32, n_list, dtype=np.uint64).astype(np.uint32)
        lst[rng.choice(n_list, len(st), replace=False)] = rng.permutation(len(st))
        cases = [(st, hits, camera, lst)]
    else:
        cases = [(st[:n], hits[:n], camera[:n], None), (st, hits, camera, rng.permutation(len(st))[:n].astype(np.uint32))]
    for s, ht, cm, lst in cases:
        sampled = _some_bytes(len(s), rng)
        film, after, samples, photons = _expected(scene, s, ht, cm, sampled, seed, stream, w, h, lst)
        got, got_bytes, got_samples, _ = _call_device(scene, w, h, s, ht, cm, sampled, seed, stream, lst)
        what = "n %s %s" % (n, "identity" if lst is None else "listed")
        assert_light_film(got, w, h, photons, what, film)
        assert got_bytes.tobytes() == after.tobytes(), what
        assert_same(got_samples, samples, what)


def test_every_splat_on_one_pixel_and_positions_that_are_not_finite(demo_paths):
    scene, seed, stream, camera, st, hits = demo_paths
    rng = np.random.default_rng(5)
    one = camera.copy()
    one["x"], one["y"] = 0.25, -0.125
    odd = camera.copy()
    odd["x"][::3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(odd["x"][::3])) % 3]
    odd["y"][1::5] = np.nan
    for what, cm in (("one pixel", one), ("not finite", odd)):
        sampled = _some_bytes(len(st), rng)
        film, after, samples, photons = _expected(scene, st, hits, cm, sampled, seed, stream, 16, 9)
        assert len(photons) > 100
        got, got_bytes, got_samples, _ = _call_device(scene, 16, 9, st, hits, cm, sampled, seed, stream)
        assert_light_film(got, 16, 9, photons, what, film)
        assert np.isfinite(got).all() and got_bytes.tobytes() == after.tobytes()
        assert_same(got_samples, samples, what)      # a state that is not splatted is sampled all the same
    assert (np.count_nonzero(_expected(scene, st, hits, one, None, seed, stream, 16, 9)[0].any(axis=1))) <= 4


# ---- 3. the drop rule's corners ----------------------------------------------------------------------------------------------

def _corner_scene():
    rows = [
        (1, 1, (0, 0, 1), (0, 0, 0), 0.0, (0.7, 0, 0)),                 # 0: the floor, a diffuse-grey plane
        (0, 0, (0, 0, 4.0), (0, 0, 0), 1.0, (6000.0, 1.0, 0)),          # 1: a sphere light: sampled
        (1, 0, (1, 0, 0), (-6.0, 0, 0), 0.0, (4500.0, 1.0, 0)),         # 2: an emissive plane: never sampled
        (1, 3, (0, -1, 0), (0, 6.0, 0), 0.0, (0.0, 0, 0)),              # 3: a mirror plane
        (0, 1, (0, 0, 0), (0, 0, 0), 40.0, (0.0, 0, 0)),                # 4: a black shell around everything
    ]
    objs = np.zeros(len(rows), R.OBJECT_DTYPE)
    for o, (sk, mk, v0, v1, f0, m) in zip(objs, rows):
        o["surface_kind"], o["material_kind"], o["v0"], o["v1"], o["m"] = sk, mk, v0, v1, m
        o["f"][0] = f0
    return objs, R.builtin_scene_desc(R.SCENE_DEMO)[1]


def _pixel_sum(film, w, h, x, y):
    """The film's sum over the (at most four) pixels a photon at x, y lands on."""
    mark = np.zeros(1, FO.PHOTON_DTYPE)
    mark["x"], mark["y"], mark["probability"], mark["wavelength"] = x, y, 1.0, 550.0
    on = _plot_of(w, h, mark).any(axis=1)
    assert 1 <= on.sum() <= 4 and not film[~on].any()
    return float(film[on].sum())


def test_the_drop_rules_corners():
    objs, cam = _corner_scene()
    scene = R.Scene(objs, cam)
    assert scene.emitters().tolist() == [1]
    n, seed, stream, w, h = 2048, 3, 1, 64, 36
    rng = np.random.default_rng(1)

    def paths(origin, direction, x, y):
        rays = np.zeros(n, R.SPECTRAL_RAY_DTYPE)
        rays["origin"], rays["direction"], rays["wavelength"] = origin, direction, 550.0
        camera = np.zeros(n, R.CAMERA_SAMPLE_DTYPE)
        camera["ray"], camera["x"], camera["y"] = rays, x, y
        return camera, scene.begin_paths(rays, 100), np.zeros(n, R.HIT_DTYPE)

    def film_of(camera, st, hits, rows, sampled):
        """The call's pixel sum; the whole film and the bytes it leaves are first held to the composition."""
        _, after, _, photons = _expected(scene, st, hits, camera, sampled, seed, stream, w, h, rows)
        plot = R.PlotUnit(0, w, h)
        plot.light_paths(scene, st, hits, camera, seed, stream, list=rows, sampled=sampled)
        assert_light_film(plot.tristimulus_buffer, w, h, photons, "corners: %d photons" % len(photons))
        assert sampled is None or sampled.tobytes() == after.tobytes()
        return _pixel_sum(plot.tristimulus_buffer, w, h, camera["x"][0], camera["y"][0])

    # from above onto the floor beside the light (a diffuse vertex, which is sampled), then wherever the bounce goes
    origin = np.zeros((n, 3), np.float32)
    origin[:, :2], origin[:, 2] = rng.uniform(2.0, 3.0, (n, 2)), 3.0
    camera, st, hits = paths(origin, (0, 0, -1), -0.5, 0.25)
    sampled = np.zeros(n, np.uint8)
    scene.step_path_list(st, seed, stream, hits=hits)
    assert (hits["object"] == 0).all() and (st["end"] == R.RL_PATH_LIVE).all()
    assert film_of(camera, st, hits, None, sampled) > 0 and sampled.all()        # the vertex splats; every vertex was sampled
    scene.step_path_list(st, seed, stream, hits=hits)
    on_sphere = np.flatnonzero((st["end"] == R.RL_PATH_END_EMITTER) & (st["object"] == 1) & (st["value"] != 0))
    on_plane = np.flatnonzero((st["end"] == R.RL_PATH_END_EMITTER) & (st["object"] == 2) & (st["value"] != 0))
    assert len(on_sphere) > 10 and len(on_plane) > 10, (len(on_sphere), len(on_plane))
    assert film_of(camera, st, hits, on_sphere, sampled.copy()) == 0             # on the sampled light after a sampled vertex: dropped
    assert film_of(camera, st, hits, on_sphere, None) > 0                        # the same with sampled = NULL: kept
    assert film_of(camera, st, hits, on_plane, sampled.copy()) > 0               # on an emitter that is never sampled: kept
    # straight from the camera onto the light
    camera, st, hits = paths((0, 0, 1.0), (0, 0, 1), 0.5, 0.25)
    sampled = np.zeros(n, np.uint8)
    scene.step_path_list(st, seed, stream, hits=hits)
    assert ((st["end"] == R.RL_PATH_END_EMITTER) & (st["object"] == 1) & (st["segments"] == 1)).all()
    assert film_of(camera, st, hits, None, sampled) > 0 and not sampled.any()
    # by way of the mirror, which is not sampled
    d = np.array([-1.5, 8.0, 0.0]) / np.hypot(1.5, 8.0)
    camera, st, hits = paths((3.0, -2.0, 4.0), d.astype(np.float32), 0.0, -0.25)
    sampled = np.zeros(n, np.uint8)
    scene.step_path_list(st, seed, stream, hits=hits)
    assert (hits["object"] == 3).all()
    assert film_of(camera, st, hits, None, sampled) == 0 and not sampled.any()   # nothing to splat at a mirror vertex, and no sample
    scene.step_path_list(st, seed, stream, hits=hits)
    on_sphere = np.flatnonzero((st["end"] == R.RL_PATH_END_EMITTER) & (st["object"] == 1) & (st["value"] != 0))
    assert len(on_sphere) > 10, len(on_sphere)
    assert film_of(camera, st, hits, on_sphere, sampled) > 0


# ---- 4. a hostile list into guarded buffers ----------------------------------------------------------------------------------

def test_hostile_list_into_guarded_prefilled_buffers():
    scene = R.Scene(*_scene("demo"))
    n, seed, stream, first, w, h = 2113, 21, 3, 1 << 35, 16, 9
    rng = np.random.default_rng(n)
    camera, st, hits = _stepped_camera(scene, n, seed, stream, first, 2)
    left_out = np.arange(n) % 3 == 1
    listed = np.flatnonzero(~left_out)
    wild = np.concatenate([[n, n + 1, 0xffffffff, 0x80000000, 0xfffffffe, n + 63, n + 64], rng.integers(n, 1 << 32, 200)]).astype(np.uint32)
    once = np.concatenate([listed.astype(np.uint32), wild])
    once = once[rng.permutation(len(once))]
    twice = np.concatenate([once, listed[:100].astype(np.uint32)])
    sampled = _some_bytes(n, rng)
    sampled[left_out] = G.FILL
    guard = lambda **kw: G.Guarded(QR.DeviceBuffer, **kw)
    film, after, samples, photons = _expected(scene, st, hits, camera, sampled, seed, stream, w, h, once)
    for fetch in FETCHES:
        for lst, exact in ((once, True), (twice, False)):
            what = "fetch %d %s" % (fetch, "distinct" if exact else "with duplicates")
            sb, hb, cb, lb = guard(initial=st), guard(initial=hits), guard(initial=camera), guard(initial=lst)
            mb, yb, fb = guard(nbytes=32 * n), guard(initial=sampled), guard(initial=np.zeros(w * h * 3, np.float32))
            plot = R.PlotUnit(0, w, h, external_xyz=fb.data_ptr())
            plot.light_paths_device(scene, sb, hb, cb, seed, stream, list=lb, n_list=len(lst), fetch=fetch, sampled=yb, samples=mb)
            plot.sync()
            got = mb.payload(what + ": samples", SAMPLE)
            got_bytes = yb.payload(what + ": sampled")
            got_film = fb.payload(what + ": film", np.float32).reshape(-1, 3)
            for b, a, word in ((sb, st, "states"), (hb, hits, "hits"), (cb, camera, "camera"), (lb, lst, "list")):
                assert b.payload(what + ": " + word).tobytes() == a.tobytes(), what + ": the " + word + " were written"
            assert (got[left_out].view(np.uint8) == G.FILL).all() and (got_bytes[left_out] == G.FILL).all(), what
            assert np.isfinite(got_film).all()
            if exact:
                G.assert_written_as(got, samples, what)
                assert got_bytes.tobytes() == after.tobytes(), what
                assert_light_film(got_film, w, h, photons, what, film)
            else:   # a state named twice: memory-safe, its own records unspecified; every other state's are as before
                rest = np.ones(n, bool)
                rest[listed[:100]] = False
                assert got[rest].tobytes() == samples[rest].tobytes() and got_bytes[rest].tobytes() == after[rest].tobytes(), what
            del plot
    # the device form's own checks: pageable host memory and misaligned buffers are refused, nothing written
    import ctypes as C
    fn, plot = R.lib.rl_plot_unit_light_paths_device, R.PlotUnit(0, w, h)
    bufs = [_Device(st), _Device(hits), _Device(camera), _Device(sampled), _Device(_prefilled(n)), _Words(once)]
    sp, hp, cp, yp, mp, lp = (C.c_void_p(d.buf.data_ptr()) for d in bufs)
    host = lambda a: a.ctypes.data_as(C.c_void_p)
    host_samples, host_bytes = _prefilled(n), sampled.copy()
    for args in ((host(st), n, lp, 8, hp, cp, yp, mp), (sp, n, host(once), 8, hp, cp, yp, mp), (sp, n, lp, 8, host(hits), cp, yp, mp),
                 (sp, n, lp, 8, hp, host(camera), yp, mp), (sp, n, lp, 8, hp, cp, host(host_bytes), mp), (sp, n, lp, 8, hp, cp, yp, host(host_samples))):
        assert fn(plot.handle, scene.handle, 0, seed, stream, *args) == -1 and b"device memory" in R.lib.rl_last_error(), args
    off = lambda p, k: C.c_void_p(p.value + k)
    for args in ((off(sp, 8), n - 1, lp, 8, hp, cp, yp, mp), (sp, n, lp, 8, hp, cp, yp, off(mp, 8)), (sp, n, lp, 8, hp, off(cp, 8), yp, mp),
                 (sp, n, off(lp, 2), 8, hp, cp, yp, mp)):
        assert fn(plot.handle, scene.handle, 0, seed, stream, *args) == -1 and b"aligned" in R.lib.rl_last_error(), args
    assert (bufs[4].get().view(np.uint8) == G.FILL).all() and bufs[3].get().tobytes() == sampled.tobytes() and not plot.tristimulus_buffer.any()
    assert (host_samples.view(np.uint8) == G.FILL).all() and host_bytes.tobytes() == sampled.tobytes()


# ---- 5. every variant on poisoned LDS ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
def test_every_variant_on_poisoned_lds(pattern):
    """The LDS of every CU filled with the pattern immediately before each call, n = 65: the assertions of the film test."""
    ran = set()
    for name in SCENES:
        objs, cam = _lit_scene(name)
        scene = R.Scene(objs, cam)
        cyl = int((objs["surface_kind"] == 4).sum() >= 40)
        n, seed, stream, first, w, h = 65, 5, 2, 12345, 16, 9
        camera, st, hits = _stepped_camera(scene, n, seed, stream, first, 2)
        sampled = _some_bytes(n, np.random.default_rng(pattern & 0xff))
        film, after, samples, photons = _expected(scene, st, hits, camera, sampled, seed, stream, w, h)
        for fetch in FETCHES:
            what = "%s pattern 0x%08X fetch %d" % (name, pattern, fetch)
            plot = R.PlotUnit(0, w, h)
            sb, hb, cb, yb, mb = _Device(st), _Device(hits), _Device(camera), _Device(sampled), _Device(_prefilled(n))
            before = R.light_film_launches()
            LP.poison_lds(pattern)
            plot.light_paths_device(scene, sb.buf, hb.buf, cb.buf, seed, stream, fetch=fetch, sampled=yb.buf, samples=mb.buf)
            launched = [a - b for a, b in zip(R.light_film_launches(), before)]
            assert sum(launched) == 1, (what, launched)
            v = launched.index(1)
            assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
            ran.add(v)
            assert_same(mb.get(), samples, what)
            assert yb.get().tobytes() == after.tobytes(), what
            assert_light_film(plot.tristimulus_buffer, w, h, photons, what, film)
    assert ran == set(range(6)), sorted(ran)


# ---- 6. the direct render ----------------------------------------------------------------------------------------------------

def _loop_of_public_calls(scene, plot, camera, seed, stream, first, max_segments, fetch=R.FETCH_LDS):
    """The film of rl_plot_unit_render_samples_direct as its contract states it, from begin_paths, step_path_list and
    PlotUnit.light_paths; returns the final states and the photons of that film in call order: per segment, the rule's photons
    (tests/_light_film_oracle.py) for the states, the `sampled` bytes and rl_scene_light_paths' samples the segment's call had."""
    n = len(camera)
    st = scene.begin_paths(np.ascontiguousarray(camera["ray"]), first)
    hits, sampled = np.zeros(n, R.HIT_DTYPE), np.zeros(n, np.uint8)
    lst, n_list = None, n
    photons = [np.zeros(0, FO.PHOTON_DTYPE)]
    for _ in range(max_segments or R.RL_PATH_MAX_SEGMENTS):
        if n_list == 0:
            break
        live = scene.step_path_list(st, seed, stream, list=lst, n_list=n_list, fetch=fetch, hits=hits)
        samples = scene.light_paths(st, hits, seed, stream, list=lst, n_list=n_list, samples=_prefilled(n))
        of_segment, after = FO.film_photons(st, samples, scene.emitters(), camera, sampled, lst, n_list)
        plot.light_paths(scene, st, hits, camera, seed, stream, list=lst, n_list=n_list, fetch=fetch, sampled=sampled)
        assert sampled.tobytes() == after.tobytes()
        photons.append(of_segment)
        lst, n_list = live, len(live)
    return st, np.concatenate(photons)


@pytest.mark.parametrize("n,max_segments,film", [(1, 0, (64, 36)), (65, 0, (64, 36)), (65, 1, (16, 9)), (65, 2, (64, 36)), (4097, 3, (64, 36)),
                                                 ((1 << 20) + 65, 2, (16, 9)), (4097, 3, (W, H))])
def test_direct_render_is_render_rays_and_the_loop_of_public_calls(n, max_segments, film):
    scene = R.Scene(*_scene("demo"))
    seed, stream, first = 4, 2, 1 << 33
    w, h = film
    camera = scene.camera_rays(W, H, seed, stream, first, n)
    camera["ray"]["wavelength"][np.arange(n) % 11 == 3] = np.nan       # paths that are never begun
    want = scene.render_spectral_rays(np.ascontiguousarray(camera["ray"]), seed, stream, first, max_segments=max_segments)
    assert n < 65 or ((want["end"] == R.RL_PATH_END_INVALID).any() and (max_segments == 0) != (want["end"] == R.RL_PATH_END_LIMIT).any())
    loop = R.PlotUnit(0, w, h)
    _, photons = _loop_of_public_calls(scene, loop, camera, seed, stream, first, max_segments)
    film_want = loop.tristimulus_buffer
    assert n < 65 or film_want.any()
    assert_light_film(film_want, w, h, photons, "the loop of public calls: film")
    if film == (W, H):
        k = IC.splat(w, h, photons)[1]
        assert len(photons) > 1000 and (k[k > 0] <= 2).mean() > 0.9
    plot = R.PlotUnit(0, w, h)
    before = R.light_film_launches()
    got = plot.render_samples_direct(scene, camera, seed, stream, first, max_segments=max_segments)
    assert sum(R.light_film_launches()) > sum(before)
    assert_same(got, want, "host form: results")
    assert_light_film(plot.tristimulus_buffer, w, h, photons, "host form: film", film_want)
    # the device form under the other fetch mode, results poisoned first
    res = np.zeros(n, R.PATH_RESULT_DTYPE)
    res["end"] = 12345
    cb, rb = QR.DeviceBuffer(camera.nbytes), QR.DeviceBuffer(res.nbytes)     # (exactly n records: the wrapper takes n from the size)
    cb.upload(np.ascontiguousarray(camera))
    rb.upload(res)
    plot = R.PlotUnit(0, w, h)
    plot.render_samples_direct_device(scene, cb, seed, stream, first, fetch=R.FETCH_GLOBAL, max_segments=max_segments, results=rb)
    rb.download(res)
    assert_same(res, want, "device form: results")
    assert_light_film(plot.tristimulus_buffer, w, h, photons, "device form: film", film_want)
    if n == 65:      # without results only the film is written
        plot = R.PlotUnit(0, w, h)
        assert plot.render_samples_direct(scene, camera, seed, stream, first, max_segments=max_segments, results=False) is None
        assert_light_film(plot.tristimulus_buffer, w, h, photons, "no results: film", film_want)


# ---- 7. it is the right estimator --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("occluder", [True, False])
def test_direct_light_with_the_drop_rule_estimates_what_the_paths_find(occluder):
    """2^16 camera paths of a small closed scene.  P: rl_scene_render_rays' value per path.  D: per path, the sum over the rounds of
    what the rule keeps (tests/_light_film_oracle.py on the samples and bytes this call writes).  Their means agree within 5
    combined standard errors; the same sum with every ending kept -- sampled lights counted twice -- does not.
    Measured on an MI355X: the rule's mean lies 1.42 (occluder) and 0.92 (none) combined standard errors from the paths' own, the
    double-counting mean 43.2 and 44.8."""
    objs, cam = closed_scene(occluder)
    scene = R.Scene(objs, cam)
    emitters = scene.emitters()
    n, seed, stream, first = 1 << 16, 17, 3, 0
    # The scene's own camera sees nothing but the black shell (every path would carry 0 and the test no power), so the camera
    # samples are the caller's own, which the film calls are for: the wavelengths and screen positions rl_scene_camera_rays draws,
    # the rays from one eye point to points spread over the lit part of the floor.
    camera = scene.camera_rays(W, H, seed, stream, first, n)
    rng = np.random.default_rng(5)
    r, a = 3.0 * np.sqrt(rng.random(n)), rng.random(n) * 2 * np.pi
    eye = np.array([4.0, -4.0, 3.0])
    d = np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1) - eye
    camera["ray"]["origin"], camera["ray"]["direction"] = eye.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.ascontiguousarray(camera["ray"])
    P = scene.render_spectral_rays(rays, seed, stream, first)["value"]
    st = scene.begin_paths(rays, first)
    hits, sampled = np.zeros(n, R.HIT_DTYPE), np.zeros(n, np.uint8)
    plot = R.PlotUnit(0, 16, 9)
    D, twice = np.zeros(n), np.zeros(n)
    lst, n_list = None, n
    splats = []
    while n_list:
        live = scene.step_path_list(st, seed, stream, list=lst, n_list=n_list, hits=hits)
        before = sampled.copy()
        samples = plot.light_paths(scene, st, hits, camera, seed, stream, list=lst, n_list=n_list, sampled=sampled, samples=np.zeros(n, SAMPLE))
        kept, after = FO.kept_values(st, samples, emitters, before, lst, n_list)
        assert after.tobytes() == sampled.tobytes()
        D += kept
        splats.append(FO.film_photons(st, samples, emitters, camera, before, lst, n_list)[0])
        twice += FO.kept_values(st, samples, emitters, before, lst, n_list, drop=False)[0]
        lst, n_list = live, len(live)
    assert (D != twice).any()
    what = "occluder %s" % occluder
    assert_means_agree(D, P, what + ": with the drop rule")
    a, b = twice.astype(np.float64), np.asarray(P, np.float64)
    se = np.sqrt(a.var(ddof=1) / n + b.var(ddof=1) / n)
    print("%s: every ending kept: mean %.6g against %.6g, %.2f standard errors apart" % (what, a.mean(), b.mean(), abs(a.mean() - b.mean()) / se))
    assert abs(a.mean() - b.mean()) > 5 * se, what + ": counting twice is not told apart from the rule"
    # the film holds the same light: it is the plot of every round's splats, which carry D between them; beside it, as before,
    # rl_plot_unit_plot_photons' film of one photon of value D per path
    splats = np.concatenate(splats)
    assert np.isclose(splats["probability"].sum(dtype=np.float64), D.sum(), rtol=1e-12, atol=0)
    photons = np.zeros(n, FO.PHOTON_DTYPE)
    photons["x"], photons["y"], photons["probability"], photons["wavelength"] = camera["x"], camera["y"], D, st["wavelength"]
    assert_light_film(plot.tristimulus_buffer, 16, 9, splats, what + ": film", _plot_of(16, 9, photons[D != 0]))
