"""Scene.render_features on the device (rl_scene_render_features): the records against the loop of public calls byte for byte
(tests/_feature_oracle.py: gpu_loop; for the built-in scene also against the CPU oracles' composition), the stats exactly, each of
the three films against its terms by rtol 2e-5 and the per-pixel splat bound, the albedo film also as the plot of its photons by the
film tests' bar (tests/_compare.py: assert_film); on all six variants, over split ranges, at full-width RNG coordinates, on poisoned
LDS and into guarded buffers, with every subset of the units, in the units' order with other work, and from the command line.  A GPU
fault ends the run: nothing here provokes one."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _feature_oracle as FO
import _guarded as G
import _lds_poison as LP
import _oracle as O
import _random_scene as RS
import _rng_width as RW
from _boundary import _ocam, _variant_of
from _compare import assert_film, assert_same
from _device_arrays import _Device
from _scenes import _lit_scene, _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
SCENES = ["demo", "many-prisms", "demo-2500", "tables-prisms", "random-6000"]   # whole scene / tables / third level, with and without CYL
W, H = 320, 180      # the camera's own film; 16x9 and 64x36 have its aspect ratio and are the contention cases for the atomics
FILMS = ((16, 9), (64, 36), (W, H))
SEED, STREAM, FIRST = 4, 2, 1 << 33      # (tests/test_feature_abi.py: PATHS -- the CPU oracle counts the kinds on these)
SIZES = (1, 63, 64, 65, 4097)
ALL = (True, True, True)


@functools.lru_cache(maxsize=None)
def _scene_of(name):
    """(the scene, its description, whether its prisms have the second bound)."""
    objs, cam = RS.random_scene(1) if name == "random-1" else _scene(name) if name == "demo" else _lit_scene(name)
    objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)
    return R.Scene(objs, cam), objs, int((objs["surface_kind"] == 4).sum() >= 40)


@functools.lru_cache(maxsize=None)
def _reference(name, n, max_segments, seed=SEED, stream=STREAM, first=FIRST):
    """The loop of public calls for n paths: made once, shared, never written."""
    scene, objs, _ = _scene_of(name)
    return FO.gpu_loop(scene, objs, W, H, seed, stream, first, n, max_segments)


@functools.lru_cache(maxsize=None)
def _cpu_reference(max_segments):
    """The CPU oracles' composition for the built-in scene's 4097 paths."""
    objs, cam = O.demo_scene_desc()
    return FO.cpu_features(objs, cam, W, H, SEED, STREAM, FIRST, SIZES[-1], max_segments, camera=_cpu_camera())


@functools.lru_cache(maxsize=None)
def _cpu_camera():
    import _direct_oracle as DO
    objs, cam = O.demo_scene_desc()
    return DO.oracle_camera_samples(objs, cam, W, H, SEED, STREAM, FIRST, SIZES[-1])


def _poisoned(n):
    return np.frombuffer(bytes([0xA5]) * (48 * n), dtype=R.FEATURE_SAMPLE_DTYPE).copy()


def assert_films(plots, w, h, records, what, given=ALL, bound_only=False):
    """Every given unit holds its film of `records` on a cleared buffer."""
    for name, plot, on in zip(FO.FILMS, plots, given):
        if on:
            FO.assert_film(plot.tristimulus_buffer, w, h, records, name, what, bound_only=bound_only)
    if given[0] and not bound_only:
        assert_film(plots[0].tristimulus_buffer, w, h, FO.albedo_photons(records), what + ": albedo as photons")


def _run(name, n, max_segments, w, h, fetch, what, n_reference=None, before_call=None, records="device", given=ALL, seed=SEED, stream=STREAM,
         first=FIRST, bound_only=False):
    """One render_features call of n paths onto cleared w x h films, held to the contract; returns (variant that ran, stats, records)."""
    scene, _, cyl = _scene_of(name)
    want_records, want_stats = _reference(name, n_reference or n, max_segments, seed, stream, first).prefix(n)
    plots = [R.PlotUnit(k, w, h) for k in range(3)]
    rb = _Device(_poisoned(n)) if records == "device" else None
    before = R.feature_launches()
    if before_call:
        before_call()
    units = dict(zip(FO.FILMS, [p if on else None for p, on in zip(plots, given)]))
    stats = scene.render_features(w, h, seed, stream, first, n, max_segments=max_segments, fetch=fetch, records=None if rb is None else rb.buf, **units)
    v = _variant_of(R.feature_launches, before)
    assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
    got = rb.get() if rb is not None else None
    if got is not None:
        assert_same(got, want_records, what + ": records")
    print("%s: variant %d, %s" % (what, v, stats))
    assert stats == want_stats, (what, stats, want_stats)
    assert_films(plots, w, h, want_records, what, given, bound_only)
    for plot, on in zip(plots, given):
        assert on or not plot.tristimulus_buffer.any(), what
    return v, stats, got


# ---- 1. the contract -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fetch", FETCHES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("max_segments", [0, 1, 2, 3])
def test_records_stats_and_films_are_the_contracts(max_segments, film, fetch):
    w, h = film
    loop = _reference("demo", SIZES[-1], max_segments)
    records, stats = loop.prefix(SIZES[-1])
    # all kinds but VOID occur (the scene is closed; tests/test_feature_abi.py has the counts), and the GPU's composition is the CPU's
    assert stats["kinds"][FO.VOID] == 0 and all(stats["kinds"][k] > 0 for k in (FO.EMITTER, FO.DIFFUSE, FO.LIMIT)), stats
    assert_same(records, _cpu_reference(max_segments).records, "the loop of public calls against the CPU oracles")
    if max_segments == 0:      # the sizes 1, 63, 64 and 65 are all DIFFUSE or EMITTER there
        assert np.isin(records["kind"][:65], (FO.EMITTER, FO.DIFFUSE)).all()
    for n in SIZES:
        what = "demo n %d max_segments %d %dx%d fetch %d" % (n, max_segments, w, h, fetch)
        _run("demo", n, max_segments, w, h, fetch, what, n_reference=SIZES[-1])


@pytest.mark.parametrize("fetch", FETCHES)
def test_all_four_kinds_on_the_open_scene(fetch):
    v, stats, records = _run("random-1", SIZES[-1], 3, 64, 36, fetch, "random_scene(1) fetch %d" % fetch)
    assert all(k > 0 for k in stats["kinds"]), stats
    void = records[records["kind"] == FO.VOID]
    assert (void["object"] == R.RL_OBJECT_NONE).all() and not void["normal"].any() and not void["albedo"].any()
    assert (void["depth"][void["segments"] == 1] == 0).all()


# ---- 2. all six variants -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ran():
    return {}


def _variants_of(name, ran):
    if name not in ran:
        ran[name] = [_run(name, 2113, 3, 64, 36, fetch, "%s fetch %d" % (name, fetch))[0] for fetch in FETCHES]
    return ran[name]


@pytest.mark.parametrize("name", SCENES)
def test_every_scene_runs_on_the_variant_meant(name, ran):
    scene, _, cyl = _scene_of(name)
    camera = scene.camera_rays(W, H, SEED, STREAM, FIRST, 2113)
    rays = np.ascontiguousarray(camera["ray"])
    for fetch, v in zip(FETCHES, _variants_of(name, ran)):
        before = R.path_launches()      # the variant the path kernel takes for this scene and fetch mode is the one meant
        scene.render_spectral_rays(rays, SEED, STREAM, FIRST, fetch=fetch, max_segments=3)
        assert v == _variant_of(R.path_launches, before), (name, fetch, v)


def test_the_scenes_cover_all_six_variants(ran):
    assert {v for name in SCENES for v in _variants_of(name, ran)} == set(range(6)), ran


# ---- 3. splits -----------------------------------------------------------------------------------------------------------------

def test_a_range_in_one_call_and_in_two():
    scene, _, _ = _scene_of("demo")
    n, cut, ms, (w, h) = SIZES[-1], 1000, 3, (64, 36)      # 1000 is no multiple of 64
    loop = _reference("demo", n, ms)
    whole, parts = [R.PlotUnit(k, w, h) for k in range(3)], [R.PlotUnit(k, w, h) for k in range(3)]
    rw, front, back = _Device(_poisoned(n)), _Device(_poisoned(cut)), _Device(_poisoned(n - cut))
    stats = scene.render_features(w, h, SEED, STREAM, FIRST, n, max_segments=ms, records=rw.buf, **dict(zip(FO.FILMS, whole)))
    a = scene.render_features(w, h, SEED, STREAM, FIRST, cut, max_segments=ms, records=front.buf, **dict(zip(FO.FILMS, parts)))
    b = scene.render_features(w, h, SEED, STREAM, FIRST + cut, n - cut, max_segments=ms, records=back.buf, **dict(zip(FO.FILMS, parts)))
    assert_same(rw.get(), loop.records, "one call")
    assert_same(np.concatenate([front.get(), back.get()]), loop.records, "two calls")
    assert a == loop.span(0, cut) and b == loop.span(cut, n) and stats == loop.prefix(n)[1]
    assert FO.add_stats(a, b) == stats, (a, b, stats)
    assert_films(whole, w, h, loop.records, "one call")
    assert_films(parts, w, h, loop.records, "two calls into the same units")


def test_one_call_beyond_2_to_the_20_paths():
    """2^20 + 65 paths, max_segments 2, on 16x9: past the slice rule's threshold and the staging chunk of the host calls the loop is
    made of.  Records and stats exactly; a component of these films has up to 35,000 terms, so they are held to the per-pixel
    bound against the exact sum alone (tests/_feature_oracle.py: assert_film).  Measured on an MI355X: the largest gap to the exact
    sum is 2.2e-5 of the film's maximum on the albedo film, 3.9e-6 on the normal film and 7.1e-6 on the aux film, no component
    outside the bound."""
    n, ms, (w, h) = (1 << 20) + 65, 2, (16, 9)
    _run("demo", n, ms, w, h, R.FETCH_LDS, "2^20 + 65 paths", bound_only=True)


# ---- 4. full-width RNG coordinates ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_full_width_seeds_streams_and_path_ranges(case):
    what = "%s: %s" % (case.id, case.why)
    _run("demo", RW.N_QUERY, 2, 64, 36, R.FETCH_LDS, what, seed=case.seed, stream=case.stream, first=case.first)


# ---- 5. dirty state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
def test_every_variant_on_poisoned_lds(pattern):
    """The LDS of every CU filled with the pattern immediately before each call (the kernel keeps its counters and four values of
    every path in the wave's scratch): the assertions of the contract test."""
    seen = set()
    for name in SCENES:
        for fetch in FETCHES:
            what = "%s pattern 0x%08X fetch %d" % (name, pattern, fetch)
            seen.add(_run(name, 65, 3, 16, 9, fetch, what, n_reference=2113, before_call=lambda: LP.poison_lds(pattern))[0])
    assert seen == set(range(6)), sorted(seen)


def test_records_into_a_guarded_buffer():
    scene, _, _ = _scene_of("demo")
    n, ms = 2113, 3
    want, want_stats = _reference("demo", n, ms).prefix(n)
    for fetch in FETCHES:
        what = "guarded, fetch %d" % fetch
        rb = G.device_guarded(nbytes=48 * n)      # prefilled 0xAA
        stats = scene.render_features(16, 9, SEED, STREAM, FIRST, n, max_segments=ms, fetch=fetch, records=rb)      # records alone, no unit
        G.assert_written_as(rb.payload(what, R.FEATURE_SAMPLE_DTYPE), want, what)      # guards intact, all 48 bytes of every record written
        assert stats == want_stats
    # pageable host memory and a misaligned buffer are refused, nothing written
    plots, host = [R.PlotUnit(k, 16, 9) for k in range(3)], _poisoned(n)
    fn = R.lib.rl_scene_render_features
    handles = [p.handle for p in plots]
    assert fn(scene.handle, 0, 16, 9, SEED, STREAM, FIRST, n, ms, *handles, host.ctypes.data_as(C.c_void_p), None) == -1
    assert b"device memory" in R.lib.rl_last_error()
    rb = _Device(_poisoned(n + 1))
    assert fn(scene.handle, 0, 16, 9, SEED, STREAM, FIRST, n, ms, *handles, C.c_void_p(rb.buf.data_ptr() + 8), None) == -1
    assert b"aligned" in R.lib.rl_last_error()
    assert host.tobytes() == _poisoned(n).tobytes() and rb.get().tobytes() == _poisoned(n + 1).tobytes()
    assert not any(p.tristimulus_buffer.any() for p in plots)


# ---- 6. the units --------------------------------------------------------------------------------------------------------------

def test_every_subset_of_the_units_gives_the_same_films_records_and_stats():
    n, ms, (w, h) = 2113, 3, (64, 36)
    outcomes = []
    for given in itertools.product((False, True), repeat=3):
        v, stats, records = _run("demo", n, ms, w, h, R.FETCH_LDS, "units %s" % (given,), given=given)
        outcomes.append((stats, records.tobytes()))
    assert all(o == outcomes[0] for o in outcomes)
    _run("demo", n, ms, w, h, R.FETCH_LDS, "no records", records=None)


def test_units_of_another_size_and_the_same_unit_twice_are_refused():
    scene, _, _ = _scene_of("demo")
    n, ms = 65, 3
    a, b, other = R.PlotUnit(0, 16, 9), R.PlotUnit(1, 16, 9), R.PlotUnit(2, 64, 36)
    rb = _Device(_poisoned(n))
    for units in (dict(albedo=a, normal=b, aux=other), dict(albedo=other), dict(aux=other, normal=a)):
        with pytest.raises(R.RlError) as e:
            scene.render_features(16, 9, SEED, STREAM, FIRST, n, max_segments=ms, records=rb.buf, **units)
        assert e.value.code == -5, e.value      # RL_E_STATE
    for units in (dict(albedo=a, normal=a), dict(albedo=a, aux=a), dict(normal=b, aux=b), dict(albedo=a, normal=a, aux=a)):
        with pytest.raises(R.RlError) as e:
            scene.render_features(16, 9, SEED, STREAM, FIRST, n, max_segments=ms, records=rb.buf, **units)
        assert e.value.code == -1 and "distinct" in str(e.value), e.value      # RL_E_INVALID
    assert rb.get().tobytes() == _poisoned(n).tobytes()
    assert not a.tristimulus_buffer.any() and not b.tristimulus_buffer.any() and not other.tristimulus_buffer.any()


# ---- 7. ordering ---------------------------------------------------------------------------------------------------------------

def test_the_call_ends_a_begun_fused_render_accumulates_and_is_seen_by_the_gather():
    objs, cam = _scene("demo")
    scene, _, _ = _scene_of("demo")
    n, ms = SIZES[-1], 3
    records, want_stats = _reference("demo", n, ms).prefix(n)
    photons = FO.albedo_photons(records)
    n_fused = 1 << 16
    fused, _ = O.Scene(np.ascontiguousarray(objs).view(O.OBJECT_DTYPE), _ocam(cam)).render(W, H, 5, 0, 0, n_fused, threads=16)
    t, plots = R.TraceUnit(0, W, H, n_photons=n_fused), [R.PlotUnit(k, W, H) for k in range(3)]
    t.render_fused_begin(scene, plots[0], n_fused, seed=5, stream=0, first_path_index=0)
    stats = scene.render_features(W, H, SEED, STREAM, FIRST, n, max_segments=ms, **dict(zip(FO.FILMS, plots)))      # ends the begun render first
    assert stats == want_stats
    assert_film(plots[0].tristimulus_buffer, W, H, np.concatenate([fused, photons]), "fused_begin + render_features")
    assert_films(plots, W, H, records, "beside a fused render", given=(False, True, True))
    # a fused render begun into a unit that is not the first given one ends first as well
    plots = [R.PlotUnit(k, W, H) for k in range(3)]
    t.render_fused_begin(scene, plots[2], n_fused, seed=5, stream=0, first_path_index=0)
    scene.render_features(W, H, SEED, STREAM, FIRST, n, max_segments=ms, **dict(zip(FO.FILMS, plots)))
    assert_films(plots, W, H, records, "a fused render begun into the aux unit", given=(True, True, False))
    assert plots[2].tristimulus_buffer.any()
    # two calls accumulate
    plots = [R.PlotUnit(k, W, H) for k in range(3)]
    scene.render_features(W, H, SEED, STREAM, FIRST, n, max_segments=ms, **dict(zip(FO.FILMS, plots)))
    scene.render_features(W, H, SEED, STREAM, FIRST, n, max_segments=ms, fetch=R.FETCH_GLOBAL, **dict(zip(FO.FILMS, plots)))
    assert_films(plots, W, H, np.concatenate([records, records]), "two calls")
    # the gather straight after the call sees each film (and clears the unit)
    plots, gathers = [R.PlotUnit(k, W, H) for k in range(3)], [R.GatherUnit(W, H) for _ in range(3)]
    scene.render_features(W, H, SEED, STREAM, FIRST, n, max_segments=ms, **dict(zip(FO.FILMS, plots)))
    for name, p, g in zip(FO.FILMS, plots, gathers):
        g.accumulate(p)
        FO.assert_film(g.tristimulus_buffer.astype(np.float32), W, H, records, name, "the gather after the call")
        assert not p.tristimulus_buffer.any()


# ---- 8. the command line -------------------------------------------------------------------------------------------------------

def test_the_command_line_writes_the_guides_of_two_render_features_calls(tmp_path):
    w, h, batch, seed = 64, 36, 4096, 3
    out, prefix = tmp_path / "out.ppm", tmp_path / "guides"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "robigo_luculenta_amd", "--direct", "--features", str(prefix), "--width", str(w), "--height", str(h),
                          "--batches", "2", "--photons-per-batch", str(batch), "--seed", str(seed), "--output", str(out), "--quiet"],
                         cwd=str(tmp_path), env=env, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    told = run.stdout.decode()
    got = np.load(str(prefix) + ".npz")
    assert sorted(got.files) == ["albedo_xyz", "aux", "normal"]
    scene = R.Scene.builtin(R.SCENE_DEMO)
    objs = np.ascontiguousarray(_scene("demo")[0]).view(R.OBJECT_DTYPE)
    plots, gathers = [R.PlotUnit(k, w, h) for k in range(3)], [R.GatherUnit(w, h) for _ in range(3)]
    total = {"paths": 0, "segments": 0, "kinds": [0, 0, 0, 0]}
    for b in range(2):
        total = FO.add_stats(total, scene.render_features(w, h, seed, 0, b * batch, batch, **dict(zip(FO.FILMS, plots))))
        for p, g in zip(plots, gathers):
            g.accumulate(p)
    records = FO.gpu_loop(scene, objs, w, h, seed, 0, 0, 2 * batch, 0).records
    assert FO.stats_of(records) == total
    for key, name, g in zip(("albedo_xyz", "normal", "aux"), FO.FILMS, gathers):
        film = got[key]
        assert film.dtype == np.float32 and film.shape == (h, w, 3)
        FO.assert_film(film.reshape(-1, 3), w, h, records, name, "the command line's " + key)
        FO.assert_film(g.tristimulus_buffer.astype(np.float32), w, h, records, name, "two calls gathered: " + key)
    assert ("features: paths %d, segments %d, void %d, emitter %d, diffuse %d, limit %d" % ((total["paths"], total["segments"]) + tuple(total["kinds"]))) in told, told
    for name in ("-normal.png", "-depth.png"):
        blob = open(str(prefix) + name, "rb").read()
        assert blob[:8] == b"\x89PNG\r\n\x1a\n" and len(blob) > 100
    # without --direct the image comes from the App's worker pool and the guides are those of the same paths
    plain = tmp_path / "plain"
    run = subprocess.run([sys.executable, "-m", "robigo_luculenta_amd", "--features", str(plain), "--max-segments", "64", "--width", str(w), "--height", str(h),
                          "--batches", "2", "--photons-per-batch", str(batch), "--seed", str(seed), "--output", str(tmp_path / "plain.ppm"), "--quiet"],
                         cwd=str(tmp_path), env=env, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert (tmp_path / "plain.ppm").exists()
    again = np.load(str(plain) + ".npz")
    for key, name in zip(("albedo_xyz", "normal", "aux"), FO.FILMS):
        FO.assert_film(again[key].reshape(-1, 3), w, h, records, name, "without --direct: " + key)
