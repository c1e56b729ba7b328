"""PlotUnit.render_direct on the device (rl_plot_unit_render_direct): the results against rl_scene_render_rays byte for byte, the
stats against the counts of the loop of public calls (tests/_direct_oracle.py: gpu_loop) exactly, the film against the CPU oracle's
plot of that loop's photons by the film tests' bar (tests/_compare.py: assert_film) with rl_plot_unit_render_samples_direct's film
of the same samples beside it; on all six variants, over split ranges, at full-width RNG coordinates, on poisoned LDS and into
guarded buffers, in the unit's order with other work, and from the command line.  A GPU fault ends the run: nothing here provokes
one."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _direct_oracle as DO
import _guarded as G
import _image_cases as IC
import _lds_poison as LP
import _oracle as O
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
SEED, STREAM, FIRST = 4, 2, 1 << 33      # (tests/test_direct_abi.py: PATHS -- the CPU oracle finds every branch on these)
SIZES = (1, 63, 64, 65, 4097)


@functools.lru_cache(maxsize=None)
def _scene_of(name):
    objs, cam = _scene(name) if name == "demo" else _lit_scene(name)
    return R.Scene(objs, cam), int((np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)["surface_kind"] == 4).sum() >= 40)


def _reference(name, n, max_segments, seed=SEED, stream=STREAM, first=FIRST):
    """(camera samples, the loop of public calls, rl_scene_render_rays' results) of n paths: made once, shared, never written."""
    return _reference_of(name, n, max_segments, seed, stream, first)


@functools.lru_cache(maxsize=None)
def _reference_of(name, n, max_segments, seed, stream, first):
    scene, _ = _scene_of(name)
    camera, loop = DO.gpu_loop(scene, W, H, seed, stream, first, n, max_segments)
    want = scene.render_spectral_rays(np.ascontiguousarray(camera["ray"]), seed, stream, first, max_segments=max_segments)
    assert_same(loop.results.view(R.PATH_RESULT_DTYPE), want, "the loop's final states against render_rays")
    return camera, loop, want


@functools.lru_cache(maxsize=None)
def _samples_direct_film(name, n, n_reference, max_segments, w, h, seed=SEED, stream=STREAM, first=FIRST):
    """rl_plot_unit_render_samples_direct's film of the first n of the reference's samples."""
    scene, _ = _scene_of(name)
    camera = _reference(name, n_reference, max_segments, seed, stream, first)[0]
    plot = R.PlotUnit(0, w, h)
    assert plot.render_samples_direct(scene, camera[:n], seed, stream, first, max_segments=max_segments, results=False) is None
    return plot.tristimulus_buffer


def _poisoned(n):
    res = np.zeros(n, R.PATH_RESULT_DTYPE)
    res["end"], res["segments"], res["value"] = 12345, 0xAAAAAAAA, np.nan
    return res


def assert_direct_film(got, w, h, photons, what, beside):
    """The film tests' bar against the CPU oracle's plot of `photons` (rtol 2e-5 plus the per-pixel splat bound, the oracle's bits
    where a component has at most two terms), and beside it the tolerance for another order of the float atomics against a film
    the device made of the same samples by other calls."""
    assert_film(got, w, h, photons, what)
    scale = float(np.abs(beside).max())
    print("%s: max |got - render_samples_direct's film| %.3e, image max %.3e" % (what, float(np.abs(got - beside).max()), scale))
    assert np.allclose(got, beside, rtol=2e-5, atol=1e-6 * scale), what


def _run(name, n, max_segments, w, h, fetch, what, n_reference=None, before_call=None, results="device", seed=SEED, stream=STREAM, first=FIRST):
    """One render_direct call of n paths onto a cleared w x h film, held to the three checks; returns the variant that ran."""
    scene, cyl = _scene_of(name)
    camera, loop, want = _reference(name, n_reference or n, max_segments, seed, stream, first)
    want_results, photons, want_stats = loop.prefix(n)
    plot = R.PlotUnit(0, w, h)
    rb = _Device(_poisoned(n)) if results == "device" else None
    before = R.direct_launches()
    if before_call:
        before_call()
    stats = plot.render_direct(scene, seed, stream, first, n, max_segments=max_segments, fetch=fetch, results=None if rb is None else rb.buf)
    v = _variant_of(R.direct_launches, before)
    assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
    if rb is not None:
        assert_same(rb.get(), want[:n], what + ": results")
    print("%s: variant %d, %s" % (what, v, stats))
    assert stats == want_stats, (what, stats, want_stats)
    assert_direct_film(plot.tristimulus_buffer, w, h, photons, what, _samples_direct_film(name, n, n_reference or n, max_segments, w, h, seed, stream, first))
    return v


# ---- 1. the contract -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fetch", FETCHES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("max_segments", [0, 1, 2, 3])
def test_results_stats_and_film_are_the_contracts(max_segments, film, fetch):
    w, h = film
    camera, loop, want = _reference("demo", SIZES[-1], max_segments)
    # the inputs reach the branches (the CPU oracle says so for 0 and 3: tests/test_direct_abi.py)
    stats = loop.prefix(SIZES[-1])[2]
    # (with one segment no vertex comes before an ending: nothing can be dropped)
    assert all(stats[f] > 0 for f in DO.STATS if max_segments != 1 or f != "endings_dropped") and len(loop.statuses) == 4, (stats, loop.statuses)
    assert (want["end"] == R.RL_PATH_END_LIMIT).any() == (max_segments != 0)
    if film == (W, H):
        k = IC.splat(w, h, loop.photons)[1]
        few = float((k[k > 0] <= 2).mean())
        print("max_segments %d: %d photons, %.1f %% of the non-empty components have k <= 2" % (max_segments, len(loop.photons), 100 * few))
        assert len(loop.photons) > 1000 and few > 0.8      # most components are held to the oracle's bits (88 % at max_segments 0, more below)
    for n in SIZES:
        what = "demo n %d max_segments %d %dx%d fetch %d" % (n, max_segments, w, h, fetch)
        _run("demo", n, max_segments, w, h, fetch, what, n_reference=SIZES[-1])
    # with results = None only the film and the stats are written
    _run("demo", 65, max_segments, w, h, fetch, "no results", n_reference=SIZES[-1], results=None)


# ---- 2. all six variants -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ran():
    return {}


def _variants_of(name, ran):
    if name not in ran:
        ran[name] = [_run(name, 2113, 3, 64, 36, fetch, "%s fetch %d" % (name, fetch)) for fetch in FETCHES]
    return ran[name]


@pytest.mark.parametrize("name", SCENES)
def test_every_scene_runs_on_the_variant_meant(name, ran):
    scene, cyl = _scene_of(name)
    rays = np.ascontiguousarray(_reference(name, 2113, 3)[0]["ray"])
    for fetch, v in zip(FETCHES, _variants_of(name, ran)):
        before = R.path_launches()      # the variant the path kernel takes for this scene and fetch mode is the one meant
        scene.render_spectral_rays(rays, SEED, STREAM, FIRST, fetch=fetch, max_segments=3)
        assert v == _variant_of(R.path_launches, before), (name, fetch, v)


def test_the_scenes_cover_all_six_variants(ran):
    assert {v for name in SCENES for v in _variants_of(name, ran)} == set(range(6)), ran


# ---- 3. splits -----------------------------------------------------------------------------------------------------------------

def test_a_range_in_one_call_and_in_two():
    scene, _ = _scene_of("demo")
    n, cut, ms, (w, h) = SIZES[-1], 1000, 3, (64, 36)      # 1000 is no multiple of 64
    camera, loop, want = _reference("demo", n, ms)
    whole, parts = R.PlotUnit(0, w, h), R.PlotUnit(0, w, h)
    rw = _Device(_poisoned(n))
    stats = whole.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms, results=rw.buf)
    front = _Device(_poisoned(cut))
    back = _Device(_poisoned(n - cut))
    a = parts.render_direct(scene, SEED, STREAM, FIRST, cut, max_segments=ms, results=front.buf)
    b = parts.render_direct(scene, SEED, STREAM, FIRST + cut, n - cut, max_segments=ms, results=back.buf)
    assert_same(rw.get(), want, "one call")
    assert_same(np.concatenate([front.get(), back.get()]), want, "two calls")
    assert a == loop.span(0, cut) and b == loop.span(cut, n) and stats == loop.prefix(n)[2]
    assert all(a[f] + b[f] == stats[f] for f in DO.STATS), (a, b, stats)
    assert_direct_film(parts.tristimulus_buffer, w, h, loop.photons, "two calls into one unit", whole.tristimulus_buffer)
    assert_film(whole.tristimulus_buffer, w, h, loop.photons, "one call")


def test_one_call_beyond_the_staging_chunk_of_the_loop():
    """2^20 + 65 paths, max_segments 2, on 16x9: past render_samples_direct's chunk of 2^20 samples and the slice rule's threshold."""
    n, ms, (w, h) = (1 << 20) + 65, 2, (16, 9)
    _run("demo", n, ms, w, h, R.FETCH_LDS, "2^20 + 65 paths")


# ---- 4. full-width RNG coordinates ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_full_width_seeds_streams_and_path_ranges(case):
    what = "%s: %s" % (case.id, case.why)
    _run("demo", RW.N_QUERY, 2, 64, 36, R.FETCH_LDS, what, seed=case.seed, stream=case.stream, first=case.first)


# ---- 5. dirty state ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
def test_every_variant_on_poisoned_lds(pattern):
    """The LDS of every CU filled with the pattern immediately before each call (the kernel keeps its counters and three values of
    every path in the wave's scratch): the assertions of the contract test."""
    seen = set()
    for name in SCENES:
        for fetch in FETCHES:
            what = "%s pattern 0x%08X fetch %d" % (name, pattern, fetch)
            seen.add(_run(name, 65, 3, 16, 9, fetch, what, n_reference=2113, before_call=lambda: LP.poison_lds(pattern)))
    assert seen == set(range(6)), sorted(seen)


def test_results_into_a_guarded_buffer():
    scene, _ = _scene_of("demo")
    n, ms = 2113, 3
    camera, loop, want = _reference("demo", n, ms)
    for fetch in FETCHES:
        what = "guarded, fetch %d" % fetch
        rb = G.device_guarded(nbytes=16 * n)      # prefilled 0xAA
        plot = R.PlotUnit(0, 16, 9)
        stats = plot.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms, fetch=fetch, results=rb)
        G.assert_written_as(rb.payload(what, R.PATH_RESULT_DTYPE), want, what)      # guards intact, every record written
        assert stats == loop.prefix(n)[2]
    # pageable host memory and a misaligned buffer are refused, nothing written
    import ctypes as C
    plot, host = R.PlotUnit(0, 16, 9), _poisoned(n)
    fn = R.lib.rl_plot_unit_render_direct
    assert fn(plot.handle, scene.handle, 0, SEED, STREAM, FIRST, n, ms, host.ctypes.data_as(C.c_void_p), None) == -1 and b"device memory" in R.lib.rl_last_error()
    rb = _Device(_poisoned(n + 1))
    assert fn(plot.handle, scene.handle, 0, SEED, STREAM, FIRST, n, ms, C.c_void_p(rb.buf.data_ptr() + 8), None) == -1 and b"aligned" in R.lib.rl_last_error()
    assert host.tobytes() == _poisoned(n).tobytes() and rb.get().tobytes() == _poisoned(n + 1).tobytes() and not plot.tristimulus_buffer.any()


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------

def test_the_call_ends_a_begun_fused_render_accumulates_and_is_seen_by_the_gather():
    objs, cam = _scene("demo")
    scene, _ = _scene_of("demo")
    n, ms = SIZES[-1], 3
    camera, loop, want = _reference("demo", n, ms)
    n_fused = 1 << 16
    fused, _ = O.Scene(np.ascontiguousarray(objs).view(O.OBJECT_DTYPE), _ocam(cam)).render(W, H, 5, 0, 0, n_fused, threads=16)
    t, p = R.TraceUnit(0, W, H, n_photons=n_fused), R.PlotUnit(0, W, H)
    t.render_fused_begin(scene, p, n_fused, seed=5, stream=0, first_path_index=0)
    stats = p.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms)      # ends the begun render first
    assert stats == loop.prefix(n)[2]
    assert_film(p.tristimulus_buffer, W, H, np.concatenate([fused, loop.photons]), "fused_begin + render_direct")
    # two calls accumulate
    p = R.PlotUnit(0, W, H)
    p.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms)
    p.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms, fetch=R.FETCH_GLOBAL)
    assert_film(p.tristimulus_buffer, W, H, np.concatenate([loop.photons, loop.photons]), "two calls")
    # the gather straight after the call sees it (and clears the unit)
    p, g = R.PlotUnit(0, W, H), R.GatherUnit(W, H)
    p.render_direct(scene, SEED, STREAM, FIRST, n, max_segments=ms)
    g.accumulate(p)
    assert_film(g.tristimulus_buffer.astype(np.float32), W, H, loop.photons, "the gather after the call")
    assert not p.tristimulus_buffer.any()


# ---- 7. the command line -------------------------------------------------------------------------------------------------------

def test_the_command_line_renders_the_image_of_two_render_direct_calls(tmp_path):
    w, h, batch, seed = 64, 36, 4096, 3
    out = tmp_path / "out.ppm"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "robigo_luculenta_amd", "--direct", "--width", str(w), "--height", str(h), "--batches", "2",
                          "--photons-per-batch", str(batch), "--seed", str(seed), "--output", str(out), "--quiet"],
                         cwd=str(tmp_path), env=env, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    told = run.stdout.decode()
    blob = out.read_bytes()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert blob.startswith(head) and len(blob) == len(head) + w * h * 3
    got = np.frombuffer(blob[len(head):], np.uint8).reshape(-1, 3)
    scene = R.Scene.builtin(R.SCENE_DEMO)
    plot, gather, total = R.PlotUnit(0, w, h), R.GatherUnit(w, h), dict.fromkeys(DO.STATS, 0)
    for b in range(2):
        for k, v in plot.render_direct(scene, seed, 0, b * batch, batch).items():
            total[k] += v
        gather.accumulate(plot)
    tm = R.TonemapUnit(w, h)
    tm.tonemap(gather)
    want = tm.rgb_buffer
    print("%d of %d bytes differ" % (int((got != want).sum()), got.size))
    assert want.any() and np.abs(got.astype(np.float64) / 255.0 - want.astype(np.float64) / 255.0).max() <= 1e-3
    assert ("direct light: " + ", ".join("%s %d" % kv for kv in total.items())) in told, told
