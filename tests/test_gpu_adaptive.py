"""Adaptive sampling on the device (rl_adaptive_unit_*, rl_plot_unit_render_adaptive): the plan read back against the numpy rule,
the samples against the host compile of the same header bit for bit, the film against the f64 sum of its weighted photons within
the per-pixel splat bound, unit lifetime, and the error model under re-planned batches.  A GPU fault ends the run: nothing here
provokes one."""
import functools
import json
import os

import numpy as np
import pytest

import _adaptive_cases as AC
import _adaptive_oracle as AO
import _compare as CMP
import _guarded as G
import _lds_poison as LP
import _path_oracle as PO
import _rng_width as RW
import _scenes as SC

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5
SHARE = AC.UNIFORM_SHARE
PLANS = ("one_hot_partial", "random")
FILMS = AC.SMALL_FILMS
FILM_IDS = ["%dx%d" % f for f in FILMS]
CARRY = RW.BY_ID["carry-mid-wave"]


@functools.lru_cache(maxsize=None)
def _desc(name):
    return SC._scene(name)


@functools.lru_cache(maxsize=None)
def _scene(name):
    objs, cam = _desc(name)
    return R.Scene(objs, cam)


@functools.lru_cache(maxsize=None)
def _host_scene(name):
    objs, cam = _desc(name)
    return AO.HostScene(np.ascontiguousarray(objs), cam)


def _planned(w, h, plan, n):
    """(unit, counts, weights): a unit that holds the plan, which is the numpy rule's bit for bit when read back."""
    g = AC.importance(plan, w, h)
    unit = R.AdaptiveUnit(w, h)
    stats = unit.plan(g, SHARE, n)
    status, counts, weights, total = AO.plan(w, h, g, SHARE, n)
    assert status == AO.PLAN_OK
    got_counts, got_weights = unit.download_plan()
    assert got_counts.reshape(-1).tobytes() == counts.tobytes() and got_weights.reshape(-1).tobytes() == weights.tobytes()
    assert (stats["n_paths"], stats["min_count"], stats["max_count"]) == (n, counts.min(), counts.max())
    assert stats["importance_sum"] == total and stats["min_weight"] == weights.min() and stats["max_weight"] == weights.max()
    return unit, counts, weights


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.IMPORTANCE)
@pytest.mark.parametrize("film", AC.FILMS, ids=lambda f: "%dx%d" % f)
def test_the_plan_on_the_device_is_the_numpy_rule(film, name):
    w, h = film
    g = AC.importance(name, w, h)
    n_min = AC.smallest_n(w, h, g, SHARE)
    unit, counts, _ = _planned(w, h, name, n_min)
    if n_min > 1:        # one below is refused, and the previous plan stays
        with pytest.raises(R.RlError) as e:
            unit.plan(g, SHARE, n_min - 1)
        assert e.value.code == RL_E_INVALID and "no sample" in str(e.value)
        assert unit.download_plan()[0].reshape(-1).tobytes() == counts.tobytes()
    over = AC.overflowing(w, h)
    if over is not None:
        with pytest.raises(R.RlError) as e:
            unit.plan(over, SHARE, 1 << 20)
        assert e.value.code == RL_E_INVALID and "overflows" in str(e.value)
        assert unit.download_plan()[0].reshape(-1).tobytes() == counts.tobytes()
    unit.plan(g, SHARE, AC.N_MAX)
    assert unit.download_plan()[0].reshape(-1).tobytes() == AO.plan(w, h, g, SHARE, AC.N_MAX)[1].tobytes()


# ---- the samples ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("film", FILMS, ids=FILM_IDS)
def test_samples_are_the_host_compiles_bit_for_bit(film, plan):
    w, h = film
    scene, host = _scene("demo"), _host_scene("demo")
    g = AC.importance(plan, w, h)
    n_min = AC.smallest_n(w, h, g, SHARE)
    for n, seed, stream, first in ((n_min, 7, 1, 0), (1 << 18, CARRY.seed, CARRY.stream, CARRY.first - (1 << 17)),
                                   (70001, RW.BY_ID["top"].seed, RW.BY_ID["top"].stream, (1 << 64) - 2 - 70001)):
        unit, counts, weights = _planned(w, h, plan, n)
        want = host.samples(w, h, counts, weights, seed, stream, first, 0, n)
        got = unit.samples(scene, seed, stream, first, 0, n)
        CMP.assert_same(got, want, "%s %dx%d n=%d" % (plan, w, h, n))
        assert (np.bincount(got["reserved0"], minlength=len(counts)) == counts).all()
        # a window that starts in the middle of a tile, host form and _device form into a guarded, prefilled buffer
        lo = int(AO.offsets(counts)[len(counts) // 2]) + int(counts[len(counts) // 2]) // 2
        k = min(n - lo, 4097)
        CMP.assert_same(unit.samples(scene, seed, stream, first, lo, k), want[lo:lo + k], "window")
        out = G.device_guarded(k * 48)
        unit.samples_device(scene, seed, stream, first, lo, out, n=k)
        G.assert_written_as(out.payload("samples_device", R.CAMERA_SAMPLE_DTYPE), want[lo:lo + k], "samples_device")
        assert unit.samples(scene, seed, stream, first, n, 0).shape == (0,)


def test_every_argument_failure_on_a_live_unit():
    scene = _scene("demo")
    unit = R.AdaptiveUnit(64, 36)
    with pytest.raises(R.RlError) as e:
        unit.samples(scene, 1, 0, 0, 0, 5)
    assert e.value.code == RL_E_STATE
    with pytest.raises(R.RlError) as e:
        unit.download_plan()
    assert e.value.code == RL_E_STATE
    plot = R.PlotUnit(0, 64, 36)
    with pytest.raises(R.RlError) as e:
        plot.render_adaptive(unit, scene, 1, 0)
    assert e.value.code == RL_E_STATE
    unit.plan(None, 1.0, 1000)
    for first_sample, n in ((990, 11), (1001, 0)):
        with pytest.raises(R.RlError) as e:
            unit.samples(scene, 1, 0, 0, first_sample, n)
        assert e.value.code == RL_E_INVALID and "past the end" in str(e.value)
    with pytest.raises(R.RlError) as e:
        R.PlotUnit(0, 33, 17).render_adaptive(unit, scene, 1, 0)
    assert e.value.code == RL_E_STATE and "does not match" in str(e.value)
    pageable = np.zeros(4 * 48 + 64, np.uint8)
    with pytest.raises(R.RlError) as e:      # pageable host memory is refused by the _device form
        _lib.check(_lib.lib.rl_adaptive_unit_samples_device(unit.handle, scene.handle, 1, 0, 0, 0, 4, pageable.ctypes.data // 16 * 16 + 16))
    assert e.value.code == RL_E_INVALID and "not device memory" in str(e.value)
    assert plot.tristimulus_buffer.tobytes() == bytes(64 * 36 * 12)


# ---- the film ---------------------------------------------------------------------------------------------------------------------

def _weighted_photons(scene, samples, seed, stream, first, fetch):
    """What the film must hold the sum of: per sample {x, y, f32(value * w_t), wavelength}, the values from rl_scene_render_rays on
    the same samples."""
    res = scene.render_spectral_rays(samples["ray"], seed, stream, first, fetch=fetch)
    photons = np.zeros(len(samples), R.PHOTON_DTYPE)
    photons["x"], photons["y"], photons["wavelength"] = samples["x"], samples["y"], samples["ray"]["wavelength"]
    photons["probability"] = res["value"] * samples["reserved1"].view(np.float32)       # one f32 multiply
    return photons


@functools.lru_cache(maxsize=None)
def _path_oracle(name):
    objs, cam = _desc(name)
    return PO.PathOracle(objs, cam)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("film", FILMS, ids=FILM_IDS)
def test_the_values_of_adaptive_samples_are_the_path_oracles(film, plan):
    """The chain's last link on the CPU: rl_scene_render_rays on the plan's samples, which the film tests take the values from, is
    tests/_path_oracle.py's render_ray for 160 samples spread over the plan, bit for bit."""
    w, h = film
    n, seed, stream, first = 1 << 14, 3, 2, 12345
    scene, oracle = _scene("demo"), _path_oracle("demo")
    unit, counts, weights = _planned(w, h, plan, n)
    samples = unit.samples(scene, seed, stream, first, 0, n)
    res = scene.render_spectral_rays(samples["ray"], seed, stream, first)
    CMP.assert_consistent(res)
    picked = np.unique(np.concatenate([np.arange(0, n, n // 128), np.flatnonzero(res["value"] != 0)[:32]]))
    assert (res["value"][picked] != 0).sum() >= 16
    for i in picked:
        r = samples["ray"][i]
        value, segments, obj, end = oracle.render_ray(r["origin"], r["direction"], r["wavelength"], seed, stream, first + int(i))
        got = res[i]
        assert (np.float32(value).tobytes(), segments, obj & 0xffffffff, end) == (got["value"].tobytes(), got["segments"], got["object"], got["end"]), \
            (i, got, value, segments, obj, end)


FILM_CASES = [(s, f, 1 << 16, p, fetch) for s in ("demo", "room-tilted") for f in FILMS for p in PLANS for fetch in (R.FETCH_LDS, R.FETCH_GLOBAL)] + \
             [("demo", FILMS[0], (1 << 20) + 65, "random", R.FETCH_LDS), ("room-tilted", FILMS[1], (1 << 20) + 65, "one_hot_partial", R.FETCH_GLOBAL)]


@pytest.mark.parametrize("scene_name,film,n,plan,fetch", FILM_CASES,
                         ids=["%s-%dx%d-%d-%s-%d" % (s, f[0], f[1], n, p, fetch) for s, f, n, p, fetch in FILM_CASES])
def test_the_film_is_the_sum_of_its_weighted_photons(scene_name, film, n, plan, fetch):
    w, h = film
    scene = _scene(scene_name)
    seed, stream, first = 3, 2, 12345
    unit, counts, weights = _planned(w, h, plan, n)
    samples = unit.samples(scene, seed, stream, first, 0, n)
    photons = _weighted_photons(scene, samples, seed, stream, first, fetch)
    assert (photons["probability"] != 0).sum() > 0
    plot = R.PlotUnit(0, w, h)
    before = R.adaptive_launches()
    plot.render_adaptive(unit, scene, seed, stream, first, fetch=fetch)
    chunks = -(-n // (1 << 20))
    assert tuple(a - b for a, b in zip(R.adaptive_launches(), before)) == (chunks, chunks, chunks)
    got = plot.tristimulus_buffer
    want = CMP.assert_film(got, w, h, photons, "%s %dx%d %s n=%d" % (scene_name, w, h, plan, n))
    if n == 1 << 16:
        # a second call adds onto the first; on poisoned LDS it is the same film
        LP.poison_lds(LP.PATTERNS[0])
        plot.render_adaptive(unit, scene, seed, stream, first, fetch=fetch)
        CMP.assert_film(plot.tristimulus_buffer, w, h, np.concatenate([photons, photons]), "twice")
        assert all(ms > 0 for ms in unit.launch_ms())


def test_unit_lifetime():
    """Destroy with a plan loaded, re-plan between renders, two units on one plot unit in turn: the film is the sum of all of it and
    nothing is left behind."""
    w, h, n = 64, 36, 1 << 14
    scene = _scene("demo")
    live = R.live_resources()
    plot = R.PlotUnit(0, w, h)
    a, _, _ = _planned(w, h, "random", n)
    b, _, _ = _planned(w, h, "one_hot_partial", n)
    parts = []
    for k, unit in enumerate((a, b, a)):
        if k == 2:
            unit.plan(None, 1.0, n // 2)       # re-planned between renders
        n_k = n // 2 if k == 2 else n
        samples = unit.samples(scene, 9, 0, k * n, 0, n_k)
        parts.append(_weighted_photons(scene, samples, 9, 0, k * n, R.FETCH_LDS))
        plot.render_adaptive(unit, scene, 9, 0, k * n)
    CMP.assert_film(plot.tristimulus_buffer, w, h, np.concatenate(parts), "three renders, two units")
    a.close()      # with a plan loaded and its scratch taken
    b.close()
    fresh = R.AdaptiveUnit(w, h)
    fresh.plan(None, 1.0, 100)
    fresh.close()  # with a plan and no scratch
    plot.close()
    assert R.live_resources() == live


# ---- the error model --------------------------------------------------------------------------------------------------------------

def test_the_error_model_holds_under_re_planned_batches():
    """64 x 36, demo scene, seed 1: 16 observed adaptive batches of 2^16 paths (stream 0), re-planned from the running tile map after
    the second, against 2^26 uniform paths of stream 1, as tests/test_gpu_error.py holds the uniform sampler -- which runs beside it
    here through the same driver.  z = (S / N - reference mean) / (se / N) over the pixels with se > 0 has a root mean square of 1 in
    expectation if the batches are independent and unbiased and the normalisation is right; batches under different plans are not
    identically distributed, which can only raise the estimate: held inside [0.5, 2], a condition on the model, not a tolerance."""
    w, h, n, k, ratio = 64, 36, 1 << 16, 16, 64
    scene = _scene("demo")
    trace, plot, ref = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    n_ref = ratio * k * n
    for first in range(0, n_ref, 1 << 24):
        trace.render_fused(scene, plot, 1 << 24, seed=1, stream=1, first_path_index=first)
        ref.accumulate(plot)
    ref_mean = ref.tristimulus_buffer.reshape(h, w, 3)[:, :, 1].astype(np.float64) / n_ref
    rms = {}
    for adaptive_sampling in (False, True):
        unit, gather, adaptive = R.ErrorUnit(w, h), R.GatherUnit(w, h), R.AdaptiveUnit(w, h)
        made, stats, tiles = R.render_adaptive_to_error(scene, plot, gather, unit, adaptive, n, k, 0.0, uniform_share=SHARE, min_observations=2,
                                                        seed=1, stream=0, adaptive_sampling=adaptive_sampling)
        assert made == k and stats["observations"] == k and stats["paths"] == k * n
        s, q, kk, paths = unit.download()
        _, se, _ = unit.estimate(tiles=False)
        on = se > 0
        z = (s[on] / paths - ref_mean[on]) / (se[on].astype(np.float64) / paths)
        rms[adaptive_sampling] = float(np.sqrt((z * z).mean()))
        print("%s: rms z = %.4f over %d of %d pixels; relative_error %.5f, worst tile %.5f"
              % ("adaptive" if adaptive_sampling else "uniform", rms[adaptive_sampling], int(on.sum()), w * h, stats["relative_error"],
                 stats["worst_tile_error"]))
        assert on.sum() > w * h // 2
        uniform = AO.plan(w, h, None, 1.0, n)[1]
        assert (adaptive.download_plan()[0].reshape(-1).tobytes() != uniform.tobytes()) == adaptive_sampling
    assert 0.5 <= rms[False] <= 2.0
    assert 0.5 <= rms[True] <= 2.0



def test_the_driver_stops_at_a_reachable_target():
    """render_adaptive_to_error ends at the first estimate that meets the target: on the CPU the uniform sampler is at 0.144 after 8
    batches and 0.106 after 16, so 0.125 is met in between, by either sampler."""
    w, h, n = 64, 36, 1 << 16
    scene, plot = _scene("demo"), R.PlotUnit(0, w, h)
    for adaptive_sampling in (False, True):
        unit, gather, adaptive = R.ErrorUnit(w, h), R.GatherUnit(w, h), R.AdaptiveUnit(w, h)
        made, stats, tiles = R.render_adaptive_to_error(scene, plot, gather, unit, adaptive, n, 16, 0.125, uniform_share=SHARE, min_observations=4,
                                                        seed=1, stream=0, adaptive_sampling=adaptive_sampling)
        print("%s: stopped after %d batches at %.5f" % ("adaptive" if adaptive_sampling else "uniform", made, stats["relative_error"]))
        assert 8 < made < 16 and stats["relative_error"] <= 0.125 and (stats["observations"], stats["paths"]) == (made, made * n)
        assert unit.download()[2] == made and tiles.shape == (3, 4, 2)
    with pytest.raises(ValueError):
        R.render_adaptive_to_error(scene, plot, gather, unit, adaptive, n, 3, 0.125, min_observations=4)


def test_the_command_line_with_adaptive_stops_at_the_target_and_writes_the_map(tmp_path, capsys):
    """--adaptive is the driver above with the command line's defaults filled in: the same 11 batches, the image, and --error-map as
    without it."""
    out, grey = str(tmp_path / "image.png"), str(tmp_path / "map.ppm")
    CLI.main(["--target-error", "0.125", "--adaptive", "--min-observations", "4", "--error-map", grey, "--output", out, "--width", "64",
              "--height", "36", "--batches", "16", "--photons-per-batch", "65536", "--quiet"])
    told = capsys.readouterr().out
    assert "relative_error" in told and "reached 1, 11 of 16 batches used" in told and "error map: wrote" in told, told
    assert "adaptive: 11 of 16 batches" in told and "target reached" in told, told
    assert open(out, "rb").read().startswith(b"\x89PNG")
    data = open(grey, "rb").read()
    assert data.startswith(b"P6\n64 36\n255\n")
    pixels = np.frombuffer(data[len(b"P6\n64 36\n255\n"):], np.uint8).reshape(36, 64, 3)
    assert pixels.max() == 255 and (pixels[:, :, 0] == pixels[:, :, 1]).all() and (pixels[:16, :16] == pixels[0, 0]).all()
    CLI.main(["--target-error", "0.01", "--adaptive", "--min-observations", "4", "--output", out, "--width", "64", "--height", "36",
              "--batches", "5", "--photons-per-batch", "65536", "--quiet"])
    told = capsys.readouterr().out
    assert "reached 0, 5 of 5 batches used" in told and "target not reached" in told, told


# ---- it helps ---------------------------------------------------------------------------------------------------------------------

def test_uniform_against_adaptive_is_what_the_cpu_run_showed():
    """64 x 36, demo scene, seed 1, 16 batches of 2^16 paths of stream 0 after a warm-up of 4 uniform batches, uniform against adaptive
    through the same driver; relative_error and worst_tile_error from rl_error_unit_estimate and the mean squared error of the XYZ
    mean against 2^23 paths of stream 1.  tools/adaptive_gain.py made the same run on the CPU oracle (tests/golden/adaptive_gain.json,
    the table in DESIGN.md): there adaptive sampling lowers relative_error (0.9555 of uniform) and the mean squared error (0.9237), and
    RAISES the worst tile's error (1.0415) -- the importance is a tile's absolute t_se, which favours bright tiles, while the worst
    tile is measured relative to its brightness.  Asserted here: the direction of the two that gain, and, the photons being the
    oracle's, that all three device ratios are the CPU ones to four digits."""
    cfg = AO.GAIN
    w, h, n, k = cfg["w"], cfg["h"], cfg["n"], AO.GAIN_TEST_BUDGET
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adaptive_gain.json")))
    assert golden["config"] == {key: (list(v) if isinstance(v, tuple) else v) for key, v in cfg.items()}
    want = golden["budgets"][str(k)]
    scene = _scene("demo")
    trace, plot, ref = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    trace.render_fused(scene, plot, cfg["n_ref"], seed=cfg["seed"], stream=cfg["ref_stream"], first_path_index=0)
    ref.accumulate(plot)
    ref_mean = ref.tristimulus_buffer.astype(np.float64) / cfg["n_ref"]
    got = {}
    for adaptive_sampling in (False, True):
        unit, gather, adaptive = R.ErrorUnit(w, h), R.GatherUnit(w, h), R.AdaptiveUnit(w, h)
        made, stats, _ = R.render_adaptive_to_error(scene, plot, gather, unit, adaptive, n, k, 0.0, uniform_share=cfg["share"],
                                                    min_observations=cfg["warmup"], seed=cfg["seed"], stream=cfg["stream"],
                                                    adaptive_sampling=adaptive_sampling)
        assert made == k
        mse = float(((gather.tristimulus_buffer.astype(np.float64) / (k * n) - ref_mean) ** 2).mean())
        got[adaptive_sampling] = {"relative_error": stats["relative_error"], "worst_tile_error": stats["worst_tile_error"], "mse": mse}
    for metric in ("relative_error", "worst_tile_error", "mse"):
        ratio = got[True][metric] / got[False][metric]
        print("%-16s uniform %.6g adaptive %.6g ratio %.5f (CPU: %.6g, %.6g, %.5f)"
              % (metric, got[False][metric], got[True][metric], ratio, want[metric]["uniform"], want[metric]["adaptive"], want[metric]["ratio"]))
    for metric in ("relative_error", "worst_tile_error", "mse"):
        ratio = got[True][metric] / got[False][metric]
        assert abs(ratio / want[metric]["ratio"] - 1.0) < 5e-4, (metric, ratio, want[metric]["ratio"])      # four digits
    assert want["relative_error"]["ratio"] < 1 and got[True]["relative_error"] < got[False]["relative_error"]
    assert want["mse"]["ratio"] < 1 and got[True]["mse"] < got[False]["mse"]
