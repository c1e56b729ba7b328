"""The noise estimate on the device (rl_error_unit_*, rl_app_run_to_error) against the CPU restatement (tests/_error_oracle.py) bit
for bit: every shape x observation set of tests/_error_cases.py, the estimate on poisoned LDS and into guarded, prefilled buffers,
what observe leaves alone, its ordering against work queued on the plot unit, a real render against a 64 times longer one, the App's
stopping rule and the command line.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _error_cases as EC
import _error_oracle as EO
import _guarded as G
import _lds_poison as LP
from _image_cases import same_bits

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5


def _err():
    return _lib.lib.rl_last_error()


@functools.lru_cache(maxsize=None)
def _rig(w, h):
    """(error unit, plot unit) of a shape: shared by its cases."""
    return R.ErrorUnit(w, h), R.PlotUnit(0, w, h)


def _same_stats(got, want):
    for key, value in want.items():
        g = got[key]
        if isinstance(value, float):
            assert same_bits(np.float64(g), np.float64(value)), (key, g, value)
        else:
            assert g == value, (key, g, value)
    assert sorted(got) == sorted(want)


def _feed(unit, plot, case, w, h):
    """The case on the device and on the oracle: returns the oracle's state."""
    unit.clear()
    state = EO.new_state(w, h)
    if case["initial"] is not None:
        state = case["initial"]
        unit.upload(*state)
    for xyz, n in case["observations"]:
        plot.upload(xyz)
        unit.observe(plot, n)
        state = EO.observe(state, xyz, n)
    return state


def _check_estimate(unit, state):
    stats, se, tiles = unit.estimate()
    want_stats, want_se, want_tiles = EO.estimate(state)
    assert same_bits(se, want_se), int((se.view(np.uint32) != want_se.view(np.uint32)).sum())
    assert same_bits(tiles, want_tiles), (tiles, want_tiles)
    _same_stats(stats, want_stats)
    return stats, se, tiles


@pytest.mark.parametrize("name", EC.CASES)
@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_and_observation_set_matches_the_oracle_bit_for_bit(shape, name):
    w, h = shape
    unit, plot = _rig(w, h)
    case = EC.case(name, w, h)
    before = R.error_launches()
    state = _feed(unit, plot, case, w, h)
    s, q, k, n = unit.download()
    assert same_bits(s, state[0]) and same_bits(q, state[1]) and (k, n) == (state[2], state[3])
    stats, se, tiles = _check_estimate(unit, state)
    after = R.error_launches()
    assert (after[0] - before[0], after[1] - before[1]) == (len(case["observations"]), 1)
    assert (stats["tiles_x"], stats["tiles_y"]) == (-(-w // 16), -(-h // 16)) == (unit.tiles_x, unit.tiles_y)
    # the estimate is a function of the state: a second one gives the same bits, with either output left out
    again = unit.estimate(se=False, tiles=True)
    assert again[1] is None and same_bits(again[2], tiles)
    again = unit.estimate(se=True, tiles=False)
    assert again[2] is None and same_bits(again[1], se)
    if name == "proportional":
        assert se.tobytes() == bytes(se.nbytes)
    if name == "huge":
        assert np.isinf(se[0, 0]) and np.isinf(se[h - 1, w - 1])
    if name == "nonfinite":
        assert np.isnan(se[0, 0]) and np.isnan(se[h - 1, w - 1])


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("shape", EC.PARTIAL + [(5, 3)], ids=lambda s: "%dx%d" % s)
def test_the_estimate_on_poisoned_lds_and_between_guards(shape, pattern):
    """Every element of the trees is written before it is read, positions outside the image included, and se and tiles are written
    whole and nowhere else: stale LDS and 0xAA bytes in and around the outputs change nothing."""
    w, h = shape
    unit, plot = _rig(w, h)
    state = _feed(unit, plot, EC.case("n_unequal", w, h), w, h)
    want_stats, want_se, want_tiles = EO.estimate(state)
    se = G.Guarded(G.HostBuffer, nbytes=4 * w * h)
    tiles = G.Guarded(G.HostBuffer, nbytes=16 * unit.tiles_x * unit.tiles_y)
    stats = _lib.RlErrorStats()
    LP.poison_lds(pattern)
    R.check(_lib.lib.rl_error_unit_estimate(unit.handle, C.byref(stats), C.c_void_p(se.data_ptr()), C.c_void_p(tiles.data_ptr())))
    assert same_bits(se.payload("se", np.float32).reshape(h, w), want_se)
    assert same_bits(tiles.payload("tiles", np.float64).reshape(want_tiles.shape), want_tiles)
    _same_stats({name: getattr(stats, name) for name, _ in _lib.RlErrorStats._fields_}, want_stats)


def test_observe_leaves_the_plot_buffer_and_the_gathered_sum_as_they_were():
    w, h = 33, 47
    unit, plot = R.ErrorUnit(w, h), R.PlotUnit(0, w, h)
    with_observes, without = R.GatherUnit(w, h), R.GatherUnit(w, h)
    case = EC.case("nonfinite", w, h)["observations"] + EC.case("negative", w, h)["observations"]
    for xyz, n in case:
        plot.upload(xyz)
        unit.observe(plot, n)
        assert same_bits(plot.tristimulus_buffer, xyz.reshape(-1, 3))
        unit.observe(plot, n)
        with_observes.accumulate(plot)
        assert not plot.tristimulus_buffer.any()
        plot.upload(xyz)
        without.accumulate(plot)
    a, b = with_observes._download(), without._download()
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert unit.download()[2:] == (2 * len(case), 2 * sum(n for _, n in case))


def test_every_argument_failure_on_a_live_unit():
    w, h = 17, 16
    unit, plot = R.ErrorUnit(w, h), R.PlotUnit(0, w, h)
    L = _lib.lib
    stats = _lib.RlErrorStats()
    launches = R.error_launches()
    for k in (0, 1):
        assert L.rl_error_unit_estimate(unit.handle, C.byref(stats), None, None) == RL_E_STATE and b"at least 2" in _err()
        unit.observe(plot, 3)
    unit.clear()
    assert unit.download()[2:] == (0, 0)
    mark = np.full((h, w), 2.5)
    unit.upload(mark, mark, 5, (1 << 64) - 4)
    for other in (R.PlotUnit(1, w + 1, h), R.PlotUnit(1, w, h + 1), R.PlotUnit(1, h, w)):
        assert L.rl_error_unit_observe(unit.handle, other.handle, 3) == RL_E_STATE and b"does not match" in _err()
    assert L.rl_error_unit_observe(unit.handle, plot.handle, 4) == RL_E_INVALID and b"overflows" in _err()
    assert L.rl_error_unit_observe(unit.handle, plot.handle, 0) == RL_E_INVALID and b"n_paths" in _err()
    s, q, k, n = unit.download()
    assert (s == 2.5).all() and (q == 2.5).all() and (k, n) == (5, (1 << 64) - 4)      # nothing was written
    unit.observe(plot, 3)                                                              # 2^64 - 1 is reached exactly
    assert unit.download()[3] == (1 << 64) - 1
    after = R.error_launches()
    assert (after[0] - launches[0], after[1] - launches[1]) == (3, 0)
    with pytest.raises(R.RlError) as e:
        R.ErrorUnit(0, 4)
    assert e.value.code == RL_E_INVALID


@functools.lru_cache(maxsize=None)
def _demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return R.Scene(objs, cam)


def test_observe_waits_for_a_fused_render_begun_into_the_plot_unit():
    """render_fused_begin into the plot unit and observe at once, with no wait between: the sums are those of the finished buffer
    (which observe leaves in place), and a second unit that observes after a host synchronisation holds the same bits."""
    w, h, n = 64, 36, 1 << 18
    scene = _demo()
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    at_once, after_sync = R.ErrorUnit(w, h), R.ErrorUnit(w, h)
    trace.render_fused_begin(scene, plot, n, seed=1, stream=0, first_path_index=0)
    at_once.observe(plot, n)
    plot.sync()
    after_sync.observe(plot, n)
    xyz = plot.tristimulus_buffer.reshape(h, w, 3)
    assert (xyz[:, :, 1] > 0).sum() > w * h // 2
    want = EO.observe(EO.new_state(w, h), xyz, n)
    for unit in (at_once, after_sync):
        s, q, k, paths = unit.download()
        assert same_bits(s, want[0]) and same_bits(q, want[1]) and (k, paths) == (1, n)


def test_a_real_render_against_one_of_64_times_as_many_paths():
    """64 x 36, demo scene, seed 1: 16 fused observations of 2^16 paths (stream 0, paths 0 .. 2^20) against 2^26 paths of stream 1.
    The unit's state is the oracle's on the downloaded buffers, bit for bit.  z = (S / N - reference mean) / (se / N) over the pixels
    with se > 0 has a root mean square of 1 in expectation (1 + 1/64 with the reference's own noise) if the batches are independent
    and the normalisation is right: held inside [0.5, 2], a condition on the model, not a tolerance.  Measured on an MI355X: 1.42
    (DESIGN.md section 4)."""
    w, h, n, k, ratio = 64, 36, 1 << 16, 16, 64
    scene = _demo()
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    unit, gather, ref = R.ErrorUnit(w, h), R.GatherUnit(w, h), R.GatherUnit(w, h)
    state = EO.new_state(w, h)
    for j in range(k):
        trace.render_fused(scene, plot, n, seed=1, stream=0, first_path_index=j * n)
        unit.observe(plot, n)
        state = EO.observe(state, plot.tristimulus_buffer.reshape(h, w, 3), n)
        gather.accumulate(plot)
    s, q, kk, paths = unit.download()
    assert same_bits(s, state[0]) and same_bits(q, state[1]) and (kk, paths) == (k, k * n)
    stats, se, tiles = _check_estimate(unit, state)
    n_ref = ratio * k * n
    for first in range(0, n_ref, 1 << 24):
        trace.render_fused(scene, plot, 1 << 24, seed=1, stream=1, first_path_index=first)
        ref.accumulate(plot)
    ref_mean = ref.tristimulus_buffer.reshape(h, w, 3)[:, :, 1].astype(np.float64) / n_ref
    on = se > 0
    z = (s[on] / paths - ref_mean[on]) / (se[on].astype(np.float64) / paths)
    rms = float(np.sqrt((z * z).mean()))
    print("rms z = %.4f over %d of %d pixels; relative_error %.5f, worst tile %.5f at (%d, %d)"
          % (rms, int(on.sum()), w * h, stats["relative_error"], stats["worst_tile_error"], stats["worst_tile_x"], stats["worst_tile_y"]))
    # the unit's own S is the gather unit's sum up to the latter's f32 rounding
    total = gather.tristimulus_buffer.reshape(h, w, 3)[:, :, 1].astype(np.float64)
    assert np.abs(total - s).max() <= 2.0 ** -20 * np.abs(s).max()
    assert on.sum() > w * h // 2
    assert 0.5 <= rms <= 2.0


APP = dict(concurrency=2, photons_per_batch=1 << 16, tonemap_interval_ms=5, fused=True)


def test_the_app_stops_at_a_reachable_target():
    cap = 4096
    rgb, st, err = R.app_run_to_error(64, 36, cap, target_error=0.1, **APP)
    stop, end = err["at_stop"], err["at_end"]
    print("reached %d after %d batches, %d estimates: at stop %.5f from %d observations of %d paths, at the end %.5f of %d paths"
          % (err["reached"], st["batches"], err["estimates"], stop["relative_error"], stop["observations"], stop["paths"],
             end["relative_error"], end["paths"]))
    assert err["reached"] == 1 and stop["relative_error"] <= 0.1 and stop["observations"] >= 16
    assert end["paths"] >= stop["paths"] and st["batches"] < cap and err["estimates"] >= 2
    assert end["paths"] == st["batches"] * (1 << 16)
    assert err["tiles"].shape == (3, 4, 2) and rgb.any()
    _same_stats(end, EO.host_stats(err["tiles"], end["observations"], end["paths"]))


def test_the_app_with_target_zero_runs_to_the_cap():
    rgb, st, err = R.app_run_to_error(64, 36, 48, target_error=0.0, **APP)
    assert err["reached"] == 0 and st["batches"] == 48 and err["estimates"] >= 1
    assert not any(err["at_stop"].values()) and err["at_end"]["paths"] == 48 * (1 << 16)
    # a worst-tile bound that cannot be met holds the run as well, whatever the image's own estimate
    rgb, st, err = R.app_run_to_error(64, 36, 48, target_error=1e9, worst_tile_error=1e-12, **APP)
    assert err["reached"] == 0 and st["batches"] == 48
    # ... and min_observations does: the cap comes first
    rgb, st, err = R.app_run_to_error(64, 36, 24, target_error=1e9, min_observations=100000, **APP)
    assert err["reached"] == 0 and st["batches"] == 24


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_the_app_counts_the_paths_of_two_ranks_on_one_device(fused):
    args = dict(APP, fused=fused)
    rgb, st, err = R.app_run_to_error(64, 36, 40, target_error=0.0, devices=[0, 0], **args)
    assert st["batches"] == 40 and err["at_end"]["paths"] == 2 * 40 * (1 << 16) and err["reached"] == 0


def test_the_app_without_a_target_is_app_run():
    before = R.error_launches()
    rgb, st, err = R.app_run_to_error(64, 36, 8, target_error=None, **APP)
    rgb2, st2 = R.app_run(64, 36, 8, **APP)
    assert R.error_launches() == before
    assert err["reached"] == 0 and err["estimates"] == 0 and err["tiles"] is None
    assert not any(err["at_stop"].values()) and not any(err["at_end"].values())
    assert (st["batches"], st["paths"], st["next_batch"]) == (st2["batches"], st2["paths"], st2["next_batch"]) == (8, 8 << 16, 8)
    assert rgb.any() and np.abs(rgb.astype(np.int32) - rgb2.astype(np.int32)).max() <= 1      # (the order of the film's atomics)


def test_the_command_line_stops_at_a_target_and_writes_the_map(tmp_path, capsys):
    out, grey = str(tmp_path / "image.png"), str(tmp_path / "map.ppm")
    CLI.main(["--target-error", "0.1", "--error-map", grey, "--output", out, "--width", "64", "--height", "36", "--batches", "4096",
              "--photons-per-batch", "65536", "--quiet"])
    told = capsys.readouterr().out
    assert "relative_error" in told and "reached 1" in told and "error map: wrote" in told, told
    used = int(told.split("reached 1, ")[1].split(" of 4096")[0])
    assert 0 < used < 4096
    data = open(grey, "rb").read()
    assert data.startswith(b"P6\n64 36\n255\n")
    pixels = np.frombuffer(data[len(b"P6\n64 36\n255\n"):], np.uint8).reshape(36, 64, 3)
    assert pixels.max() == 255 and (pixels[:, :, 0] == pixels[:, :, 1]).all() and (pixels[:16, :16] == pixels[0, 0]).all()
