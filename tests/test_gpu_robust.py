"""The robust film on the device (rl_robust_unit_*) against the CPU restatement (tests/_robust_oracle.py) bit for bit: every shape x
bucket count x observation schedule of tests/_robust_cases.py, the resolve's edge states on poisoned LDS and over a dst that held a
film, a size at which both grid-stride loops iterate, real plot buffers, the round trip through the host, what the calls refuse on a
live unit, a real render of the glass-stress scene, and the command line.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _accumulation as A
import _lds_poison as LP
import _robust_cases as RC
import _robust_oracle as RO
from _compare import assert_same

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5
INF = float("inf")


def _err():
    return _lib.lib.rl_last_error()


@functools.lru_cache(maxsize=None)
def _rig(w, h, m):
    """(robust unit, plot unit, gather unit) of a shape and bucket count: shared by its cases."""
    return R.RobustUnit(w, h, m), R.PlotUnit(0, w, h), R.GatherUnit(w, h)


@functools.lru_cache(maxsize=None)
def _scene(which):
    objs, cam = R.builtin_scene_desc(which)
    return R.Scene(objs, cam)


def _feed(unit, plot, observations, state):
    """Every observation on the device and on the oracle; after each the plot buffer holds its bytes unchanged."""
    for xyz, n, bucket in observations:
        plot.upload(xyz)
        unit.observe(plot, n, None if bucket == RC.NEXT else bucket)
        assert_same(plot.tristimulus_buffer, xyz.reshape(-1, 3), "the plot buffer after observe")
        state = RO.observe(state, xyz, n, bucket)
    return state


def _check_state(unit, state):
    sums, paths, k = unit.download()
    assert sums.shape == state[0].shape
    assert_same(sums.reshape(sums.shape[0] * 3, -1), state[0].reshape(sums.shape[0] * 3, -1), "the planes")
    assert [int(x) for x in paths] == state[1] and k == state[2]


def _check_resolve(unit, dst, state, gain, max_trim):
    want_film, want_trim, want_stats = RO.resolve(state, gain, max_trim)
    stats, trim = unit.resolve(dst, gain=gain, max_trim=max_trim, trim=True)
    film, comp = dst._download()
    what = "gain %r max_trim %r" % (gain, max_trim)
    assert_same(film, want_film.reshape(-1, 3), "the film, " + what)
    assert comp.tobytes() == bytes(comp.nbytes), "the compensation is +0, " + what
    assert_same(trim, want_trim, "the trim, " + what)
    assert stats == want_stats, (what, stats, want_stats)
    return film, trim, stats


@pytest.mark.parametrize("schedule", RC.SCHEDULES)
@pytest.mark.parametrize("m", RC.BUCKETS)
@pytest.mark.parametrize("shape", RC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_bucket_count_and_schedule_matches_the_oracle_bit_for_bit(shape, m, schedule):
    w, h = shape
    unit, plot, dst = _rig(w, h, m)
    observations = RC.schedule(schedule, w, h, m)
    before = R.robust_launches()
    unit.clear()
    state = _feed(unit, plot, observations, RO.new_state(w, h, m))
    _check_state(unit, state)
    for gain, max_trim in RC.PARAMS:
        _check_resolve(unit, dst, state, gain, max_trim)
    after = R.robust_launches()
    assert (after[0] - before[0], after[1] - before[1]) == (len(observations), len(RC.PARAMS))
    # the resolve is a function of the state: without stats or trim it writes the same film
    want = dst._download()[0]
    params = _lib.RlRobustParams(*RC.PARAMS[-1], 0)
    plot.upload(np.full((h, w, 3), 7.0, np.float32))
    dst.accumulate(plot)
    R.check(_lib.lib.rl_robust_unit_resolve(unit.handle, C.byref(params), dst.handle, None, None))
    assert_same(dst._download()[0], want, "the film without stats and trim")


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("m", RC.BUCKETS)
@pytest.mark.parametrize("shape", [(17, 5), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_the_edge_states_on_poisoned_lds_over_a_dst_that_held_a_film(shape, m, pattern):
    """Ties, NaN, infinities, negatives, zeros, one and two outliers and c = cmax (tests/_robust_cases.py: edge_state) under every
    (gain, max_trim): every LDS word the resolve reads it wrote first, and dst's previous film and compensation are replaced."""
    w, h = shape
    unit, plot, dst = _rig(w, h, m)
    state = RC.edge_state(w, h, m)
    unit.upload(*state)
    _check_state(unit, state)
    seen = set()
    for gain, max_trim in RC.PARAMS:
        for k in range(3):                                              # a film and a compensation that are not zero
            plot.upload(RC.noisy(np.random.default_rng(k), w, h, 4096) + np.float32(1e-3))
            dst.accumulate(plot)
        assert dst._download()[1].any()
        LP.poison_lds(pattern)
        film, trim, stats = _check_resolve(unit, dst, state, gain, max_trim)
        seen.add(stats["largest_trim"])
        assert stats["untrimmable_pixels"] == sum(1 for q in range(w * h) if q % 12 in (4, 5, 6, 7, 8, 10))
    assert seen >= {0, 1, (m - 1) // 2}                                  # c = cmax for this M, even or odd, was reached


def test_a_size_at_which_both_grid_stride_loops_iterate():
    w, h = RC.GRID_STRIDE_SHAPE
    m = 3
    assert w * h > 2 * 256 * 8 * LP.cu_count(), "the shape no longer exceeds one pass of the observe grid on this device"
    unit, plot, dst = R.RobustUnit(w, h, m), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    rng = np.random.default_rng(11)
    observations = [(RC.noisy(rng, w, h, 4096), 4096 + i, RC.NEXT) for i in range(2 * m + 1)]
    state = _feed(unit, plot, observations, RO.new_state(w, h, m))
    _check_state(unit, state)
    film, trim, stats = _check_resolve(unit, dst, state, 2.0, RC.NO_LIMIT)    # (M = 3: gain 1 never trims)
    assert 0 < stats["trimmed_pixels"] < w * h


@pytest.mark.parametrize("shape", [(16, 9), (64, 36)], ids=lambda s: "%dx%d" % s)
def test_real_plot_buffers_in_turn_and_in_explicit_buckets(shape):
    """A few thousand paths of the demo scene per buffer, rendered fused into the plot unit and observed where they lie: 2 M + 1
    observations in turn, then every bucket once more by number with another path count."""
    w, h = shape
    m, n = 4, 3000
    unit, plot, dst = R.RobustUnit(w, h, m), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    trace = R.TraceUnit(0, w, h, n_photons=64)
    state = RO.new_state(w, h, m)
    schedule = [(n, RC.NEXT)] * (2 * m + 1) + [(n + 1000 * j, j) for j in (2, 0, 3, 1)]
    for i, (paths, bucket) in enumerate(schedule):
        plot.clear()
        trace.render_fused(_scene(R.SCENE_DEMO), plot, paths, seed=3, stream=0, first_path_index=i * 8192)
        xyz = plot.tristimulus_buffer
        assert xyz.any()
        unit.observe(plot, paths, None if bucket == RC.NEXT else bucket)
        assert_same(plot.tristimulus_buffer, xyz, "the plot buffer after observe")
        state = RO.observe(state, xyz.reshape(h, w, 3), paths, bucket)
    _check_state(unit, state)
    for gain, max_trim in RC.PARAMS:
        _check_resolve(unit, dst, state, gain, max_trim)


def test_a_round_trip_through_the_host_and_a_cleared_unit():
    w, h, m = 17, 5, 15
    unit, plot, dst = _rig(w, h, m)
    other = R.RobustUnit(w, h, m)
    unit.clear()
    state = _feed(unit, plot, RC.schedule("unequal", w, h, m), RO.new_state(w, h, m))
    film, trim, stats = _check_resolve(unit, dst, state, 1.0, RC.NO_LIMIT)
    sums, paths, k = unit.download()
    unit.clear()
    params = _lib.RlRobustParams(1.0, RC.NO_LIMIT, 0)
    assert _lib.lib.rl_robust_unit_resolve(unit.handle, C.byref(params), dst.handle, None, None) == RL_E_STATE
    assert b"every bucket needs an observation" in _err()
    assert_same(dst._download()[0], film, "dst after a refused resolve")
    _check_state(unit, RO.new_state(w, h, m))
    for target in (unit, other):
        target.upload(sums, paths, k)
        stats2, trim2 = target.resolve(dst, trim=True)
        assert_same(dst._download()[0], film, "the film after the round trip")
        assert_same(trim2, trim, "the trim after the round trip")
        assert stats2 == stats
    # any of download's outputs may be left out
    k_only = C.c_uint64(0)
    R.check(_lib.lib.rl_robust_unit_download(unit.handle, None, None, C.byref(k_only)))
    assert k_only.value == k
    R.check(_lib.lib.rl_robust_unit_download(unit.handle, None, None, None))


def test_every_argument_failure_on_a_live_unit():
    w, h, m = 17, 16, 5
    unit, plot, dst = R.RobustUnit(w, h, m), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    L = _lib.lib
    mark = np.full((m, 3, h, w), 2.5)
    unit.upload(mark, [1, 2, 3, 4, (1 << 64) - 14], 9)
    plot.upload(np.ones((h, w, 3), np.float32))
    dst.accumulate(plot)
    plot.upload(np.ones((h, w, 3), np.float32))
    before = dst._download()
    launches = R.robust_launches()
    for other in (R.PlotUnit(1, w + 1, h), R.PlotUnit(1, w, h + 1), R.PlotUnit(1, h, w)):
        assert L.rl_robust_unit_observe(unit.handle, other.handle, 3, 0) == RL_E_STATE and b"does not match" in _err()
    assert L.rl_robust_unit_observe(unit.handle, plot.handle, 0, 0) == RL_E_INVALID and b"n_paths" in _err()
    assert L.rl_robust_unit_observe(unit.handle, plot.handle, 1, m) == RL_E_INVALID and b"bucket 5 of 5" in _err()
    assert L.rl_robust_unit_observe(unit.handle, plot.handle, 5, 0) == RL_E_INVALID and b"overflows" in _err()     # the total
    assert L.rl_robust_unit_observe(unit.handle, plot.handle, 14, 4) == RL_E_INVALID and b"overflows" in _err()    # n[4] itself
    params = _lib.RlRobustParams(1.0, RC.NO_LIMIT, 0)
    for other in (R.GatherUnit(w + 1, h), R.GatherUnit(h, w)):
        assert L.rl_robust_unit_resolve(unit.handle, C.byref(params), other.handle, None, None) == RL_E_STATE and b"does not match" in _err()
    for gain in (float("nan"), -1.0):
        assert L.rl_robust_unit_resolve(unit.handle, C.byref(_lib.RlRobustParams(gain, 0, 0)), dst.handle, None, None) == RL_E_INVALID
    assert L.rl_robust_unit_upload(unit.handle, mark.ctypes.data_as(C.c_void_p), np.ones(m, np.uint64).ctypes.data_as(C.c_void_p), 4) == RL_E_INVALID
    sums, paths, k = unit.download()
    assert (sums == 2.5).all() and [int(x) for x in paths] == [1, 2, 3, 4, (1 << 64) - 14] and k == 9               # nothing was written
    after = dst._download()
    assert_same(after[0], before[0], "dst")
    assert_same(after[1], before[1], "dst's compensation")
    assert R.robust_launches() == launches
    unit.observe(plot, 3, 0)                                                                                      # 2^64 - 1 is reached exactly
    assert sum(int(x) for x in unit.download()[1]) == (1 << 64) - 1
    stats = unit.resolve(dst)
    assert stats["paths"] == (1 << 64) - 1 and stats["observations"] == 10
    with pytest.raises(R.RlError) as e:
        R.RobustUnit(4, 4, 2)
    assert e.value.code == RL_E_INVALID


def test_observe_waits_for_a_fused_render_begun_into_the_plot_unit():
    w, h, n, m = 64, 36, 1 << 18, 3
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    at_once, after_sync = R.RobustUnit(w, h, m), R.RobustUnit(w, h, m)
    trace.render_fused_begin(_scene(R.SCENE_DEMO), plot, n, seed=1, stream=0, first_path_index=0)
    at_once.observe(plot, n, 1)
    plot.sync()
    after_sync.observe(plot, n, 1)
    xyz = plot.tristimulus_buffer.reshape(h, w, 3)
    assert (xyz[:, :, 1] > 0).sum() > w * h // 2
    want = RO.observe(RO.new_state(w, h, m), xyz, n, 1)
    for unit in (at_once, after_sync):
        _check_state(unit, want)


def test_a_render_of_the_glass_stress_scene_end_to_end():
    """64 x 36, 30 fused batches of 4,096 paths, M = 15, each batch observed and then gathered.  The resolved film is the oracle's
    resolve of the downloaded plot buffers, bit for bit.  With gain 0 it is the pooled mean of equal buckets times N, the sum of the
    buffers: the gather unit's film of the same buffers lies within its Kahan bound of their exact sum (tests/_accumulation.py:
    kahan_bound at KAHAN_GATHERS, times 1 + 1e-6, as accumulation_bound has it; the splat terms of that bound do not apply, both
    films being sums of the same buffers), and the robust film within one f32 rounding of it, u S, plus its f64 roundings (the 30
    additions, 15 divisions, 15 additions, one division and one multiplication are under 2^-46 S together).  S = sum_j |P_j|."""
    w, h, m, batches, n = 64, 36, 15, 30, 4096
    scene = _scene(R.SCENE_GLASS_STRESS)
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    unit, gather, dst = R.RobustUnit(w, h, m), R.GatherUnit(w, h), R.GatherUnit(w, h)
    state, s_abs = RO.new_state(w, h, m), np.zeros((w * h, 3), np.float64)
    for b in range(batches):
        trace.render_fused_sync(scene, plot, n, seed=1, stream=0, first_path_index=b * n)
        xyz = plot.tristimulus_buffer
        unit.observe(plot, n)
        state = RO.observe(state, xyz.reshape(h, w, 3), n)
        s_abs += np.abs(xyz.astype(np.float64))
        gather.accumulate(plot)
    _check_state(unit, state)
    film, trim, stats = _check_resolve(unit, dst, state, 1.0, RC.NO_LIMIT)
    print("glass-stress, %d x %d paths: %s; trim histogram %s" % (batches, n, stats, np.bincount(trim.reshape(-1), minlength=8).tolist()))
    assert stats["paths"] == batches * n and stats["observations"] == batches and stats["trimmed_pixels"] > 0
    plain = _check_resolve(unit, dst, state, 0.0, RC.NO_LIMIT)[0]
    bound = A.kahan_bound(A.KAHAN_GATHERS, s_abs) * (1 + 1e-6) + A.U * s_abs + 2.0 ** -46 * s_abs
    bad, excess = A.violations(plain, gather.tristimulus_buffer.astype(np.float64), bound)
    print("gain 0 against the gather unit: worst |difference| / bound %.3f" % excess)
    assert not len(bad), (bad[:8], excess)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "fused"])
def test_the_command_line_writes_both_images_and_leaves_the_output_alone(direct, tmp_path, capsys):
    """15 batches of 64 paths each, one wave's worth: the order of the film's float atomics, which may move a byte of two runs of a
    larger batch apart, has nothing to reorder."""
    out, robust, plain = str(tmp_path / "image.ppm"), str(tmp_path / "robust.ppm"), str(tmp_path / "plain.ppm")
    common = ["--width", "64", "--height", "36", "--batches", "15", "--photons-per-batch", "64", "--quiet", "--scene", "glass"]
    common += ["--direct"] if direct else []
    CLI.main(common + ["--output", out, "--robust", robust])
    told = capsys.readouterr().out
    assert "robust film: 15 buckets, gain 1, 15 observations of 960 paths" in told and "wrote %s" % robust in told, told
    CLI.main(common + ["--output", plain])
    assert "robust film" not in capsys.readouterr().out
    head = b"P6\n64 36\n255\n"
    images = [open(p, "rb").read() for p in (out, robust, plain)]
    assert all(data.startswith(head) and len(data) == len(head) + 64 * 36 * 3 for data in images)
    assert images[0] == images[2], "--output with --robust and without"
    assert any(images[0][len(head):])
    CLI.main(common + ["--output", out, "--robust", robust, "--robust-buckets", "3", "--robust-gain", "0"])
    told = capsys.readouterr().out
    assert "robust film: 3 buckets, gain 0, 15 observations of 960 paths; 0 pixels trimmed" in told, told
