"""The robust film's noise estimate on the device (rl_robust_unit_estimate) against the CPU restatement
(tests/_robust_error_oracle.py) bit for bit: every shape x bucket count x observation schedule x (gain, max_trim) of
tests/_robust_error_cases.py, the edge states on poisoned LDS, that the call only reads the unit, what it refuses on a live unit, real
plot buffers, the driver render_robust_to_error step by step, and the command line.  A GPU fault ends the run: nothing here
provokes one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _adaptive_oracle as AO
import _image_cases as IC
import _lds_poison as LP
import _robust_error_cases as EC
import _robust_error_oracle as REO
import _robust_oracle as RO
from _compare import assert_same

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5
NEXT = 0xFFFFFFFF


def _err():
    return _lib.lib.rl_last_error()


@functools.lru_cache(maxsize=None)
def _rig(w, h, m):
    """(robust unit, plot unit) of a shape and bucket count: shared by its cases."""
    return R.RobustUnit(w, h, m), R.PlotUnit(0, w, h)


@functools.lru_cache(maxsize=None)
def _scene(which):
    objs, cam = R.builtin_scene_desc(which)
    return R.Scene(objs, cam)


def _same(got, want, what):
    """Two float arrays bit for bit, by the rule the error unit's tests hold its estimate to (_image_cases.same_bits): every bit
    equal, but that a NaN on the host and a NaN on the device at the same place count as equal.  The host's inf - inf is the
    x86 default NaN, sign bit set; the device's has it clear: no contract on the arithmetic reaches that bit."""
    if not IC.same_bits(got, want):
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        rows = np.flatnonzero((got.reshape(-1).view(u) != want.reshape(-1).view(u)) & ~(np.isnan(got.reshape(-1)) & np.isnan(want.reshape(-1))))
        raise AssertionError("%s: %d of %d values differ, first %d: got %r want %r" % (what, len(rows), got.size, rows[0],
                                                                                     got.reshape(-1)[rows[0]], want.reshape(-1)[rows[0]]))


def _same_stats(got, want, what):
    """RlErrorStats as dicts: the integers equal, the doubles by _same's rule."""
    assert sorted(got) == sorted(want), (what, got, want)
    for name in want:
        if isinstance(want[name], float):
            assert IC.same_bits(np.float64(got[name]), np.float64(want[name])), (what, name, got[name], want[name])
        else:
            assert got[name] == want[name], (what, name, got[name], want[name])


def _check_estimate(unit, state, gain, max_trim):
    want_stats, want_se, want_tiles, want_trim = REO.estimate(state, gain, max_trim)
    before = R.robust_estimate_launches()
    stats, se, tiles, trim = unit.estimate(gain, max_trim, trim=True)
    assert R.robust_estimate_launches() == before + 1
    what = "gain %r max_trim %r" % (gain, max_trim)
    _same(se, want_se, "se, " + what)
    _same(tiles, want_tiles, "the tiles, " + what)
    assert_same(trim, want_trim, "the trim, " + what)
    _same_stats(stats, want_stats, what)
    return stats, se, tiles, trim


@pytest.mark.parametrize("schedule", EC.SCHEDULES)
@pytest.mark.parametrize("m", EC.BUCKETS)
@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_shape_bucket_count_and_schedule_matches_the_oracle_bit_for_bit(shape, m, schedule):
    w, h = shape
    unit, plot = _rig(w, h, m)
    unit.clear()
    state = RO.new_state(w, h, m)
    for xyz, n, bucket in EC.schedule(schedule, w, h, m):
        plot.upload(xyz)
        unit.observe(plot, n, None if bucket == NEXT else bucket)
        state = RO.observe(state, xyz, n, bucket)
    launches = R.robust_launches()
    for gain, max_trim in EC.PARAMS:
        _check_estimate(unit, state, gain, max_trim)
    assert R.robust_launches() == launches                               # a counter of its own
    # the stats are a function of the state: two calls without se, tiles and trim give them again
    want = REO.estimate(state, *EC.PARAMS[-1])[0]
    params = _lib.RlRobustParams(*EC.PARAMS[-1], 0)
    for _ in range(2):
        stats = _lib.RlErrorStats()
        R.check(_lib.lib.rl_robust_unit_estimate(unit.handle, C.byref(params), C.byref(stats), None, None, None))
        _same_stats({name: getattr(stats, name) for name, _ in _lib.RlErrorStats._fields_}, want, "without se, tiles and trim")


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("m", EC.BUCKETS)
@pytest.mark.parametrize("shape", EC.POISON_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_edge_states_on_poisoned_lds(shape, m, pattern):
    """Ties, NaN, infinities, negatives, zeros, one and two outliers and c = cmax (tests/_robust_cases.py: edge_state) under every
    (gain, max_trim): every LDS word the estimate reads it wrote first, the trees' words included.  A NaN tile is a NaN tile on the
    oracle too (_same)."""
    w, h = shape
    unit, _ = _rig(w, h, m)
    state = EC.edge_state(w, h, m)
    unit.upload(*state)
    seen = set()
    for gain, max_trim in EC.PARAMS:
        LP.poison_lds(pattern)
        stats, se, tiles, trim = _check_estimate(unit, state, gain, max_trim)
        seen.add(int((trim & 0x7F).max()))
        assert int((trim >> 7).sum()) == sum(1 for q in range(w * h) if q % 12 in (4, 5, 6, 7, 8, 10))
    assert np.isnan(tiles).any()
    assert seen >= {0, (m - 2) // 2}                                     # c = cmax for this M was reached


def test_the_estimate_only_reads_the_unit_and_leaves_resolves_alone():
    w, h, m = 33, 17, 15
    unit, plot = _rig(w, h, m)
    first, second = R.GatherUnit(w, h), R.GatherUnit(w, h)
    state = EC.edge_state(w, h, m, seed=1)
    unit.upload(*state)
    stats_a, trim_a = unit.resolve(first, trim=True)
    film_a, comp_a = first._download()
    sums, paths, k = unit.download()
    for gain, max_trim in EC.PARAMS:
        _check_estimate(unit, state, gain, max_trim)
    after = unit.download()
    assert after[0].tobytes() == sums.tobytes() and after[1].tobytes() == paths.tobytes() and after[2] == k
    assert_same(first._download()[0], film_a, "a gather unit resolved before")
    assert_same(first._download()[1], comp_a, "its compensation")
    stats_b, trim_b = unit.resolve(second, trim=True)                    # an estimate between two resolves changes neither
    assert stats_b == stats_a
    assert_same(trim_b, trim_a, "the second resolve's trim")
    assert_same(second._download()[0], film_a, "the second resolve's film")


def test_refusals_on_a_live_unit_write_nothing_and_launch_nothing():
    w, h, m = 17, 16, 5
    unit, plot = R.RobustUnit(w, h, m), R.PlotUnit(0, w, h)
    L = _lib.lib
    mark = np.full((m, 3, h, w), 2.5)
    unit.upload(mark, [1, 2, 3, 4, 5], 9)
    stats = _lib.RlErrorStats()
    stats.observations = 77
    se, tiles, trim = np.full((h, w), 3.0, np.float32), np.full((1, 2, 2), 4.0), np.full((h, w), 9, np.uint8)
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in (se, tiles, trim)]
    launches = R.robust_estimate_launches()
    good = _lib.RlRobustParams(1.0, EC.NO_LIMIT, 0)
    assert L.rl_robust_unit_estimate(None, C.byref(good), C.byref(stats), *ptrs) == RL_E_INVALID
    assert L.rl_robust_unit_estimate(unit.handle, None, C.byref(stats), *ptrs) == RL_E_INVALID
    assert L.rl_robust_unit_estimate(unit.handle, C.byref(good), None, *ptrs) == RL_E_INVALID and b"null robust unit, params or stats" in _err()
    for gain in (float("nan"), -1.0, -float("inf")):
        assert L.rl_robust_unit_estimate(unit.handle, C.byref(_lib.RlRobustParams(gain, 0, 0)), C.byref(stats), *ptrs) == RL_E_INVALID
        assert b"gain is negative or not a number" in _err()
    unit.upload(mark, [1, 2, 0, 4, 5], 9)                                # an empty bucket
    assert L.rl_robust_unit_estimate(unit.handle, C.byref(good), C.byref(stats), *ptrs) == RL_E_STATE
    assert b"bucket 2 holds no paths" in _err()
    unit.clear()
    assert L.rl_robust_unit_estimate(unit.handle, C.byref(good), C.byref(stats), *ptrs) == RL_E_STATE and b"bucket 0 holds no paths" in _err()
    assert stats.observations == 77 and (se == 3.0).all() and (tiles == 4.0).all() and (trim == 9).all()
    assert R.robust_estimate_launches() == launches
    unit.upload(mark, [1, 2, 3, 4, 5], 9)
    _check_estimate(unit, (mark, [1, 2, 3, 4, 5], 9), 1.0, EC.NO_LIMIT)
    assert unit.estimate_ms() > 0


def test_real_buffers_of_the_glass_stress_scene():
    """64 x 36, 30 fused batches of 4,096 paths, M = 15: the estimate is the oracle's on the downloaded plot buffers, bit for bit, under
    gain 1 and gain 0, and its trim is the resolve's wherever the resolve stays below its own cap of 7 (the estimate's is 6).  The two
    relative errors are printed, not compared: nothing says which way they must differ on a real film."""
    w, h, m, batches, n = 64, 36, 15, 30, 4096
    scene = _scene(R.SCENE_GLASS_STRESS)
    trace, plot = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    unit, dst = R.RobustUnit(w, h, m), R.GatherUnit(w, h)
    state = RO.new_state(w, h, m)
    for b in range(batches):
        trace.render_fused_sync(scene, plot, n, seed=1, stream=0, first_path_index=b * n)
        xyz = plot.tristimulus_buffer
        unit.observe(plot, n)
        state = RO.observe(state, xyz.reshape(h, w, 3), n)
        plot.clear()
    stats, se, tiles, trim = _check_estimate(unit, state, 1.0, EC.NO_LIMIT)
    plain = _check_estimate(unit, state, 0.0, EC.NO_LIMIT)[0]
    assert (stats["observations"], stats["paths"], stats["tiles_x"], stats["tiles_y"]) == (batches, batches * n, 4, 3)
    assert (trim & 0x7F).any() and stats["relative_error"] > 0
    print("glass-stress, %d x %d paths: relative_error %.5f trimmed, %.5f untrimmed; %d pixels trimmed"
          % (batches, n, stats["relative_error"], plain["relative_error"], int(((trim & 0x7F) > 0).sum())))
    resolved = unit.resolve(dst, trim=True)[1]
    agree = resolved < (m - 1) // 2
    assert ((trim & 0x7F)[agree] == resolved[agree]).all()


class _RecordingRobust(R.RobustUnit):
    """A robust unit that keeps the oracle's state of what it was shown and checks every estimate against it."""

    def start(self):
        self.state, self.estimates = RO.new_state(self.width, self.height, self.n_buckets), []

    def observe(self, plot_unit, n_paths, bucket=None):
        xyz = plot_unit.tristimulus_buffer.reshape(self.height, self.width, 3)
        self.state = RO.observe(self.state, xyz, n_paths, NEXT if bucket is None else bucket)
        super().observe(plot_unit, n_paths, bucket)

    def estimate(self, gain=1.0, max_trim=0xFFFFFFFF, se=True, trim=False):
        out = super().estimate(gain, max_trim, se=se, trim=trim)
        want = REO.estimate(self.state, gain, max_trim)
        _same_stats(out[0], want[0], "estimate %d of the driver" % len(self.estimates))
        _same(out[2], want[2], "tiles of estimate %d of the driver" % len(self.estimates))
        self.estimates.append((self.state[2], want[2]))
        return out


class _RecordingAdaptive(R.AdaptiveUnit):
    """An adaptive unit that keeps the counts of every plan it made."""

    def start(self):
        self.plans = []

    def plan(self, importance, uniform_share, n_paths):
        out = super().plan(importance, uniform_share, n_paths)
        self.plans.append(self.download_plan()[0].reshape(-1).copy())
        return out


@pytest.mark.parametrize("adaptive_sampling", [True, False], ids=["adaptive", "uniform"])
def test_the_driver_step_by_step(adaptive_sampling):
    """render_robust_to_error at 64 x 36 with 64-path batches -- one wave, so the film's atomics have nothing to reorder -- and M = 3,
    6 batches and a target no estimate meets: estimates after batches 3 .. 6, each the oracle's of the plot buffers shown so far; the
    first plan uniform and, with adaptive sampling, the plan after each estimate but the last the plan rule's of that estimate's
    t_se.  uniform_share 0.75: a bottom-row tile's area share is at least 15.5 x 3.5 / (63 x 35) = 0.0246, so its
    0.75 x 64 x 0.0246 = 1.18 paths by area keep it from ever being empty, which the plan rule refuses."""
    w, h, m, n, batches, share = 64, 36, 3, 64, 6, 0.75
    scene, plot, gather = _scene(R.SCENE_DEMO), R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    robust, adaptive = _RecordingRobust(w, h, m), _RecordingAdaptive(w, h)
    robust.start()
    adaptive.start()
    made, stats, tiles = R.render_robust_to_error(scene, plot, gather, robust, adaptive, n, batches, -1.0, gain=2.0, uniform_share=share,
                                                  seed=3, adaptive_sampling=adaptive_sampling)
    assert made == batches and [k for k, _ in robust.estimates] == [3, 4, 5, 6]
    assert (stats["observations"], stats["paths"]) == (batches, batches * n)
    _same(tiles, robust.estimates[-1][1], "the returned tiles")
    uniform = AO.plan(w, h, None, share, n)[1]
    want = [uniform]
    if adaptive_sampling:
        for _, t in robust.estimates[:-1]:
            status, counts, _, _ = AO.plan(w, h, t[:, :, 0].reshape(-1), share, n)
            assert status == AO.PLAN_OK
            want.append(counts)
    assert len(adaptive.plans) == len(want)
    for i, (got, counts) in enumerate(zip(adaptive.plans, want)):
        assert got.tobytes() == counts.tobytes(), ("plan %d" % i, got, counts)
    assert any(p.tobytes() != uniform.tobytes() for p in adaptive.plans) == adaptive_sampling
    film = gather.tristimulus_buffer
    assert film.any()
    with pytest.raises(ValueError):
        R.render_robust_to_error(scene, plot, gather, robust, adaptive, n, m - 1, 0.5)
    # the first estimate waits for min_observations where that is more than M
    robust.clear()
    robust.start()
    R.render_robust_to_error(scene, plot, gather, robust, adaptive, n, batches, -1.0, min_observations=5, uniform_share=share, seed=3,
                             adaptive_sampling=False)
    assert [k for k, _ in robust.estimates] == [5, 6]


def test_the_command_line_writes_both_images_and_the_map_and_leaves_the_output_alone(tmp_path, capsys):
    """64-path batches, one wave's worth.  --robust-error-map alone estimates once at the end; --robust-target-error ends the run at the
    first estimate that meets it; either way --output is what --robust alone writes after that many batches."""
    out, robust, grey, plain = (str(tmp_path / name) for name in ("image.ppm", "robust.ppm", "map.ppm", "plain.ppm"))
    common = ["--width", "64", "--height", "36", "--photons-per-batch", "64", "--quiet", "--scene", "glass"]
    head = b"P6\n64 36\n255\n"
    CLI.main(common + ["--batches", "15", "--output", out, "--robust", robust, "--robust-error-map", grey])
    told = capsys.readouterr().out
    assert "robust estimate: 15 of 15 batches, relative_error" in told and "no target" in told and "error map: wrote %s" % grey in told, told
    assert "robust film: 15 buckets, gain 1, 15 observations of 960 paths" in told, told
    CLI.main(common + ["--batches", "15", "--output", plain, "--robust", str(tmp_path / "other.ppm")])
    assert "robust estimate" not in capsys.readouterr().out
    images = [open(p, "rb").read() for p in (out, robust, grey, plain)]
    assert all(data.startswith(head) and len(data) == len(head) + 64 * 36 * 3 for data in images)
    assert images[0] == images[3], "--output with --robust-error-map and without"
    assert any(images[0][len(head):])
    pixels = np.frombuffer(images[2][len(head):], np.uint8).reshape(36, 64, 3)
    assert pixels.max() == 255 and (pixels[:, :, 0] == pixels[:, :, 1]).all() and (pixels[:16, :16] == pixels[0, 0]).all()
    # a target that the first estimate meets: the run ends after one batch per bucket
    CLI.main(common + ["--batches", "15", "--output", out, "--robust", robust, "--robust-buckets", "3", "--robust-target-error", "1e30"])
    told = capsys.readouterr().out
    assert "robust estimate: 3 of 15 batches" in told and "target 1e+30 reached" in told, told
    assert "robust film: 3 buckets, gain 1, 3 observations of 192 paths" in told, told
    CLI.main(common + ["--batches", "3", "--output", plain, "--robust", str(tmp_path / "other.ppm"), "--robust-buckets", "3"])
    capsys.readouterr()
    assert open(out, "rb").read() == open(plain, "rb").read(), "--output with --robust-target-error and without, 3 batches"
    # a target that none meets, with the adaptive batches
    CLI.main(["--width", "64", "--height", "36", "--photons-per-batch", "4096", "--quiet", "--batches", "4", "--output", out, "--robust", robust,
              "--robust-buckets", "3", "--robust-target-error", "0", "--robust-adaptive", "--robust-error-map", grey])
    told = capsys.readouterr().out
    assert "robust estimate: 4 of 4 batches" in told and "target 0 not reached" in told and "error map: wrote" in told, told
    assert "robust film: 3 buckets, gain 1, 4 observations of 16384 paths" in told, told
