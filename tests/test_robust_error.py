"""The robust film's noise estimate on the CPU (tests/_robust_error_oracle.py): the vector code against the per-pixel loop, the
estimate against the error unit's and the resolve's where they must agree, what a firefly does to it, its calibration at a fixed
trim, the recorded figures (tests/golden/robust_error_gain.json) and the command line's rules.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import _error_oracle as EO
import _robust_error_cases as EC
import _robust_error_oracle as REO
import _robust_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: F401,E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import __main__ as CLI  # noqa: E402

INF = float("inf")


def _bits(a):
    return np.asarray(a).tobytes()


@pytest.mark.parametrize("m", EC.BUCKETS)
def test_the_vector_code_is_the_per_pixel_loop(m):
    w, h = 17, 5
    sums, n, k = EC.edge_state(w, h, m)
    for gain, max_trim in EC.PARAMS:
        px = REO.pixels((sums, n, k), gain, max_trim)
        stats, se, tiles, trim = REO.estimate((sums, n, k), gain, max_trim)
        for y in range(h):
            for x in range(w):
                p = y * w + x
                got = REO.estimate_pixel(sums[:, 1, y, x], n, gain, max_trim)
                want = (px["se"][p], px["ay"][p], px["var"][p], px["f"][p])
                assert [_bits(np.float64(a)) for a in got[:4]] == [_bits(np.float64(a)) for a in want], (x, y, gain, max_trim, got, want)
                assert _bits(np.float32(got[0])) == _bits(se[y, x])
                assert got[4] | (0x80 if got[5] else 0) == trim[y, x], (x, y, gain, max_trim, got, trim[y, x])
        assert int((trim & 0x7F).max()) <= min(max_trim, (m - 2) // 2)
        assert (stats["observations"], stats["paths"], stats["tiles_x"], stats["tiles_y"]) == (k, sum(n), 2, 1)
        assert tiles.shape == (1, 2, 2)


@pytest.mark.parametrize("m", EC.BUCKETS)
def test_gain_zero_with_equal_counts_is_the_error_units_estimate(m):
    """One observation per bucket, equal n, nothing trimmed: v = d N / (k - 1) algebraically.  f32 rounding is 6e-8 and the f64
    cancellation of Q - S^2 / N below 1e-12 on these buffers: 1e-5 relative wherever both are > 0."""
    w, h, n = 33, 17, 4096
    rng = np.random.default_rng(m)
    robust, plain = RO.new_state(w, h, m), EO.new_state(w, h)
    for _ in range(m):
        xyz = EC.noisy(rng, w, h, n)
        robust = RO.observe(robust, xyz, n)
        plain = EO.observe(plain, xyz, n)
    _, se, _, trim = REO.estimate(robust, gain=0.0)
    want = EO.pixels(plain)[0]
    both = (se > 0) & (want > 0)
    assert both.sum() > w * h // 2 and not (trim & 0x7F).any()
    assert (np.abs(se[both].astype(np.float64) - want[both]) <= 1e-5 * want[both]).all()


@pytest.mark.parametrize("m", EC.BUCKETS)
def test_where_the_trims_agree_the_bytes_and_the_film_are_the_resolves(m):
    state = EC.edge_state(33, 17, m)
    same = 0
    for gain, max_trim in EC.PARAMS:
        film, c_resolve, _ = RO.resolve(state, gain, max_trim)
        px = REO.pixels(state, gain, max_trim)
        trim = REO.estimate(state, gain, max_trim)[3]
        agree = (px["c"] == c_resolve.reshape(-1))
        same += int(agree.sum())
        assert ((trim & 0x7F).reshape(-1)[agree] == c_resolve.reshape(-1)[agree]).all()
        assert _bits(px["f"].astype(np.float32)[agree]) == _bits(film[:, :, 1].reshape(-1)[agree])
        # they differ only where the resolve's cap is beyond the estimate's: odd M at full trim
        assert (~agree).sum() == 0 or (m % 2 == 1 and (c_resolve.reshape(-1)[~agree] == (m - 1) // 2).all())
    assert same > 0


def test_odd_m_at_full_trim_keeps_three_buckets_and_three_never_trims():
    for m in (3, 5, 15, 31):
        y = np.random.default_rng(m).permutation(m).astype(np.float64) + 1.0
        sums = np.zeros((m, 3, 1, 1))
        sums[:, 1, 0, 0] = y * 2.0
        px = REO.pixels((sums, [2] * m, m), gain=INF)
        assert px["c"][0] == (m - 3) // 2 and m - 2 * px["c"][0] == 3
        assert RO.resolve((sums, [2] * m, m), gain=INF)[1][0, 0] == (m - 1) // 2
    for m in (4, 32):
        sums = np.zeros((m, 3, 1, 1))
        sums[:, 1, 0, 0] = np.arange(m) + 1.0
        assert REO.pixels((sums, [1] * m, m), gain=INF)["c"][0] == (m - 2) // 2       # even M: the middle pair
    for gain, max_trim in EC.PARAMS:
        assert not (REO.estimate(EC.edge_state(17, 5, 3), gain, max_trim)[3] & 0x7F).any()


@pytest.mark.parametrize("m", [4, 15, 32])
def test_a_firefly_in_every_pixel_stops_inflating_the_estimate(m):
    """Bucket 0 times 1000 in each of 2,000 pixels: se under gain 1 is below half of se under gain 0 at every pixel, and the median
    ratio is below 0.02 (computed in numpy beforehand: worst 0.24, 0.21, 0.18; medians 0.003 to 0.005)."""
    state = EC.firefly_state(m)
    trimmed, plain = REO.pixels(state, gain=1.0)["se"].astype(np.float64), REO.pixels(state, gain=0.0)["se"].astype(np.float64)
    ratio = trimmed / plain
    print("M = %d: worst ratio %.4f, median %.5f" % (m, ratio.max(), np.median(ratio)))
    assert (plain > 0).all() and (ratio < 0.5).all()
    assert np.median(ratio) < 0.02


@pytest.mark.parametrize("draw", sorted(EC.DRAWS))
@pytest.mark.parametrize("m,c", EC.CALIBRATION)
def test_at_a_fixed_trim_the_variance_is_calibrated(m, c, draw):
    """gain infinity and max_trim = c fix the trim; over 20,000 i.i.d. pixels the mean of var over the empirical variance of the
    trimmed means lies in [0.9, 1.15] (over three seeds beforehand: 0.975 to 1.051)."""
    state = EC.iid_state(m, EC.DRAWS[draw])
    px = REO.pixels(state, gain=INF, max_trim=c)
    fixed = px["c"] == c
    assert fixed.mean() > 0.999                                   # (an all-equal or all-zero pixel would not trim)
    trimmed_mean = px["f"][fixed] / np.float64(m)                 # n[j] = 1: N = M
    ratio = px["var"][fixed].mean() / trimmed_mean.var()
    print("M = %d, c = %d, %s: mean var / empirical variance %.4f" % (m, c, draw, ratio))
    assert 0.9 <= ratio <= 1.15


def test_the_recorded_figures_are_the_oracles():
    """The smallest configuration of tests/golden/robust_error_gain.json (tools/robust_error_gain.py) derived again: the same figures
    exactly."""
    import _mirror as M
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "robust_error_gain.json")))
    assert table["config"] == REO.GAIN
    assert [(r["scene"], r["batches"], r["paths_per_batch"]) for r in table["runs"]] == [(["demo", "glass"][s], b, n) for s, b, n in REO.GAIN_CONFIGS]
    which, batches, n = REO.GAIN_CONFIGS[0]
    objs, cam = M.builtin_desc(which)
    got = REO.gain_figures(objs, cam, batches, n)
    got["scene"] = "glass"
    assert got == table["runs"][0], (got, table["runs"][0])
    for run in table["runs"]:
        assert run["tiles"] == 12 and 0 <= run["firefly_tiles"] <= 12
        for name in ("plain", "robust"):
            assert math.isfinite(run[name]["relative_error"]) and run[name]["relative_error"] > 0


def test_the_command_lines_rules_for_the_robust_estimate(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "15", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base + ["--robust", "r.png"])
    assert (a.robust_target_error, a.robust_adaptive, a.robust_error_map) == (None, False, None)
    a = CLI.parse_args(base + ["--robust", "r.png", "--robust-target-error", "0.05"])
    assert (a.robust_target_error, a.robust_adaptive, a.robust_error_map) == (0.05, False, None)
    a = CLI.parse_args(base + ["--robust", "r.png", "--robust-target-error", "0", "--robust-adaptive", "--robust-error-map", "m.png",
                               "--robust-buckets", "3", "--robust-gain", "2"])
    assert (a.robust_target_error, a.robust_adaptive, a.robust_error_map, a.robust_buckets, a.robust_gain) == (0.0, True, "m.png", 3, 2.0)
    assert CLI.parse_args(base + ["--robust", "r.png", "--robust-error-map", "m.ppm"]).robust_error_map == "m.ppm"
    for args, words in ((["--robust-target-error", "0.1"], ("--robust-target-error", "needs --robust PATH")),
                        (["--robust-adaptive"], ("--robust-adaptive", "needs --robust PATH")),
                        (["--robust-error-map", "m.png"], ("--robust-error-map", "needs --robust PATH")),
                        (["--robust", "r.png", "--robust-adaptive"], ("--robust-adaptive", "--robust-target-error")),
                        (["--robust", "r.png", "--robust-adaptive", "--robust-error-map", "m.png"], ("--robust-adaptive", "--robust-target-error")),
                        (["--robust", "r.png", "--robust-target-error", "-1"], ("--robust-target-error", ">= 0")),
                        (["--robust", "r.png", "--robust-target-error", "nan"], ("--robust-target-error", ">= 0")),
                        (["--robust", "r.png", "--direct", "--robust-target-error", "0.1"], ("--robust-target-error", "--direct")),
                        (["--robust", "r.png", "--direct", "--robust-target-error", "0.1", "--robust-adaptive"], ("--direct",)),
                        (["--robust", "r.png", "--direct", "--robust-error-map", "m.png"], ("--robust-error-map", "--direct")),
                        (["--robust", "r.png", "--robust-target-error", "0.1", "--robust-adaptive", "--photons-per-batch", str(1 << 32)],
                         ("--robust-adaptive", "--photons-per-batch")),
                        # the refusals from before the estimate stay as they were
                        (["--robust", "r.png", "--target-error", "0.1"], ("--target-error", "--robust")),
                        (["--robust", "r.png", "--error-map", "e.png"], ("--error-map", "--robust")),
                        (["--robust", "r.png", "--target-error", "0.1", "--adaptive", "--min-observations", "4"], ("--adaptive", "--robust")),
                        (["--robust", "r.png", "--robust-target-error", "0.1", "--target-error", "0.1"], ("--target-error", "--robust")),
                        (["--robust", "r.png", "--robust-error-map", "m.png", "--error-map", "e.png"], ("--error-map", "--robust")),
                        (["--robust", "r.png", "--robust-target-error", "0.1", "--batches", "14"], ("--batches", "--robust-buckets"))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + args)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), (args, told)
