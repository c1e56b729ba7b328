"""The robust film's CPU restatement (tests/_robust_oracle.py): the estimator's properties on synthetic sums, the vector code against
the per-pixel loop, the recorded gain figures (tests/golden/robust_gain.json) and the command line's rules.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import _robust_cases as RC
import _robust_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: F401,E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import __main__ as CLI  # noqa: E402

INF = float("inf")


def _state(means, n, w=1, h=1):
    """A state whose bucket means are `means` (M, 3) on every pixel: sums = mean * n (exact for the small integers used here)."""
    means = np.asarray(means, np.float64)
    sums = np.broadcast_to((means * np.asarray(n, np.float64)[:, None])[:, :, None, None], means.shape + (h, w)).copy()
    return sums, list(n), len(n)


def _bits(a):
    return np.asarray(a).tobytes()


def test_equal_buckets_are_pooled_untrimmed():
    for m in RC.BUCKETS:
        film, trim, stats = RO.resolve(_state([[2.0, 3.0, 5.0]] * m, [8] * m, 3, 2), gain=INF)
        assert not trim.any() and stats["trimmed_pixels"] == 0 and stats["untrimmable_pixels"] == 0
        assert _bits(film) == _bits(np.broadcast_to(np.float32([2.0, 3.0, 5.0]) * np.float32(8 * m), (2, 3, 3)))
        assert (stats["observations"], stats["paths"], stats["buckets"]) == (m, 8 * m, m)


def test_one_bucket_times_1000_is_dropped():
    for m in RC.BUCKETS:
        means = [[1.0 + 0.25 * (j % 3), 2.0 + 0.125 * j, 0.5]for j in range(m)]
        means[m // 2] = [1000.0, 2000.0, 500.0]
        # (M = 3: G <= 2 / 3, so gain 1 gives v = G M / 2 < 1 and never trims; the smallest M needs a larger gain)
        film, trim, stats = RO.resolve(_state(means, [4] * m), gain=2.0 if m == 3 else 1.0)
        c = int(trim[0, 0])
        assert c >= 1 and stats["largest_trim"] == c and stats["trimmed_buckets"] == 2 * c
        order = sorted(range(m), key=lambda j: (means[j][1], j))
        kept = order[c:m - c]
        assert m // 2 not in kept
        want = np.mean([means[j] for j in kept], axis=0) * 4 * m
        assert np.allclose(film[0, 0], want, rtol=1e-6, atol=0)
        assert film[0, 0, 1] < 4 * m * 3.0 + 4 * m * 0.125 * m           # the firefly's 2000 is gone


def test_gain_zero_and_max_trim_zero_give_the_plain_film():
    rng = np.random.default_rng(3)
    for m in RC.BUCKETS:
        state = RC.edge_state(5, 4, m)
        for kw in (dict(gain=0.0), dict(gain=1.0, max_trim=0), dict(gain=INF, max_trim=0)):
            film, trim, stats = RO.resolve(state, **kw)
            assert not trim.any() and stats["trimmed_buckets"] == 0
        n = [int(x) for x in rng.integers(1, 9, size=m)]
        means = rng.integers(0, 64, size=(m, 3)).astype(np.float64)
        film, trim, _ = RO.resolve(_state(means, n), gain=0.0)
        assert np.allclose(film[0, 0], means.mean(axis=0) * sum(n), rtol=1e-6)
        # equal n: the sum a gather unit would hold
        film, _, _ = RO.resolve(_state(means, [4] * m), gain=0.0)
        assert np.allclose(film[0, 0], (means * 4).sum(axis=0), rtol=1e-6)


def test_gain_infinity_gives_the_median_or_the_middle_pair():
    for m in RC.BUCKETS:
        rng = np.random.default_rng(m)
        y = rng.permutation(m).astype(np.float64) + 1.0
        means = np.stack([y * 2.0, y, y * 0.5], axis=1)
        film, trim, _ = RO.resolve(_state(means, [2] * m), gain=INF)
        assert trim[0, 0] == (m - 1) // 2
        middle = (m + 1) / 2.0                                           # the median of 1 .. M, or the mean of the middle pair
        assert _bits(film[0, 0]) == _bits(np.float32([middle * 2.0, middle, middle * 0.5]) * np.float32(2 * m))
        assert RO.resolve(_state(means, [2] * m), gain=INF, max_trim=1)[1][0, 0] == 1


def test_exact_ties_in_y_are_decided_by_bucket_number():
    """All Y equal but the first bucket's, which is larger: with c = 1 the dropped pair is bucket 1 (the lowest (key, j) among the
    tied) and bucket 0 (the largest key), and the distinct X of the tied buckets shows which of them went."""
    m = 5
    means = [[100.0, 9.0, 0.0], [1.0, 3.0, 0.0], [2.0, 3.0, 0.0], [4.0, 3.0, 0.0], [8.0, 3.0, 0.0]]
    film, trim, _ = RO.resolve(_state(means, [1] * m), gain=INF, max_trim=1)
    assert trim[0, 0] == 1
    assert _bits(film[0, 0]) == _bits(np.float32([(2.0 + 4.0 + 8.0) / 3.0 * 5.0, 15.0, 0.0]))
    means = means[1:] + means[:1]                                        # the large one last: bucket 0 is the lowest of the tied
    film, trim, _ = RO.resolve(_state(means, [1] * m), gain=INF, max_trim=1)
    assert _bits(film[0, 0]) == _bits(np.float32([(2.0 + 4.0 + 8.0) / 3.0 * 5.0, 15.0, 0.0]))
    film, trim, _ = RO.resolve(_state(means, [1] * m), gain=INF, max_trim=2)
    assert trim[0, 0] == 2 and _bits(film[0, 0]) == _bits(np.float32([4.0 * 5.0, 15.0, 0.0]))   # ranks 2: bucket 2 of 1 2 4 8 | 100


@pytest.mark.parametrize("key", [float("nan"), INF, -INF, -1.0])
def test_a_key_that_is_not_finite_or_negative_makes_the_pixel_untrimmable(key):
    m = 5
    means = [[1.0, 1.0, 1.0]] * 3 + [[1.0, key, 1.0], [50.0, 900.0, 2.0]]
    film, trim, stats = RO.resolve(_state(means, [2] * m, 2, 1), gain=INF)
    assert not trim.any() and stats["untrimmable_pixels"] == 2 and stats["trimmed_pixels"] == 0
    assert _bits(film[0, 0, [0, 2]]) == _bits(np.float32([54.0 / 5.0 * 10.0, 6.0 / 5.0 * 10.0]))   # pooled in bucket order
    y = film[0, 0, 1]
    assert math.isnan(y) if key != key else (y == key * np.float32(1) if abs(key) == INF else y == np.float32((903.0 + key) / 5.0 * 10.0))


def test_an_all_zero_pixel_is_plus_zero_and_untrimmable():
    film, trim, stats = RO.resolve(_state([[0.0, 0.0, 0.0]] * 4, [3] * 4), gain=INF)
    assert _bits(film) == bytes(12) and not trim.any() and stats["untrimmable_pixels"] == 1
    film, trim, stats = RO.resolve(_state([[0.0, -0.0, -0.0]] * 4, [3] * 4), gain=INF)
    assert _bits(film) == bytes(12) and stats["untrimmable_pixels"] == 1


def test_unequal_path_counts():
    """Buckets of 1, 10 and 100 paths and one of 2^33 + 1 with the same mean are equal buckets; the result is mean * N."""
    n = [1, 10, 100, (1 << 33) + 1, 7]
    film, trim, stats = RO.resolve(_state([[0.5, 0.25, 2.0]] * 5, n), gain=INF)
    assert not trim.any() and stats["paths"] == sum(n)
    assert _bits(film[0, 0]) == _bits((np.float64([0.5, 0.25, 2.0]) * np.float64(sum(n))).astype(np.float32))
    # the outlier is judged by its mean, not its sum: 100 paths at mean 1 against 1 path at mean 50
    film, trim, _ = RO.resolve(_state([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [50.0, 50.0, 50.0]], [100, 100, 1]), gain=INF)
    assert trim[0, 0] == 1 and _bits(film[0, 0]) == _bits(np.float32([201.0] * 3))


@pytest.mark.parametrize("m", RC.BUCKETS)
def test_the_vector_code_is_the_per_pixel_loop(m):
    w, h = 17, 5
    states = [RC.edge_state(w, h, m)]
    state = RO.new_state(w, h, m)
    for xyz, n, bucket in RC.schedule("unequal", w, h, m):
        state = RO.observe(state, xyz, n, bucket)
    states.append(state)
    for sums, n, k in states:
        for gain, max_trim in RC.PARAMS:
            film, trim, stats = RO.resolve((sums, n, k), gain, max_trim)
            untrimmable = 0
            for y in range(h):
                for x in range(w):
                    out, c, u = RO.resolve_pixel(sums[:, :, y, x], n, gain, max_trim)
                    assert _bits(np.float32(out)) == _bits(film[y, x]) and c == trim[y, x], (x, y, gain, max_trim, out, film[y, x])
                    untrimmable += u
            assert stats["untrimmable_pixels"] == untrimmable
            assert stats["trimmed_pixels"] == int((trim > 0).sum()) and stats["trimmed_buckets"] == 2 * int(trim.sum())
            assert stats["largest_trim"] == int(trim.max()) <= min(max_trim, (m - 1) // 2)


def test_observe_takes_the_buckets_in_turn_and_leaves_its_input_alone():
    w, h, m = 3, 1, 4
    state = RO.new_state(w, h, m)
    for i in range(2 * m + 1):
        xyz = np.full((h, w, 3), i + 1, np.float32)
        before = state[0].copy()
        new = RO.observe(state, xyz, 10 + i)
        assert _bits(state[0]) == _bits(before)
        state = new
    assert state[1] == [10 + 14 + 18, 11 + 15, 12 + 16, 13 + 17] and state[2] == 9
    assert state[0][0, 0, 0, 0] == 1 + 5 + 9 and state[0][3, 2, 0, 2] == 4 + 8
    state = RO.observe(state, np.ones((h, w, 3), np.float32), 1, bucket=2)
    assert state[1][2] == 29 and state[2] == 10


def test_the_recorded_gain_figures_are_the_oracles():
    """The smallest configuration of tests/golden/robust_gain.json (tools/robust_gain.py) derived again: the same figures exactly."""
    import _mirror as M
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "robust_gain.json")))
    assert table["config"] == RO.GAIN
    assert [(r["scene"], r["batches"], r["paths_per_batch"]) for r in table["runs"]] == [(["demo", "glass"][s], b, n) for s, b, n in RO.GAIN_CONFIGS]
    which, batches, n = RO.GAIN_CONFIGS[0]
    objs, cam = M.builtin_desc(which)
    got = RO.gain_figures(objs, cam, batches, n)
    got["scene"] = "glass"
    assert got == table["runs"][0], (got, table["runs"][0])
    for run in table["runs"]:
        assert sum(run["trim_histogram"]) == 64 * 36 and run["stats"]["buckets"] == 15


def test_the_command_lines_rules_for_robust(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "15", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base)
    assert a.robust is None and a.robust_buckets is None and a.robust_gain is None
    a = CLI.parse_args(base + ["--robust", "r.png"])
    assert (a.robust, a.robust_buckets, a.robust_gain) == ("r.png", 15, 1.0)
    a = CLI.parse_args(base + ["--robust", "r.png", "--robust-buckets", "3", "--robust-gain", "inf", "--direct"])
    assert (a.robust_buckets, a.robust_gain, a.direct) == (3, INF, True)
    assert CLI.parse_args(base + ["--robust", "r.png", "--robust-gain", "0"]).robust_gain == 0.0
    for args, words in ((["--robust-buckets", "5"], ("--robust-buckets", "--robust")),
                        (["--robust-gain", "2"], ("--robust-gain", "--robust")),
                        (["--robust", "r.png", "--target-error", "0.1", "--adaptive", "--min-observations", "4"], ("--adaptive", "--robust")),
                        (["--robust", "r.png", "--resume"], ("--resume", "--robust")),
                        (["--robust", "r.png", "--unfused"], ("--unfused", "--robust")),
                        (["--robust", "r.png", "--concurrency", "2"], ("--concurrency", "--robust")),
                        (["--robust", "r.png", "--spectral", "c.npy"], ("--spectral", "--robust")),
                        (["--robust", "r.png", "--batches", "14"], ("--batches", "--robust-buckets")),
                        (["--robust", "r.png", "--robust-buckets", "16"], ("--batches", "--robust-buckets")),
                        (["--robust", "r.png", "--robust-buckets", "2"], ("--robust-buckets", "3 .. 32")),
                        (["--robust", "r.png", "--batches", "40", "--robust-buckets", "33"], ("--robust-buckets", "3 .. 32")),
                        (["--robust", "r.png", "--robust-gain", "-1"], ("--robust-gain",)),
                        (["--robust", "r.png", "--robust-gain", "nan"], ("--robust-gain",))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + args)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), (args, told)
