"""Adaptive sampling (rl_adaptive_unit_*) without a GPU: the library's plan rule and per-sample arithmetic, compiled for the host
(tests/adaptive_host), against their numpy restatement (tests/_adaptive_oracle.py) bit for bit; the plan's properties on their own;
one check that does not come from the new text (a one-cell film against rl_scene_camera_rays' oracle); and the two kernels'
resources from the device compile."""
import math

import numpy as np
import pytest

import _adaptive_cases as AC
import _adaptive_oracle as AO
import _rng_width as RW
from _device_build import kernels  # noqa: F401  (a fixture)

SHARE = AC.UNIFORM_SHARE


def _both(w, h, g, share, n):
    """The host compile's plan and the numpy rule's, asserted equal bit for bit; returns the numpy one."""
    status, counts, weights, total = AO.plan(w, h, g, share, n)
    h_status, h_counts, h_weights, h_cells, h_total = AO.host_plan(w, h, g, share, n)
    assert h_status == status, (w, h, n, status, h_status)
    assert h_total == total or (math.isnan(h_total) and math.isnan(total))
    if status == AO.PLAN_OK:
        assert h_counts.tobytes() == counts.tobytes() and h_weights.tobytes() == weights.tobytes(), (w, h, n)
        assert h_cells.tobytes() == AO.cells(w, h)[0].astype(np.float32).tobytes()
    return status, counts, weights


def _properties(w, h, g, share, n, counts, weights):
    q = AO.shares(w, h, g, share)[0]
    _, a = AO.cells(w, h)
    area = float((w - 1) * (h - 1))
    assert int(counts.astype(np.uint64).sum()) == n                                   # the sum is exact
    assert (counts >= 1).all()
    assert (np.abs(counts.astype(np.float64) - np.float64(n) * q) < 1.0).all()       # floor plus largest remainder
    ratio = counts.astype(np.float64) * weights.astype(np.float64) / a                # c_t w_t / a_t = n / A: unbiased
    assert (np.abs(ratio - n / area) <= 2.0 ** -23 * (n / area)).all()


@pytest.mark.parametrize("name", AC.IMPORTANCE)
@pytest.mark.parametrize("film", AC.FILMS, ids=lambda f: "%dx%d" % f)
def test_the_plan_is_the_numpy_rule_bit_for_bit_and_has_its_properties(film, name):
    w, h = film
    g = AC.importance(name, w, h)
    n_min = AC.smallest_n(w, h, g, SHARE)
    print("%d x %d, %s: the smallest n is %d" % (w, h, name, n_min))
    # (between n_min and 1 / min q_t a plan may be refused again -- the largest remainder is not monotone in n; from there on every
    # floor is at least 1)
    n_sure = int(math.ceil(1.0 / AO.shares(w, h, g, SHARE)[0].min())) + 1
    assert n_min <= n_sure
    for n in (n_min, n_sure, 3 * n_sure + 1, AC.N_MAX):
        status, counts, weights = _both(w, h, g, SHARE, n)
        assert status == AO.PLAN_OK, (n, status)
        _properties(w, h, g, SHARE, n, counts, weights)
    if n_min > 1:        # one below: a tile would get nothing
        assert _both(w, h, g, SHARE, n_min - 1)[0] == AO.PLAN_EMPTY_TILE
    if name in ("null", "all_zero"):     # G == 0 means uniform
        assert _both(w, h, g, SHARE, n_min)[1].tobytes() == AO.plan(w, h, None, 1.0, n_min)[1].tobytes()


@pytest.mark.parametrize("film", AC.FILMS, ids=lambda f: "%dx%d" % f)
def test_an_importance_sum_that_overflows_is_refused(film):
    w, h = film
    g = AC.overflowing(w, h)
    if g is None:
        g = np.array([np.inf])       # one tile: an infinite entry counts as 0, the plan is the uniform one
        assert _both(w, h, g, SHARE, 5)[1].tolist() == [5]
        return
    assert np.isfinite(g).all()
    assert _both(w, h, g, SHARE, 1 << 24)[0] == AO.PLAN_OVERFLOW


def test_the_cells_tile_the_film_exactly():
    """The cells the library's rule hands to the device (the host compile's, which are f32: exact at these sizes)."""
    for w, h in AC.FILMS + [(17, 49), (1280, 720)]:
        status, _, _, c, _ = AO.host_plan(w, h, None, 1.0, 1 << 24)
        assert status == AO.PLAN_OK
        c = c.astype(np.float64)
        a = (c[:, 1] - c[:, 0]) * (c[:, 3] - c[:, 2])
        tx, ty = AO.tiles_of(w, h)
        assert a.sum() == (w - 1) * (h - 1) and (a > 0).all()                         # exact: quarters of pixels
        rows = c.reshape(ty, tx, 4)
        assert rows[0, 0, 0] == 0 and rows[0, -1, 1] == w - 1 and rows[0, 0, 2] == 0 and rows[-1, 0, 3] == h - 1
        assert (rows[:, 1:, 0] == rows[:, :-1, 1]).all() and (rows[1:, :, 2] == rows[:-1, :, 3]).all()
    last = AO.host_plan(33, 17, None, 1.0, 1 << 16)[3][2]
    assert last[1] - last[0] == 0.5                                                   # width = 16 i + 1


@pytest.mark.parametrize("film", AC.FILMS, ids=lambda f: "%dx%d" % f)
def test_every_weight_of_a_uniform_plan_of_k_areas_is_exactly_one(film):
    w, h = film
    for k in (4, 12, 1024):          # (a corner cell may be a quarter pixel: k a_t is whole for k a multiple of 4)
        n = k * (w - 1) * (h - 1)
        status, counts, weights = _both(w, h, None, SHARE, n)
        assert status == AO.PLAN_OK and (weights == np.float32(1.0)).all()
        assert (counts.astype(np.float64) == k * AO.cells(w, h)[1]).all()


def test_the_one_hot_plan_puts_the_guided_share_on_its_tile():
    w, h = 64, 36
    n = 1 << 16
    status, counts, weights = _both(w, h, AC.importance("one_hot_partial", w, h), SHARE, n)
    assert status == AO.PLAN_OK
    # w_t = (a_t / A) / (c_t / n), and c_t is within 1 of n q_t: 1 / u on the tiles with no importance, (a / A) / (u a / A + 1 - u) on the one
    share_last = AO.cells(w, h)[1][-1] / (63.0 * 35.0)
    want = np.full(len(counts), 1.0 / SHARE)
    want[-1] = share_last / (SHARE * share_last + 1.0 - SHARE)
    assert counts[-1] >= (1 - SHARE) * n
    assert (np.abs(weights / want - 1.0) <= 1.0 / (counts - 1.0) + 2.0 ** -23).all()


# ---- samples ----------------------------------------------------------------------------------------------------------------------

def _demo():
    import _mirror as M
    return M.builtin_desc(0)


@pytest.mark.parametrize("name", ["one_hot_partial", "random"])
@pytest.mark.parametrize("film", AC.SMALL_FILMS, ids=lambda f: "%dx%d" % f)
def test_the_samples_are_the_numpy_positions_inside_their_cells(film, name):
    w, h = film
    objs, cam = _demo()
    g = AC.importance(name, w, h)
    n = AC.smallest_n(w, h, g, SHARE) + 1000
    _, counts, weights = AO.plan(w, h, g, SHARE, n)[:3]
    seed, stream, first = 11, 3, (1 << 32) - n // 2         # the path range carries into the high counter word
    got = AO.HostScene(objs, cam).samples(w, h, counts, weights, seed, stream, first, 0, n)
    tile = AO.tile_of(counts, np.arange(n))
    assert (np.bincount(got["reserved0"], minlength=len(counts)) == counts).all()      # the per-tile counts are c_t
    assert (got["reserved0"] == tile).all() and (got["reserved1"] == weights.view(np.uint32)[tile]).all()
    words = RW.numpy_words(seed, stream, RW.paths_of(first, n), 0)
    cell = AO.cells(w, h)[0][tile]
    px, py, x, y = AO.positions(w, h, cell, AO.closed01(words[:, 1]), AO.closed01(words[:, 2]))
    assert got["x"].tobytes() == x.tobytes() and got["y"].tobytes() == y.tobytes()
    assert ((px >= cell[:, 0]) & (px <= cell[:, 1]) & (py >= cell[:, 2]) & (py <= cell[:, 3])).all()
    wavelength = AO.closed01(words[:, 0]) * np.float32(400.0) + np.float32(380.0)
    assert got["ray"]["wavelength"].tobytes() == wavelength.tobytes()
    # where the splat puts them: plot_pixel's px from x.  px / m1 rounds by 2^-25, - 0.5 by 2^-26, back + 0.5 by 2^-25 (all on values
    # <= 1), * m1 by 2^-24 relative: (2^-25 + 2^-26 + 2^-25 + 2^-24) m1 < 2^-22 m1
    back = (got["x"] * np.float32(0.5) + np.float32(0.5)) * np.float32(w - 1)
    assert (np.abs(back.astype(np.float64) - px) <= 2.0 ** -22 * (w - 1)).all()
    # a window of the plan is the same samples
    part = AO.HostScene(objs, cam).samples(w, h, counts, weights, seed, stream, first, int(counts[0]) + 1, 100)
    assert part.tobytes() == got[int(counts[0]) + 1:int(counts[0]) + 101].tobytes()


def test_on_a_film_of_one_cell_the_samples_are_the_camera_rays_oracles():
    """Independent of the new text: on 16 x 16 the single cell is the whole film, so every sample is rl_scene_camera_rays' sample of
    the same path, up to the few ulps between x = (15 u / 15 - 0.5) 2 and x = 2 u - 1 (AO.whole_film_tolerances)."""
    import _direct_oracle as DO
    objs, cam = _demo()
    n, seed, stream, first = 512, 5, 1, 77
    _, counts, weights = AO.plan(16, 16, None, 1.0, n)[:3]
    got = AO.HostScene(objs, cam).samples(16, 16, counts, weights, seed, stream, first, 0, n)
    want = DO.oracle_camera_samples(objs, cam, 16, 16, seed, stream, first, n)
    tol_xy, tol_dir = AO.whole_film_tolerances(16, cam)
    assert tol_xy < 2e-7 and tol_dir < 1e-5
    assert got["ray"]["wavelength"].tobytes() == want["ray"]["wavelength"].tobytes()
    assert got["ray"]["origin"].tobytes() == want["ray"]["origin"].tobytes()          # the lens and the camera time alone
    for axis in ("x", "y"):
        d = np.abs(got[axis].astype(np.float64) - want[axis].astype(np.float64))
        print("%s: the largest difference is %.3g (bound %.3g)" % (axis, d.max(), tol_xy))
        assert d.max() <= tol_xy
    d = np.abs(got["ray"]["direction"].astype(np.float64) - want["ray"]["direction"].astype(np.float64))
    print("direction: the largest difference is %.3g (bound %.3g)" % (d.max(), tol_dir))
    assert d.max() <= tol_dir
    assert (got["reserved0"] == 0).all() and (got["reserved1"] == weights.view(np.uint32)[0]).all()


def test_the_cpu_run_of_uniform_against_adaptive_and_its_committed_figures():
    """tools/adaptive_gain.py's run in small (2^12 paths a batch, 6 batches, no reference): the CPU restatement of the driver plans
    from the tile map after the warm-up and its films stay unbiased; and the committed figures are the configuration's, and DESIGN.md's."""
    import json
    import os
    import _mirror as M
    objs, cam = M.builtin_desc(0)
    cfg = dict(AO.GAIN, n=1 << 12, warmup=2, budgets=(6,))
    zero = np.zeros((36 * 64, 3))
    uniform, adaptive = AO.cpu_gain(objs, cam, False, zero, cfg)[6], AO.cpu_gain(objs, cam, True, zero, cfg)[6]
    assert uniform != adaptive and all(np.isfinite(v) and v > 0 for v in list(uniform.values()) + list(adaptive.values()))
    assert abs(adaptive["mse"] / uniform["mse"] - 1) < 0.2        # (against zero: the squared image itself, which both estimate)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    golden = json.load(open(os.path.join(root, "tests", "golden", "adaptive_gain.json")))
    assert golden["config"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in AO.GAIN.items()}
    design = open(os.path.join(root, "DESIGN.md")).read()
    for budget, row in golden["budgets"].items():
        for metric, r in row.items():
            assert "%-12.6g %-12.6g %.4f" % (r["uniform"], r["adaptive"], r["ratio"]) in design, (budget, metric)
    assert str(AO.GAIN_TEST_BUDGET) in golden["budgets"]


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def test_both_kernels_keep_to_32_vgprs_without_scratch_or_lds(kernels):
    mine = {n: k for n, k in kernels.items() if "rl_adaptive_" in n}
    assert len(mine) == 2 and any("rl_adaptive_samples_kernel" in n for n in mine) and any("rl_adaptive_splat_kernel" in n for n in mine), sorted(mine)
    for name, k in sorted(mine.items()):
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                                                                                    k["private_segment_fixed_size"]))
        assert k["vgpr_count"] <= 32, (name, k)        # they run beside a resident open trace kernel (tests/test_error.py)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["dynamic_stack"] == 0
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256
