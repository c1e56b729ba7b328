"""The relight film without a GPU: rl_relight_gains_black_body against its numpy restatement, the re-trace identity the feature
rests on (on the CPU oracles), and the routing of objects to groups.  The oracle is tests/_relight_oracle.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _relight_cases as RC
import _relight_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402

RL_E_INVALID = -1


# ---- the gains helper ---------------------------------------------------------------------------------------------------------------

LIGHTS = [(6504.0, 1.0, 3200.0, 0.5), (3200.0, 0.5, 6504.0, 1.0), (7600.0, 0.6, 5000.0, 0.6), (1000.0, 1.0, 20000.0, 3.0),
          (20000.0, 3.0, 1000.0, 1e-3), (2856.0, 1e3, 2856.0, 1e-3), (800.0, 1.0, 6504.0, 1.0)]


@pytest.mark.parametrize("n_nodes", [2, 5, 81, 401])
def test_the_gains_are_the_restatements_within_one_unit_of_the_last_place(n_nodes):
    """The only freedom is the last bit of a double exp, which reaches an f32 result as at most one unit of its last place (the lights
    keep get_intensity a normal f32 at every node: a quotient of subnormal numbers magnifies their last bit)."""
    for light in LIGHTS:
        got, want = R.relight_gains_black_body(n_nodes, *light), RO.gains_black_body(n_nodes, *light)
        assert got.dtype == np.float32 and got.shape == (n_nodes,)
        assert np.isfinite(want).all() and (want > 0).all(), light
        worst = int(RO.ulps(got, want).max())
        print("%d nodes, %r: %d ulp" % (n_nodes, light, worst))
        assert worst <= 1, (light, worst)


def test_the_gains_are_exactly_one_where_nothing_changes_and_zero_where_the_light_gave_nothing():
    for kelvins, intensity in ((6504.0, 1.0), (3200.0, 0.5), (1000.0, 7.0), (20000.0, 1e-3)):
        assert (R.relight_gains_black_body(81, kelvins, intensity, kelvins, intensity) == 1.0).all()
    # 60 K: at every visible wavelength the spectrum is below the smallest f32, get_intensity is 0, and so is the gain
    cold = R.relight_gains_black_body(81, 60.0, 1.0, 6504.0, 1.0)
    assert cold.tobytes() == bytes(4 * 81) and RO.gains_black_body(81, 60.0, 1.0, 6504.0, 1.0).tobytes() == bytes(4 * 81)
    # twice the intensity is twice the gain, bit for bit (a power of two)
    assert (R.relight_gains_black_body(81, 6504.0, 1.0, 3200.0, 1.0) == 2 * R.relight_gains_black_body(81, 6504.0, 1.0, 3200.0, 0.5)).all()


def test_the_gains_helper_refuses_what_the_header_says():
    out = np.full(401, 7.0, np.float32)
    P = out.ctypes.data_as(C.c_void_p)
    call = _lib.lib.rl_relight_gains_black_body
    last = lambda: _lib.lib.rl_last_error().decode()
    assert call(81, 6504.0, 1.0, 3200.0, 0.5, None) == RL_E_INVALID and "null output" in last()
    for n_nodes in (0, 1, 402, 0xFFFFFFFF):
        assert call(n_nodes, 6504.0, 1.0, 3200.0, 0.5, P) == RL_E_INVALID and "n_nodes %d outside" % n_nodes in last()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        for slot in range(4):
            args = [6504.0, 1.0, 3200.0, 0.5]
            args[slot] = bad
            assert call(81, *args, P) == RL_E_INVALID and "finite and greater than 0" in last(), (bad, slot)
    assert (out == 7.0).all()                                           # a refused call writes nothing
    with pytest.raises(R.RlError):
        R.relight_gains_black_body(81, 6504.0, 1.0, 0.0, 1.0)


# ---- the re-trace identity ------------------------------------------------------------------------------------------------------------

def test_a_relit_film_is_the_retraced_film_within_the_bound_the_data_gives():
    """Description A is the demo, B the demo with the sun sphere at 3200 K and half the intensity.  The same 2^16 paths at 64 x 36
    by _path_oracle: they differ in nothing but the value of the paths that ended on the sun, and A's relight film mixed with that
    light's gains under the CIE table is B's XYZ film within _relight_oracle.retrace_bound."""
    samples, a, b = RC.retrace()
    for field in ("segments", "object", "end"):
        assert (a[field] == b[field]).all(), field
    differs = a["value"].view(np.uint32) != b["value"].view(np.uint32)
    on_sun = a["object"] == RC.SUN
    assert differs.sum() > 1000 and (on_sun[differs]).all()
    assert (a["end"][on_sun] == 1).all() and ((a["object"] != RO.NONE) == (a["end"] == 1)).all()
    gap, bound, data, rounding, retraced = RC.retrace_figures()
    lit = retraced.sum(axis=1) > 0
    on = bound > 0
    print("%d lit pixels; largest gap %.3e = %.3e of the image maximum, %.4f of the bound; the data term is %.2f of the bound on average"
          % (lit.sum(), gap.max(), gap.max() / retraced.max(), (gap[on] / bound[on]).max(), (data[on] / bound[on]).mean()))
    assert lit.sum() > 1000
    assert (gap <= bound).all(), (int((gap > bound).sum()), float((gap[on] / bound[on]).max()))
    assert (gap[~on] == 0).all()
    # the README's figures are the ones this computes (tools/relight_gain.py writes them)
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "relight_retrace.json")))
    assert recorded["paths"] == RC.RETRACE["n"] and recorded["lit_pixels"] == int(lit.sum())
    assert recorded["largest_gap_of_image_maximum"] == pytest.approx(gap.max() / retraced.max(), rel=1e-3)
    assert recorded["largest_gap_of_bound"] == pytest.approx((gap[on] / bound[on]).max(), rel=1e-3)


# ---- group routing ------------------------------------------------------------------------------------------------------------------

def test_the_group_cubes_and_what_drop_removed_add_up_to_the_one_group_cube():
    """The demo's three lights routed to group 0, group n_groups - 1 and RL_RELIGHT_DROP: per element the terms of the cubes and of
    the dropped light's own cube are the one-group cube's, so their counts add exactly and their f64 sums up to f64 rounding."""
    c = RC.RETRACE
    w, h, n_nodes = c["w"], c["h"], 81
    samples, a, _ = RC.retrace()
    objs, _, _ = RC.demo_descriptions()
    lights = np.nonzero(objs["material_kind"] == RO.BLACK_BODY)[0]
    assert len(lights) == 3 and lights[0] == RC.SUN
    everything = RO.splat(w, h, n_nodes, 1, samples, a, RO.groups_of(objs, 1))
    for n_groups in (2, 3, 16):
        table = np.full(len(objs), RO.DROP, np.uint8)
        table[lights[0]], table[lights[1]] = 0, n_groups - 1
        only = np.full(len(objs), RO.DROP, np.uint8)
        only[lights[2]] = 0
        film, k, s, exact = RO.splat(w, h, n_nodes, n_groups, samples, a, table)
        dropped = RO.splat(w, h, n_nodes, 1, samples, a, only)
        assert film[0].any() and film[n_groups - 1].any() and dropped[0].any()
        assert not film[1:n_groups - 1].any()
        assert (k.sum(axis=0) + dropped[1][0] == everything[1][0]).all()
        total = exact.sum(axis=0) + dropped[3][0]
        assert (np.abs(total - everything[3][0]) <= (everything[1][0] + 4) * 2.0 ** -52 * everything[2][0]).all()   # (k adds in f64 on each side)
        assert np.allclose(s.sum(axis=0) + dropped[2][0], everything[2][0], rtol=1e-12, atol=0)


def test_relight_groups_numbers_the_black_bodies_in_scan_order():
    objs, _ = R.builtin_scene_desc(R.SCENE_DEMO)
    for n_groups in (1, 2, 3, 16):
        table = R.relight_groups(objs, n_groups)
        assert table.dtype == np.uint8 and (table == RO.groups_of(objs, n_groups)).all()
        assert list(table[[0, 4, 5]]) == [min(i, n_groups - 1) for i in range(3)]
        assert (np.delete(table, [0, 4, 5]) == R.RL_RELIGHT_DROP).all()
    for n_groups in (0, 17):
        with pytest.raises(ValueError):
            R.relight_groups(objs, n_groups)


def test_the_oracle_skips_what_the_contract_skips():
    w, h, n_groups = 16, 9, 3
    table = RC.table(n_groups)
    samples, results = RC.synthetic_records(w, h)
    on = RO.kept(samples, results, table)
    assert 100 < on.sum() < len(on) - 100
    obj = results["object"]
    assert not on[obj >= RC.N_OBJECTS].any() and (obj == RO.NONE).any() and (obj == RC.N_OBJECTS).any() and (obj == RC.N_OBJECTS - 1).any()
    assert not on[results["value"] == 0].any() and not on[~np.isfinite(samples["ray"]["wavelength"])].any()
    assert not on[~np.isfinite(samples["x"]) | ~np.isfinite(samples["y"])].any()
    inside = obj < RC.N_OBJECTS
    assert not on[inside][table[obj[inside]] == RO.DROP].any()
    assert not RO.splat(w, h, 5, n_groups, samples[~on], results[~on], table)[0].view(np.uint32).any()
    assert RO.splat(w, h, 5, n_groups, samples, results, table)[0].any()
