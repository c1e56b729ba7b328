"""Wavelength importance sampling without a GPU: the table rule of rl_wavelength.h (its g++ compile, tests/wavelength_host) against
the numpy restatement bit for bit, the per-path draw and bin_of likewise, the weight's expectation, the camera path through the CPU
path oracle, the new kernels' resources, and the shape of the recorded gain."""
import json
import os

import numpy as np
import pytest

import _path_oracle as PO
import _scenes as SC
import _wavelength_oracle as WO
from _device_build import kernels  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = WO.M
CIE = WO.cie_importance()


def _messy(n):
    g = np.random.default_rng(n).random(n)
    g[1 % n], g[3 % n], g[5 % n], g[7 % n] = np.nan, np.inf, -1.0, 0.0
    return g


TABLES = {
    "null-81": (None, 81, 1.0), "null-2": (None, 2, 0.3),
    "cie-1": (CIE, 81, 1.0), "cie-0.25": (CIE, 81, 0.25), "cie-0.1": (CIE, 81, 0.1), "cie-0.01": (CIE, 81, 0.01),
    "random-2": (np.random.default_rng(2).random(2), 2, 0.1), "random-3": (np.random.default_rng(3).random(3), 3, 0.1),
    "random-4096": (np.random.default_rng(4096).random(4096), 4096, 0.1),
    "one-hot-0.05": (WO.one_hot(81, 40), 81, 0.05), "one-hot-1e-3": (WO.one_hot(81, 40), 81, 1.0e-3),
    "one-hot-first": (WO.one_hot(81, 0), 81, 1.0e-3), "one-hot-last-4096": (WO.one_hot(4096, 4095), 4096, 1.0e-3),
    "nan-inf-negative-zero": (_messy(81), 81, 0.1), "all-zero": (np.zeros(81), 81, 0.1), "all-nan": (np.full(81, np.nan), 81, 0.1),
    "huge": (np.full(81, 8.0e307), 81, 0.1),       # finite nodes whose sum is not
}


@pytest.mark.parametrize("name", list(TABLES))
def test_the_host_compile_of_the_table_rule_is_the_numpy_rule(name):
    g, n, u = TABLES[name]
    status, q, w = WO.table(g, n, u)
    host_status, host_q, host_w = WO.host_table(g, n, u)
    assert host_status == status, (status, host_status)
    if name == "huge":
        assert status == WO.OVERFLOW
        return
    assert status == WO.OK
    assert host_q.tobytes() == q.tobytes() and host_w.tobytes() == w.tobytes()
    assert q[0] == 380.0 and q[M] == 780.0 and (np.diff(q.astype(np.float64)) > 0).all()
    assert abs(w.astype(np.float64).mean() - 1.0) < 1.0e-7        # the bins' widths sum to 400 nm: exact but for W's rounding
    if g is None or name in ("all-zero", "all-nan", "cie-1", "random-2"):   # (two nodes: one segment, whose density is constant)
        assert (w == 1.0).all() and (np.diff(q) == np.float32(400.0 / M)).all()


def test_the_quantiles_always_increase_for_the_node_counts_the_rule_admits():
    """The rule's second refusal cannot be met through the entry point: a segment is 400 / (n - 1) >= 400 / 4095 nm wide and holds at
    most all M bins at a constant density, so a bin is at least 400 / 4095 / 256 = 3.8e-4 nm, six f32 steps at 780 nm (6.1e-5).  The
    densest tables the rule can make, at a share of 1e-300."""
    for k in (0, 1, 2047, 4094, 4095):
        status, q, w = WO.host_table(WO.one_hot(4096, k), 4096, 1.0e-300)
        assert status == WO.OK and np.diff(q.astype(np.float64)).min() > 3.0e-4, k
        assert WO.table(WO.one_hot(4096, k), 4096, 1.0e-300)[1].tobytes() == q.tobytes()


def test_the_cie_importance_is_the_sum_of_the_three_curves():
    assert WO.host_cie_importance().tobytes() == CIE.tobytes()
    assert CIE.shape == (81,) and abs(CIE.sum() * 5.0 - 3.0 * 106.86) < 0.5      # three curves of equal area, about 106.9 each


@pytest.mark.parametrize("name", ["cie-0.1", "one-hot-1e-3", "null-81"])
def test_the_draw_and_the_bin_found_again_are_numpys(name):
    status, q, w = WO.table(*TABLES[name])
    tab = WO.packed(q, w)
    low = np.arange(1 << 16, dtype=np.uint32)
    v = np.concatenate([(np.uint32(i) << np.uint32(16)) | low for i in (0, 137, 255)] +            # all 2^16 places of three bins
                       [np.arange(M, dtype=np.uint32) << np.uint32(16), (np.arange(M, dtype=np.uint32) << np.uint32(16)) | np.uint32(0xffff)])
    for shift_in in (0, 0xff):        # the low 8 bits of the word are not read
        w0 = (v << np.uint32(8)) | np.uint32(shift_in)
        lam, b, weight = WO.host_draws(tab, w0)
        want = WO.draw(q, w0)
        assert lam.tobytes() == want.tobytes()
        assert (b == WO.bin_of(q, want)).all() and weight.tobytes() == w[b].tobytes()
        assert (lam >= 380.0).all() and (lam <= 780.0).all()
    edges = WO.host_draws(tab, (np.arange(M, dtype=np.uint32) << np.uint32(24)))
    assert edges[0].tobytes() == q[:M].tobytes() and (edges[1] == np.arange(M)).all()      # f = 0: the quantile itself, in its own bin


def _edge_bias_bound(q, w, observer_max):
    """What taking the weight from the wavelength, not from the bin drawn, can cost the expectation.  A draw of bin i whose f32
    wavelength rounds up to Q[i+1] is found in bin i + 1 and carries W[i+1]: that takes (Q[i+1] - Q[i]) * (1 - f) below one f32 step
    of Q[i+1], at most a share step / width + 2^-16 of the bin's 2^16 places.  Summed over the bins, each 1 / M of the draws."""
    step = np.spacing(q[1:M + 1]).astype(np.float64)
    width = np.diff(q.astype(np.float64))
    share = np.minimum(1.0, step / width + 2.0 ** -16)[:M - 1]
    return float((share * np.abs(np.diff(w.astype(np.float64)))).sum() / M * observer_max)


@pytest.mark.parametrize("name", ["cie-0.25", "cie-0.1", "cie-0.01", "one-hot-1e-3"])
def test_the_weighted_observer_keeps_its_expectation(name):
    """E[W(lambda) y-bar(lambda)] under the table's density is the uniform draw's, the trapezoid integral of y-bar over 400 nm: to 1e-5
    relative over every 13th of the 2^24 draws (the draw takes the left end of each of a bin's 2^16 places: 2^-17 of a bin's change).
    The one-hot table at a share of 1e-3 is the stress case of the rule that the weight follows the wavelength: its bins at 585 nm are
    0.039 nm wide, 640 f32 steps, beside one of weight 125 -- measured 1.4e-3 high, inside _edge_bias_bound's 2.9e-3; the CIE tables
    are held to the 1e-5 alone (measured 7e-7 and below)."""
    status, q, w = WO.table(*TABLES[name])
    v = np.arange(0, 1 << 24, 13, dtype=np.uint32)
    lam, b, weight = WO.host_draws(WO.packed(q, w), v << np.uint32(8))
    with open(os.path.join(ROOT, "tests", "golden", "cie1931_xyz.json")) as f:
        ybar = np.asarray(json.load(f)["Y"], dtype=np.float64)
    nodes = np.linspace(380.0, 780.0, 81)
    got = (weight.astype(np.float64) * np.interp(lam.astype(np.float64), nodes, ybar)).mean()
    want = ((ybar[:-1] + ybar[1:]) * 0.5 * 5.0).sum() / 400.0
    bound = _edge_bias_bound(q, w, ybar.max()) / want
    print("%s: E[W y-bar] / integral - 1 = %.3e, edge bound %.3e, bins found elsewhere %.3e" % (name, got / want - 1.0, bound, ((v >> np.uint32(16)) != b).mean()))
    assert abs(got / want - 1.0) < 1.0e-5 + (0.0 if name.startswith("cie") else bound), (got, want, bound)
    assert ((v >> np.uint32(16)) != b).mean() < (1.0e-4 if name.startswith("cie") else 1.0e-3)      # the bin found again is the bin drawn but at a few rounded edges


def test_the_camera_path_through_the_path_oracle():
    """512 paths of the demo scene: the host compile's camera half (ray, x, y, wavelength from the table) traced by the CPU path
    oracle, its value times W[bin_of(wavelength)] in one f32 multiply: the photons of the host compile's whole path, and its segments."""
    objs, cam = SC._scene("demo")
    host = WO.HostScene(np.ascontiguousarray(objs), cam)
    w, h, n, seed, stream, first = 64, 36, 512, 7, 3, 1000
    status, q, wt = WO.table(*TABLES["cie-0.1"])
    tab = WO.packed(q, wt)
    rays, xy = host.camera(w, h, tab, seed, stream, first, n)
    plain_rays, plain_xy = host.camera(w, h, None, seed, stream, first, n)
    assert xy.tobytes() == plain_xy.tobytes() and rays[:, :3].tobytes() == plain_rays[:, :3].tobytes()     # the position and the lens: the same draws
    assert (rays[:, 3] != plain_rays[:, 3]).any()
    results = PO.PathOracle(objs, cam).render_rays(rays[:, 0:3], rays[:, 4:7], rays[:, 3], seed, stream, first)
    photons, segments, values = host.render(w, h, tab, seed, stream, first, n)
    weight = wt[WO.bin_of(q, rays[:, 3])]
    assert photons["wavelength"].tobytes() == rays[:, 3].tobytes()
    assert photons["x"].tobytes() == xy[:, 0].tobytes() and photons["y"].tobytes() == xy[:, 1].tobytes()
    assert values.tobytes() == results["value"].tobytes()
    assert photons["probability"].tobytes() == (results["value"] * weight).astype(np.float32).tobytes()
    assert segments == int(results["segments"].sum()) and (photons["probability"] != 0).sum() > 20
    # without a table the host compile is tests/host_mirror's render
    import _mirror as MI
    want, want_segments = MI.Scene(np.ascontiguousarray(objs).view(MI.O.OBJECT_DTYPE), MI.O.RlCameraDesc.from_buffer_copy(bytes(cam))).render(w, h, seed, stream, first, n)
    got, got_segments, _ = host.render(w, h, None, seed, stream, first, n)
    assert got.tobytes() == want.tobytes() and got_segments == want_segments


def test_the_new_instantiations_keep_their_siblings_resources(kernels):
    """All 24 (stage, fused, open, cyl) combinations exist with the table, within 128 registers (plain) and 120 (open), with no
    scratch, no dynamic stack and the register count of four waves per SIMD (512 / 4)."""
    import re
    seen = set()
    for name, k in kernels.items():
        m = re.match(r"_Z\d+(rl_wl_trace_kernel|rl_wl_trace_open_kernel)ILi([012])ELb([01])ELb([01])E", name)
        if not m:
            continue
        seen.add(m.groups())
        cap = 120 if "open" in m.group(1) else 128
        assert k["vgpr_count"] <= cap and k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
    assert len(seen) == 24, sorted(seen)
    plain = {n: k for n, k in kernels.items() if re.match(r"_Z\d+(rl_trace_kernel|rl_trace_kernel_open)ILi", n)}
    assert len(plain) == 24


def test_the_recorded_gain():
    """tests/golden/wavelength_gain.json (tools/wavelength_gain.py): the uniform draw against the CIE table at u = 0.1 on the CPU, 8, 16
    and 32 batches of 2^16 paths.  Importance sampling lowers the Y relative_error at every budget."""
    with open(os.path.join(ROOT, "tests", "golden", "wavelength_gain.json")) as f:
        gain = json.load(f)
    cfg = gain["config"]
    assert (cfg["w"], cfg["h"], cfg["n"], cfg["seed"], cfg["share"], cfg["n_ref"]) == (64, 36, 1 << 16, 1, 0.1, 1 << 23)
    for budget in ("8", "16", "32"):
        for sampler in ("uniform", "importance"):
            for component in "XYZ":
                row = gain[sampler][budget][component]
                assert set(row) == {"relative_error", "worst_tile_error", "mse"} and all(np.isfinite(v) and v > 0 for v in row.values())
        ratio = gain["importance"][budget]["Y"]["relative_error"] / gain["uniform"][budget]["Y"]["relative_error"]
        assert ratio < 1.0, (budget, ratio)
        assert abs(gain["ratio_relative_error"][budget]["Y"] - ratio) < 1e-12
