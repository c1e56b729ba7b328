"""The image kernels against the oracle at odd shapes and edge values: exposure + tonemap (rl_exposure_kernel,
rl_tonemap_kernel), the Kahan gather and its clear (rl_gather_kernel), rl_add_kernel, and the splat, un-fused
(rl_plot_kernel) and fused into the trace kernel in plain and open launches.  Shapes, synthetic images, gather states and
the splat bound come from tests/_image_cases.py (proved on the CPU by tests/test_image_cases.py).  Exposure, tonemap,
gather and add are compared bit for bit (NaNs as NaNs); the splat's atomically ordered sums stay within
(k_p - 1) 2^-24 S_p of their exact sum, pixel by pixel, and pixels of at most two terms match the oracle exactly."""
import numpy as np
import pytest

import _image_cases as IC
import _oracle as O

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), O.RlCameraDesc.from_buffer_copy(bytes(cam)))


def _check(ok, what, got, want):
    assert ok, "%s: %s" % (what, IC.first_difference(got, want))


@pytest.mark.parametrize("shape", IC.SHAPES, ids=IC.shape_id)
def test_exposure_and_tonemap_match_the_oracle(shape):
    """PlotUnit.upload -> GatherUnit.accumulate -> TonemapUnit.tonemap of every synthetic class: max_intensity, the float
    sRGB and the bytes are the oracle's bit for bit."""
    w, h = shape
    for cls, make in IC.XYZ_CLASSES.items():
        xyz = make(shape, 1)
        acc, comp = np.zeros_like(xyz), np.zeros_like(xyz)
        O.accumulate(acc, comp, xyz)
        rgb, srgb, mx = O.tonemap(acc, w, h)
        p, g, tm = R.PlotUnit(0, w, h), R.GatherUnit(w, h), R.TonemapUnit(w, h)
        p.upload(xyz)
        g.accumulate(p)
        tm.tonemap(g)
        got_srgb, got_mx = tm.srgb_float()
        what = "%s %s" % (IC.shape_id(shape), cls)
        _check(IC.same_bits(g.tristimulus_buffer, acc), what + " gathered", g.tristimulus_buffer, acc)
        _check(IC.same_bits(np.float32(got_mx), np.float32(mx)), what + " max_intensity", np.float32([got_mx]), np.float32([mx]))
        _check(IC.same_bits(got_srgb, srgb), what + " srgb_float", got_srgb, srgb)
        got_rgb = tm.rgb_buffer
        _check(IC.same_bits(got_rgb, rgb), what + " rgb", got_rgb, rgb)


@pytest.mark.parametrize("shape", [s for s in IC.SHAPES if s != (3840, 2160)], ids=IC.shape_id)
def test_gather_three_accumulations_from_adversarial_states(shape, tmp_path):
    """GatherUnit.load of an adversarial (acc, comp) state, then three accumulate calls: both buffers are O.accumulate's
    bit for bit, and the plot buffer is all (+0) zeros after each, the scalar tail included."""
    w, h = shape
    acc, comp, pxs = IC.kahan_states(shape, 1)
    path = str(tmp_path / "buffer.raw")
    IC.write_gather_raw(path, acc, comp)
    p, g = R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    g.load(path)
    a, c = acc.copy(), comp.copy()
    zeros = np.zeros_like(acc)
    for k, px in enumerate(pxs):
        p.upload(px)
        g.accumulate(p)
        O.accumulate(a, c, px)
        cleared = p.tristimulus_buffer
        _check(IC.same_bits(cleared, zeros), "%s plot buffer after accumulate %d" % (IC.shape_id(shape), k), cleared, zeros)
    got_a, got_c = g.tristimulus_buffer, g.compensation_buffer
    _check(IC.same_bits(got_a, a), IC.shape_id(shape) + " tristimulus", got_a, a)
    _check(IC.same_bits(got_c, c), IC.shape_id(shape) + " compensation", got_c, c)


ADD_SHAPES = [(1, 1), (2, 1), (3, 1), (1, 5), (3, 5), (7, 7), (3, 6), (5, 7), (37, 101), (333, 127), (2049, 1), (1919, 1079)]


@pytest.mark.parametrize("shape", ADD_SHAPES, ids=IC.shape_id)
def test_plot_unit_add_at_odd_shapes(shape):
    w, h = shape
    for cls in ("loguniform", "negative_nonfinite", "denormal"):
        x, y = IC.XYZ_CLASSES[cls](shape, 1), IC.XYZ_CLASSES[cls](shape, 2)
        a, b = R.PlotUnit(0, w, h), R.PlotUnit(1, w, h)
        a.upload(x)
        b.upload(y)
        a.add(b)
        with np.errstate(all="ignore"):
            want = x + y
        got = a.tristimulus_buffer
        _check(IC.same_bits(got, want), "%s %s" % (IC.shape_id(shape), cls), got, want)
        _check(IC.same_bits(b.tristimulus_buffer, y), "%s %s src" % (IC.shape_id(shape), cls), b.tristimulus_buffer, y)


def _assert_splat(got, want, k, s, exact, what):
    bad, excess = IC.splat_violations(got, want, k, s, exact)
    if len(bad):
        i, c = bad[0]
        raise AssertionError("%s: %d pixel components outside the bound (worst excess %.3g); first (%d, %d): got %r want %r "
                             "k_p %d S_p %.6g exact %.9g" % (what, len(bad), excess, i, c, got[i, c], want[i, c], k[i, c], s[i, c], exact[i, c]))


@pytest.mark.parametrize("shape", IC.SPLAT_SHAPES, ids=IC.shape_id)
def test_trace_and_splat_at_odd_shapes(demo, shape):
    """Trace photons bit-exact at the shape; the un-fused plot, the fused render and the open fused launch each within the
    per-pixel bound of the numpy / oracle splat of those photons."""
    scene, oscene = demo
    w, h = shape
    N, seed, stream, first = 1 << 14, 6, 1, 4096
    want_ph, segs = oscene.render(w, h, seed, stream, first, N, threads=8)
    img, k, s, exact = IC.splat(w, h, want_ph)
    assert IC.same_bits(img, O.plot(w, h, want_ph))
    t = R.TraceUnit(0, w, h, n_photons=N)
    t.render(scene, seed=seed, stream=stream, first_path_index=first)
    assert t.mapped_photons.tobytes() == want_ph.tobytes()
    p = R.PlotUnit(0, w, h)
    p.plot([t])
    _assert_splat(p.tristimulus_buffer, img, k, s, exact, IC.shape_id(shape) + " un-fused")
    p_fused = R.PlotUnit(1, w, h)
    t.render_fused(scene, p_fused, N, seed=seed, stream=stream, first_path_index=first)
    t.sync()
    _assert_splat(p_fused.tristimulus_buffer, img, k, s, exact, IC.shape_id(shape) + " fused")
    p_open = R.PlotUnit(2, w, h)
    before = R.variant_launches()
    t.render_fused_begin(scene, p_open, N, seed=seed, stream=stream, first_path_index=first)
    got_open = p_open.tristimulus_buffer                       # a download ends the begun render
    ran = [a - b for a, b in zip(R.variant_launches(), before)]
    assert sum(ran[i] for i in range(len(ran)) if i & 6 == 6) >= 1, ran   # a fused open launch carried it
    _assert_splat(got_open, img, k, s, exact, IC.shape_id(shape) + " open fused")
    assert img.any()


@pytest.mark.parametrize("entry", IC.load_edge_paths(), ids=lambda e: "%d-%d-%d" % tuple(e[:3]))
def test_edge_paths_render_and_splat(demo, entry):
    """A 64-path window around each path of tests/golden/edge_paths.json (x or the y draw at -1 / +1, wavelength at
    380 / 780 nm), at a landscape, a portrait and a one-pixel-wide shape: photons bit-exact, un-fused and fused splats
    within the bound."""
    scene, oscene = demo
    seed, stream, path, flags, reaches = entry
    first = path - path % 64
    for w, h in IC.EDGE_SHAPES:
        what = "%s path %d" % (IC.shape_id((w, h)), path)
        want_ph, _ = oscene.render(w, h, seed, stream, first, 64)
        me = want_ph[path - first]
        if flags & (IC.EDGE_X_MINUS | IC.EDGE_X_PLUS):
            assert abs(me["x"]) == 1.0, what
        if flags & (IC.EDGE_WL_380 | IC.EDGE_WL_780):
            assert me["wavelength"] in (380.0, 780.0), what
        if (w, h) == IC.EDGE_SHAPES[0]:
            assert int(me["probability"] > 0) == reaches, what
        img, k, s, exact = IC.splat(w, h, want_ph)
        t = R.TraceUnit(0, w, h, n_photons=64)
        t.render(scene, seed=seed, stream=stream, first_path_index=first)
        assert t.mapped_photons.tobytes() == want_ph.tobytes(), what
        p = R.PlotUnit(0, w, h)
        p.plot([t])
        _assert_splat(p.tristimulus_buffer, img, k, s, exact, what + " un-fused")
        p_fused = R.PlotUnit(1, w, h)
        t.render_fused(scene, p_fused, 64, seed=seed, stream=stream, first_path_index=first)
        t.sync()
        _assert_splat(p_fused.tristimulus_buffer, img, k, s, exact, what + " fused")
