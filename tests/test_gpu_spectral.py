"""SpectralUnit on the device (rl_spectral_unit_*) against the CPU restatement (tests/_spectral_oracle.py): the splat of photons the
oracle and no renderer make, host and device forms, onto a film that holds something; plot() of trace units beside a plot unit; the
projection bit for bit into a prefilled gather unit; the 81-node identity with the XYZ film on rendered paths; every argument
failure in the documented order; the ordering of project against the film and dst; the command line.  A GPU fault ends the run:
nothing here provokes one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _image_cases as IC
import _spectral_cases as SC
import _spectral_oracle as SO
from _device_arrays import _upload
from _image_cases import same_bits

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5
COMBINATIONS = SC.combinations()
combo_id = lambda c: "%dx%dx%d" % c


def _err():
    return _lib.lib.rl_last_error()


def _held(got, want_film, k, s, exact, what):
    bad, excess = SO.violations(got, want_film, k, s, exact)
    print("%s: up to %d terms on an element, %d violations, worst excess %.3e" % (what, int(k.max()), len(bad), excess))
    assert not len(bad), (what, bad[:8], excess)


def _photon_sets(w, h):
    return (("demo", SC.demo_photons(w, h, 4096)), ("synthetic", SC.synthetic_photons(w, h)))


# ---- the splat ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBINATIONS, ids=combo_id)
def test_the_splat_matches_the_oracle_in_both_forms_and_adds_onto_the_film(combo):
    w, h, n_nodes = combo
    for name, photons in _photon_sets(w, h):
        want = SO.splat(w, h, n_nodes, photons)
        assert np.count_nonzero(want[0])
        host, dev = R.SpectralUnit(w, h, n_nodes), R.SpectralUnit(w, h, n_nodes)
        assert host.download().tobytes() == bytes(4 * w * h * n_nodes)          # created zeroed
        before = R.spectral_launches()
        host.plot_photons(photons)
        dev.plot_photons(_upload(np.ascontiguousarray(photons)))
        assert R.spectral_launches() == (before[0] + 2, before[1])
        first = host.download()
        assert first.shape == (n_nodes, h, w) and first.dtype == np.float32
        _held(first, *want, "%s, host form" % name)
        _held(dev.download(), *want, "%s, device form" % name)
        # a second call adds onto what the film holds: the other set, in the other form, onto the host unit's film
        other = [p for n, p in _photon_sets(w, h) if n != name][0]
        host.plot_photons(_upload(np.ascontiguousarray(other)))
        _held(host.download(), *SO.splat(w, h, n_nodes, other, onto=first), "%s, then the other set" % name)
        # n = 0 launches nothing; clear() zeroes
        before = R.spectral_launches()
        host.plot_photons(photons[:0])
        assert R.spectral_launches() == before
        host.clear()
        assert host.download().tobytes() == bytes(4 * w * h * n_nodes)


def test_photons_that_are_skipped_leave_a_cleared_film_all_zero_bits():
    w, h, n_nodes = 64, 36, 81
    ph = SC.synthetic_photons(w, h)
    skipped = ph[~SO.kept(ph)].copy()
    outside = ph[SO.kept(ph) & np.isfinite(ph["probability"])].copy()     # (an infinite probability times r = 0 is a NaN)
    outside["wavelength"] = np.resize(np.array([375.0, 785.0, 0.0, 1e4, -3e38, 3e38, 374.99, 785.01, 1.1e10, -1.1e10], np.float32), len(outside))
    for photons in (skipped, outside):
        assert len(photons) > 100
        for form in (lambda a: a, lambda a: _upload(np.ascontiguousarray(a))):
            unit = R.SpectralUnit(w, h, n_nodes)
            unit.plot_photons(form(photons))
            assert unit.download().tobytes() == bytes(4 * w * h * n_nodes)


def test_the_host_form_stages_in_chunks_of_2_to_the_20():
    w, h, n_nodes = 64, 36, 81
    ph = SC.synthetic_photons(w, h)
    ph = ph[SO.kept(ph) & np.isfinite(ph["probability"])]
    photons = np.resize(ph, (1 << 20) + 4097)
    unit = R.SpectralUnit(w, h, n_nodes)
    before = R.spectral_launches()
    unit.plot_photons(photons)
    assert R.spectral_launches() == (before[0] + 2, before[1])
    _held(unit.download(), *SO.splat(w, h, n_nodes, photons), "2^20 + 4097 photons")


def test_the_device_form_refuses_host_memory():
    unit = R.SpectralUnit(8, 8, 3)
    photons = np.ascontiguousarray(SC.synthetic_photons(8, 8)[:64])
    before = R.spectral_launches()
    rc = _lib.lib.rl_spectral_unit_plot_photons_device(unit.handle, photons.ctypes.data_as(C.c_void_p), 64)
    assert rc == RL_E_INVALID and b"device memory" in _err() and b"rl_spectral_unit_plot_photons" in _err()
    assert R.spectral_launches() == before and not unit.download().any()


# ---- plot(trace_units) ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _demo_scene():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return R.Scene(objs, cam)


def _xyz_held(got, w, h, photons, what):
    want, k, s, exact = IC.splat(w, h, photons)
    bad, excess = IC.splat_violations(got, want, k, s, exact)
    assert not len(bad), (what, bad[:8], excess)


def test_plot_of_trace_units_is_plot_photons_of_their_photons_beside_a_plot_unit():
    w, h, n, n_nodes = 64, 36, 1 << 14, 81
    scene = _demo_scene()
    traces = [R.TraceUnit(i, w, h, n_photons=n) for i in range(2)]
    for i, t in enumerate(traces):
        t.render(scene, seed=1, stream=0, first_path_index=i * n)
    photons = np.concatenate([t.mapped_photons for t in traces])
    assert (photons["probability"] != 0).sum() > 1000
    before_plot, spectral, after_plot = R.PlotUnit(0, w, h), R.SpectralUnit(w, h, n_nodes), R.PlotUnit(1, w, h)
    launches = R.spectral_launches()
    before_plot.plot(traces)
    spectral.plot(traces)
    after_plot.plot(traces)
    assert R.spectral_launches() == (launches[0] + 2, launches[1])
    _held(spectral.download(), *SO.splat(w, h, n_nodes, photons), "plot of two trace units")
    _xyz_held(before_plot.tristimulus_buffer, w, h, photons, "the plot unit plotted before")
    _xyz_held(after_plot.tristimulus_buffer, w, h, photons, "the plot unit plotted after")
    # the trace units render on as ever: the next render's photons, plotted again, add onto the film
    first = spectral.download()
    traces[0].render(scene, seed=1, stream=0, first_path_index=2 * n)
    spectral.plot(traces[:1])
    _held(spectral.download(), *SO.splat(w, h, n_nodes, traces[0].mapped_photons, onto=first), "the next render")
    # an empty list does nothing; a missing trace unit is RL_E_STATE, as for rl_plot_unit_plot
    spectral.plot([])
    arr = (C.c_void_p * 1)(None)
    assert _lib.lib.rl_spectral_unit_plot(spectral.handle, arr, 1) == RL_E_STATE and b"trace unit" in _err()
    assert _lib.lib.rl_plot_unit_plot(before_plot.handle, arr, 1) == RL_E_STATE


# ---- the projection -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBINATIONS, ids=combo_id)
def test_the_projection_matches_the_oracle_bit_for_bit_into_a_prefilled_dst(combo, tmp_path):
    """(The projection kernel has no LDS, so there is nothing stale to read: no poisoned-LDS variant.)"""
    w, h, n_nodes = combo
    unit, dst = R.SpectralUnit(w, h, n_nodes), R.GatherUnit(w, h)
    path = str(tmp_path / "aa.raw")
    with open(path, "wb") as f:
        f.write(b"\xaa" * (w * h * 24))
    for kind in SC.FILMS:
        film = SC.film(kind, w, h, n_nodes)
        unit.upload(film)
        assert same_bits(unit.download(), film)
        for name in SC.MATRICES:
            matrix = SC.matrix(name, n_nodes)
            dst.load(path)
            assert dst._download()[1].tobytes() == b"\xaa" * (w * h * 12)
            before = R.spectral_launches()
            assert unit.project(matrix, dst) is dst
            assert R.spectral_launches() == (before[0], before[1] + 1)
            got, comp = dst._download()
            want = SO.project(film, matrix)
            assert same_bits(got, want), (kind, name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            assert comp.tobytes() == bytes(comp.nbytes)
        assert same_bits(unit.download(), film)       # the film is left as it was
    # what the library's own observer gives is what the oracle's restatement gives
    assert same_bits(R.spectral_observer_cie1931(n_nodes), SC.matrix("cie", n_nodes))


def test_at_81_nodes_the_cie_projection_is_the_plot_units_film_on_rendered_paths():
    """2^16 paths of the demo scene at 64 x 36, un-fused, into a plot unit and a spectral unit: _spectral_oracle.identity_bound counts
    k - 1 adds in any order on each side, so it holds the two devices' films to each other as it holds the two oracles'."""
    w, h, n = 64, 36, 1 << 16
    trace = R.TraceUnit(0, w, h, n_photons=n)
    trace.render(_demo_scene(), seed=1, stream=0, first_path_index=0)
    plot, spectral, dst = R.PlotUnit(0, w, h), R.SpectralUnit(w, h, 81), R.GatherUnit(w, h)
    plot.plot([trace])
    spectral.plot([trace])
    table = R.spectral_observer_cie1931(81)
    got = spectral.project(table, dst).tristimulus_buffer
    want = plot.tristimulus_buffer
    bound, s, k, nodes = SO.identity_bound(w, h, trace.mapped_photons, table)
    d = np.abs(got.astype(np.float64) - want)
    on = s > 0
    print("up to %d terms and %d nodes on a pixel; largest difference %.3f of the bound, %.2f 2^-24 S"
          % (k.max(), nodes.max(), (d[on] / bound[on]).max(), (d[on] / (SO.U * s[on])).max()))
    assert on.sum() > 1000 and (d <= bound).all()
    # and the tonemap takes the projected gather unit as any other
    tonemap = R.TonemapUnit(w, h)
    tonemap.tonemap(dst)
    assert tonemap.rgb_buffer.any()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------

def test_every_argument_failure_in_the_documented_order():
    w, h, n_nodes = 9, 8, 5
    L = _lib.lib
    unit = R.SpectralUnit(w, h, n_nodes)
    film = SC.film("loguniform", w, h, n_nodes)
    unit.upload(film)
    matrix = np.ascontiguousarray(SC.matrix("signed", n_nodes))
    M = matrix.ctypes.data_as(C.c_void_p)
    mark = np.full((h, w, 3), 3.5, np.float32)

    def marked(w_, h_):
        plot, gather = R.PlotUnit(0, w_, h_), R.GatherUnit(w_, h_)
        plot.upload(np.full((h_, w_, 3), 3.5, np.float32))
        gather.accumulate(plot)
        return gather
    dst = marked(w, h)
    launches = R.spectral_launches()
    for args in ((None, None, None), (None, M, dst.handle), (unit.handle, None, dst.handle), (unit.handle, M, None)):
        assert L.rl_spectral_unit_project(*args) == RL_E_INVALID and b"null" in _err()
    # a dst of another size: RL_E_STATE, and nothing is written -- a NULL matrix comes first
    for other in (marked(w, h + 1), marked(w + 1, h), marked(h, w)):
        assert L.rl_spectral_unit_project(unit.handle, None, other.handle) == RL_E_INVALID
        assert L.rl_spectral_unit_project(unit.handle, M, other.handle) == RL_E_STATE and b"does not match" in _err()
        t, c = other._download()
        assert (t == 3.5).all() and not c.any()
    if R.device_count() > 1:
        elsewhere = R.GatherUnit(w, h, device=1)
        assert L.rl_spectral_unit_project(unit.handle, M, elsewhere.handle) == RL_E_STATE and b"does not match" in _err()
        trace = R.TraceUnit(0, w, h, n_photons=64, device=1)
        assert L.rl_spectral_unit_plot(unit.handle, (C.c_void_p * 1)(trace.handle), 1) == RL_E_STATE
    # the splats and the copies: a NULL unit, then NULL photons with n > 0, before any device work; n = 0 does nothing
    photons = _upload(np.ascontiguousarray(SC.synthetic_photons(w, h)[:64]))
    P = C.c_void_p(photons.data_ptr())
    for fn in (L.rl_spectral_unit_plot_photons, L.rl_spectral_unit_plot_photons_device):
        assert fn(None, None, 5) == RL_E_INVALID and b"null spectral unit" in _err()
        assert fn(unit.handle, None, 5) == RL_E_INVALID and b"null photon buffer" in _err()
        assert fn(unit.handle, None, 0) == 0 and fn(unit.handle, P, 0) == 0
    assert L.rl_spectral_unit_plot(None, None, 0) == RL_E_INVALID and L.rl_spectral_unit_plot(unit.handle, None, 2) == RL_E_INVALID
    assert L.rl_spectral_unit_download(unit.handle, None) == RL_E_INVALID and L.rl_spectral_unit_upload(unit.handle, None) == RL_E_INVALID
    t, c = dst._download()
    assert same_bits(t, mark.reshape(-1, 3)) and not c.any() and R.spectral_launches() == launches
    assert same_bits(unit.download(), film)
    # create: the order of its checks, and the limits themselves
    for args, code, word in (((0, 4, 81), RL_E_INVALID, "zero"), ((4, 0, 1), RL_E_INVALID, "zero"), ((4, 4, 1), RL_E_INVALID, "n_nodes"),
                             ((65536, 65536, 402), RL_E_INVALID, "n_nodes"), ((65536, 65536, 2), RL_E_INVALID, "RL_MAX_PIXELS")):
        with pytest.raises(R.RlError) as e:
            R.SpectralUnit(*args)
        assert e.value.code == code and word in str(e.value), (args, str(e.value))
    for args in ((1, 1, 2), (1, 1, 401), (3, 2, R.RL_SPECTRAL_MAX_NODES)):
        small = R.SpectralUnit(*args)
        assert small.download().shape == (args[2], args[1], args[0]) and not small.download().any()
    with pytest.raises(R.RlError) as e:
        R.SpectralUnit(4, 4, 3, device=R.device_count())
    assert e.value.code == RL_E_INVALID


# ---- ordering -------------------------------------------------------------------------------------------------------------------------

def test_project_sees_the_splat_before_it_and_overwrites_what_is_queued_on_dst():
    w, h, n_nodes = 64, 36, 81
    photons = SC.demo_photons(w, h, 4096)
    table = R.spectral_observer_cie1931(n_nodes)
    unit, dst = R.SpectralUnit(w, h, n_nodes), R.GatherUnit(w, h)
    # work queued on dst's stream immediately before: an accumulate of a film of 7s, which the projection must come after
    plot = R.PlotUnit(0, w, h)
    plot.upload(np.full((h, w, 3), 7.0, np.float32))
    unit.clear()                                   # (queued on the film)
    unit.plot_photons(photons)
    dst.accumulate(plot)
    unit.project(table, dst)
    got, comp = dst._download()
    film = unit.download()
    assert film.any() and same_bits(got, SO.project(film, table)) and not comp.any()
    _held(film, *SO.splat(w, h, n_nodes, photons), "the splat before the projection")
    # a clear queued on the film immediately before the projection is seen too
    unit.clear()
    unit.project(table, dst)
    assert dst._download()[0].tobytes() == bytes(w * h * 12)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_the_command_line_saves_a_cube_whose_cie_projection_is_an_image(tmp_path):
    out, cube_path = str(tmp_path / "image.png"), str(tmp_path / "cube.npy")
    CLI.main(["--spectral", cube_path, "--output", out, "--width", "64", "--height", "36", "--batches", "1", "--photons-per-batch", "65536",
              "--quiet"])
    cube = np.load(cube_path)
    assert cube.shape == (81, 36, 64) and cube.dtype == np.float32
    assert np.isfinite(cube).all() and (cube >= 0).all() and cube.any()
    unit, dst, tonemap = R.SpectralUnit(64, 36, 81), R.GatherUnit(64, 36), R.TonemapUnit(64, 36)
    unit.upload(cube)
    tonemap.tonemap(unit.project(R.spectral_observer_cie1931(81), dst))
    assert tonemap.rgb_buffer.any()
    # the cube is the film of the paths the image shows: paths 0 .. 65535 of stream 0, seed 1
    trace = R.TraceUnit(0, 64, 36, n_photons=65536)
    trace.render(_demo_scene(), seed=1, stream=0, first_path_index=0)
    _held(cube, *SO.splat(64, 36, 81, trace.mapped_photons), "the command line's cube")
