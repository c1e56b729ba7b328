"""RelightUnit on the device (rl_relight_unit_*) against the CPU restatement (tests/_relight_oracle.py): the routed splat of records
no renderer makes and of rendered paths, host and device forms, onto a film that holds something; render against its public
composition, and chunked; the mix bit for bit into a prefilled gather unit; the identity with the XYZ film; the re-trace on the
device; every argument failure in the documented order; ordering; the command line.  A GPU fault ends the run: nothing here
provokes one."""
import ctypes as C
import functools

import numpy as np
import pytest

import _relight_cases as RC
import _relight_oracle as RO
import _spectral_oracle as SO
from _device_arrays import _upload
from _image_cases import same_bits

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5
COMBINATIONS = RC.combinations()
combo_id = lambda c: "%dx%dx%dx%d" % c
SEED, STREAM = 1, 0


def _err():
    return _lib.lib.rl_last_error()


def _held(got, want_film, k, s, exact, what):
    bad, excess = SO.violations(got, want_film, k, s, exact)
    print("%s: up to %d terms on an element, %d violations, worst excess %.3e" % (what, int(k.max()), len(bad), excess))
    assert not len(bad), (what, bad[:8], excess)


@functools.lru_cache(maxsize=None)
def _demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return objs, cam, R.Scene(objs, cam)


@functools.lru_cache(maxsize=None)
def _rendered(w, h, n, first=0):
    """(samples, results) of demo paths first .. first + n - 1 by the public host calls, read-only."""
    scene = _demo()[2]
    samples = scene.camera_rays(w, h, SEED, STREAM, first, n)
    results = scene.render_spectral_rays(np.ascontiguousarray(samples["ray"]), SEED, STREAM, first)
    samples.setflags(write=False)
    results.setflags(write=False)
    return samples, results


def _unit(w, h, n_nodes, n_groups, table):
    unit = R.RelightUnit(w, h, n_nodes, n_groups)
    unit.set_groups(table)
    return unit


def _record_sets(w, h, n_groups):
    return (("synthetic", RC.table(n_groups), *RC.synthetic_records(w, h)),
            ("demo", R.relight_groups(_demo()[0], n_groups), *_rendered(w, h, 4096)))


# ---- the routed splat ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBINATIONS, ids=combo_id)
def test_the_splat_matches_the_oracle_in_both_forms_onto_a_film_that_holds_something(combo):
    w, h, n_nodes, n_groups = combo
    onto = RC.film("with_zeros", w, h, n_nodes, n_groups)
    for name, table, samples, results in _record_sets(w, h, n_groups):
        want = RO.splat(w, h, n_nodes, n_groups, samples, results, table, onto=onto)
        assert RO.kept(samples, results, table).sum() > 100 and (table == RO.DROP).any()
        host, dev = _unit(w, h, n_nodes, n_groups, table), _unit(w, h, n_nodes, n_groups, table)
        assert host.download().tobytes() == bytes(4 * w * h * n_nodes * n_groups)          # created zeroed
        host.upload(onto)
        dev.upload(onto)
        before = R.relight_launches()
        host.plot_results(samples, results)
        dev.plot_results(_upload(np.ascontiguousarray(samples)), _upload(np.ascontiguousarray(results)))
        assert R.relight_launches() == (before[0] + 2, before[1], before[2])
        first = host.download()
        assert first.shape == (n_groups, n_nodes, h, w) and first.dtype == np.float32
        _held(first, *want, "%s, host form" % name)
        _held(dev.download(), *want, "%s, device form" % name)
        # n = 0 launches nothing; clear() zeroes
        before = R.relight_launches()
        host.plot_results(samples[:0], results[:0])
        assert _lib.lib.rl_relight_unit_plot_results_device(host.handle, None, None, 0) == 0
        assert R.relight_launches() == before and same_bits(host.download(), first)
        host.clear()
        assert host.download().tobytes() == bytes(4 * w * h * n_nodes * n_groups)


def test_records_that_are_skipped_leave_a_cleared_film_all_zero_bits():
    w, h, n_nodes, n_groups = 33, 17, 81, 3
    table = RC.table(n_groups)
    samples, results = RC.synthetic_records(w, h)
    on = RO.kept(samples, results, table)
    skipped = (np.ascontiguousarray(samples[~on]), np.ascontiguousarray(results[~on]))
    assert len(skipped[0]) > 500
    for reason in (results["value"] == 0, ~np.isfinite(samples["x"]), ~np.isfinite(samples["ray"]["wavelength"]), results["object"] == RO.NONE,
                   results["object"] == RC.N_OBJECTS):
        assert (reason & ~on).any()
    for form in (lambda a: a, _upload):
        unit = _unit(w, h, n_nodes, n_groups, table)
        before = R.relight_launches()
        unit.plot_results(form(skipped[0]), form(skipped[1]))
        assert R.relight_launches() == (before[0] + 1, before[1], before[2])
        assert unit.download().tobytes() == bytes(4 * w * h * n_nodes * n_groups)


# ---- render -------------------------------------------------------------------------------------------------------------------------

def test_render_is_its_public_composition():
    """camera_rays_device, render_rays_device and plot_results_device called here against one render call: the same records, so
    both films are held to the oracle's film of them, and so to each other."""
    w, h, n, n_nodes, n_groups = 64, 36, 1 << 14, 81, 3
    objs, cam, scene = _demo()
    table = R.relight_groups(objs, n_groups)
    samples_dev = _upload(np.zeros(n, R.CAMERA_SAMPLE_DTYPE))
    scene.camera_rays_device(w, h, SEED, STREAM, 0, samples_dev)
    samples = np.zeros(n, R.CAMERA_SAMPLE_DTYPE)
    samples_dev.download(samples)
    rays_dev, results_dev = _upload(np.ascontiguousarray(samples["ray"])), _upload(np.zeros(n, R.PATH_RESULT_DTYPE))
    scene.render_rays_device(rays_dev, results_dev, SEED, STREAM, 0)
    results = np.zeros(n, R.PATH_RESULT_DTYPE)
    results_dev.download(results)
    assert (results["object"] != RO.NONE).sum() > 1000
    composed, rendered = _unit(w, h, n_nodes, n_groups, table), _unit(w, h, n_nodes, n_groups, table)
    composed.plot_results(samples_dev, results_dev)
    before, paths_before = R.relight_launches(), sum(R.path_launches())
    rendered.render(scene, SEED, STREAM, 0, n)
    assert R.relight_launches() == (before[0] + 1, before[1] + 1, before[2]) and sum(R.path_launches()) == paths_before + 1
    want = RO.splat(w, h, n_nodes, n_groups, samples, results, table)
    assert all(want[0][g].any() for g in range(n_groups))
    _held(composed.download(), *want, "the composition")
    _held(rendered.download(), *want, "render")
    assert all(ms > 0 for ms in rendered.launch_ms()[:2])
    # n_paths = 0 does nothing
    before = R.relight_launches()
    rendered.render(scene, SEED, STREAM, 5, 0)
    assert R.relight_launches() == before


def test_render_in_chunks_of_2_to_the_20():
    """2^20 + 65 paths in one call (two chunks) and in two calls split at 2^20 - 1 (one chunk each): two launches of each kind
    either way, and both films within the per-element bound of the oracle's film of the same records."""
    w, h, n_nodes, n_groups, n = 16, 9, 5, 3, (1 << 20) + 65
    objs, cam, scene = _demo()
    table = R.relight_groups(objs, n_groups)
    samples, results = _rendered(w, h, n)
    want = RO.splat(w, h, n_nodes, n_groups, samples, results, table)
    one, two = _unit(w, h, n_nodes, n_groups, table), _unit(w, h, n_nodes, n_groups, table)
    before = R.relight_launches()
    one.render(scene, SEED, STREAM, 0, n)
    assert R.relight_launches() == (before[0] + 2, before[1] + 2, before[2])
    split = (1 << 20) - 1
    two.render(scene, SEED, STREAM, 0, split)
    two.render(scene, SEED, STREAM, split, n - split)
    assert R.relight_launches() == (before[0] + 4, before[1] + 4, before[2])
    _held(one.download(), *want, "one call")
    _held(two.download(), *want, "two calls")


# ---- the mix ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBINATIONS, ids=combo_id)
def test_the_mix_matches_the_oracle_bit_for_bit_into_a_prefilled_dst(combo, tmp_path):
    w, h, n_nodes, n_groups = combo
    unit, dst = R.RelightUnit(w, h, n_nodes, n_groups), R.GatherUnit(w, h)
    path = str(tmp_path / "aa.raw")
    with open(path, "wb") as f:
        f.write(b"\xaa" * (w * h * 24))
    for kind in RC.FILMS:
        film = RC.film(kind, w, h, n_nodes, n_groups)
        unit.upload(film)
        assert same_bits(unit.download(), film)
        for gain_kind in RC.GAINS:
            gains = RC.gains(gain_kind, n_groups, n_nodes)
            for name in RC.MATRICES:
                matrix = RC.matrix(name, n_nodes)
                dst.load(path)
                assert dst._download()[1].tobytes() == b"\xaa" * (w * h * 12)
                before = R.relight_launches()
                assert unit.mix(gains, matrix, dst) is dst
                assert R.relight_launches() == (before[0], before[1], before[2] + 1)
                got, comp = dst._download()
                want = RO.mix(film, gains, matrix)
                assert same_bits(got, want), (kind, gain_kind, name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                assert comp.tobytes() == bytes(comp.nbytes)
        assert same_bits(unit.download(), film)       # the film is left as it was
    assert unit.launch_ms()[2] > 0


def test_all_ones_gains_under_the_cie_table_give_the_plot_units_film_on_rendered_paths():
    """2^16 paths of the demo scene at 64 x 36 into a plot unit (rl_plot_unit_render_samples_device) and, by render, into a one-group
    relight unit: _spectral_oracle.identity_bound holds the mix to the XYZ film."""
    w, h, n = 64, 36, 1 << 16
    objs, cam, scene = _demo()
    samples, results = _rendered(w, h, n)
    plot, unit, dst = R.PlotUnit(0, w, h), _unit(w, h, 81, 1, R.relight_groups(objs, 1)), R.GatherUnit(w, h)
    plot.render_samples_device(scene, _upload(np.ascontiguousarray(samples)), SEED, STREAM, 0)
    unit.render(scene, SEED, STREAM, 0, n)
    table = R.spectral_observer_cie1931(81)
    got = unit.mix(np.ones((1, 81), np.float32), table, dst).tristimulus_buffer
    want = plot.tristimulus_buffer
    bound, s, k, nodes = SO.identity_bound(w, h, RO.photons_of(samples, results), table)
    d = np.abs(got.astype(np.float64) - want)
    on = s > 0
    print("up to %d terms and %d nodes on a pixel; largest difference %.3f of the bound" % (k.max(), nodes.max(), (d[on] / bound[on]).max()))
    assert (on.any(axis=1)).sum() > 1000 and (d <= bound).all()
    assert same_bits(unit.mix(None, table, dst).tristimulus_buffer, got)                  # NULL gains are all-ones gains
    tonemap = R.TonemapUnit(w, h)
    tonemap.tonemap(dst)
    assert tonemap.rgb_buffer.any()


def test_the_relit_film_is_the_retraced_film_on_the_device():
    """tests/test_relight.py's re-trace case with the device's films: scene B is created from the changed description and rendered
    into a plot unit; A's relight film under the library's gains for the sun is held to it by _relight_oracle.retrace_bound."""
    c = RC.RETRACE
    w, h, n, n_groups = c["w"], c["h"], c["n"], 3
    objs, cam, scene_a = _demo()
    changed = objs.copy()
    assert tuple(changed["m"][RC.SUN][:2]) == RC.SUN_FROM
    changed["m"][RC.SUN][:2] = RC.SUN_TO
    scene_b = R.Scene(changed, cam)
    samples, a = _rendered(w, h, n)
    b = scene_b.render_spectral_rays(np.ascontiguousarray(samples["ray"]), SEED, STREAM, 0)
    for field in ("segments", "object", "end"):
        assert (a[field] == b[field]).all(), field
    differs = a["value"].view(np.uint32) != b["value"].view(np.uint32)
    assert differs.sum() > 1000 and (a["object"][differs] == RC.SUN).all()
    plot, dst = R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    plot.render_samples_device(scene_b, _upload(np.ascontiguousarray(samples)), SEED, STREAM, 0)
    table = R.relight_groups(objs, n_groups)
    unit = _unit(w, h, 81, n_groups, table)
    unit.render(scene_a, SEED, STREAM, 0, n)
    gains = np.ones((n_groups, 81), np.float32)
    gains[table[RC.SUN]] = R.relight_gains_black_body(81, *RC.SUN_FROM, *RC.SUN_TO)
    cie = R.spectral_observer_cie1931(81)
    relit = unit.mix(gains, cie, dst).tristimulus_buffer.astype(np.float64)
    retraced = plot.tristimulus_buffer.astype(np.float64)
    bound, data, rounding = RO.retrace_bound(w, h, samples, a, b, RC.SUN, gains[table[RC.SUN]], cie, n_groups)
    gap = np.abs(relit - retraced)
    on = bound > 0
    print("largest gap %.3e = %.3e of the image maximum, %.4f of the bound" % (gap.max(), gap.max() / retraced.max(), (gap[on] / bound[on]).max()))
    assert (retraced.sum(axis=1) > 0).sum() > 1000 and (gap <= bound).all()
    # the sun alone, and everything but the sun: two more slider positions of the same film
    solo = np.zeros_like(gains)
    solo[table[RC.SUN]] = 1.0
    alone = unit.mix(solo, cie, dst).tristimulus_buffer.copy()
    rest = unit.mix(1.0 - solo, cie, dst).tristimulus_buffer.copy()
    assert alone.any() and rest.any() and same_bits(alone, RO.mix(unit.download(), solo, cie))


# ---- arguments, ordering, memory ----------------------------------------------------------------------------------------------------

def test_every_argument_failure_in_the_documented_order():
    w, h, n_nodes, n_groups = 9, 8, 5, 3
    L = _lib.lib
    objs, cam, scene = _demo()
    unit = R.RelightUnit(w, h, n_nodes, n_groups)
    film = RC.film("loguniform", w, h, n_nodes, n_groups)
    unit.upload(film)
    samples, results = (np.ascontiguousarray(a[:64]) for a in RC.synthetic_records(w, h))
    S, P = _upload(samples), _upload(results)
    Sp, Pp = C.c_void_p(S.data_ptr()), C.c_void_p(P.data_ptr())
    launches = R.relight_launches()
    # no table yet: RL_E_STATE from every call that needs one, after its null checks
    for fn in (L.rl_relight_unit_plot_results, L.rl_relight_unit_plot_results_device):
        assert fn(None, Sp, Pp, 5) == RL_E_INVALID and b"null relight unit" in _err()
        assert fn(unit.handle, None, Pp, 5) == RL_E_INVALID and fn(unit.handle, Sp, None, 5) == RL_E_INVALID and b"null sample or result" in _err()
        assert fn(unit.handle, Sp, Pp, 5) == RL_E_STATE and b"no table" in _err()
    assert L.rl_relight_unit_render(unit.handle, scene.handle, 0, 1, 0, 0, 16, 0) == RL_E_STATE and b"no table" in _err()
    # set_groups: a bad entry keeps the previous table
    good = R.relight_groups(objs, n_groups)
    bad = good.copy()
    bad[7] = n_groups
    assert L.rl_relight_unit_set_groups(unit.handle, bad.ctypes.data_as(C.c_void_p), len(bad)) == RL_E_INVALID and b"object 7 has group 3" in _err()
    assert L.rl_relight_unit_render(unit.handle, scene.handle, 0, 1, 0, 0, 16, 0) == RL_E_STATE and b"no table" in _err()
    unit.set_groups(good)
    assert L.rl_relight_unit_set_groups(unit.handle, bad.ctypes.data_as(C.c_void_p), len(bad)) == RL_E_INVALID
    assert L.rl_relight_unit_set_groups(unit.handle, good.ctypes.data_as(C.c_void_p), 0) == RL_E_INVALID and b"n_objects is 0" in _err()
    # render: arguments, (table), range, then the table against the scene
    H, SC_ = unit.handle, scene.handle
    assert L.rl_relight_unit_render(None, SC_, 0, 1, 0, 0, 16, 0) == RL_E_INVALID and L.rl_relight_unit_render(H, None, 0, 1, 0, 0, 16, 0) == RL_E_INVALID
    assert L.rl_relight_unit_render(H, SC_, 9, 1, 0, 0, 16, 0) == RL_E_INVALID and b"fetch" in _err()
    assert L.rl_relight_unit_render(H, SC_, 0, 1, 0, 0, 16, 65537) == RL_E_INVALID and b"max_segments" in _err()
    assert L.rl_relight_unit_render(H, SC_, 0, 1, 0, 2 ** 64 - 17, 16, 0) == RL_E_INVALID and b"2^64 - 1" in _err()
    unit.set_groups(good[:-1])
    assert L.rl_relight_unit_render(H, SC_, 0, 1, 0, 2 ** 64 - 17, 16, 0) == RL_E_INVALID                       # the range before the scene
    assert L.rl_relight_unit_render(H, SC_, 0, 1, 0, 0, 16, 0) == RL_E_STATE and b"objects and the scene" in _err()
    unit.set_groups(good)
    if R.device_count() > 1:
        elsewhere = R.Scene(objs, cam, device=1)
        assert L.rl_relight_unit_render(H, elsewhere.handle, 0, 1, 0, 0, 16, 0) == RL_E_STATE and b"different devices" in _err()
    # the _device form refuses host memory
    rc = L.rl_relight_unit_plot_results_device(H, samples.ctypes.data_as(C.c_void_p), Pp, 64)
    assert rc == RL_E_INVALID and b"device memory" in _err() and b"rl_relight_unit_plot_results" in _err()
    rc = L.rl_relight_unit_plot_results_device(H, Sp, results.ctypes.data_as(C.c_void_p), 64)
    assert rc == RL_E_INVALID and b"device memory" in _err()
    # mix: nulls, then a dst of another size, and nothing is written
    matrix = np.ascontiguousarray(RC.matrix("signed", n_nodes))
    M = matrix.ctypes.data_as(C.c_void_p)

    def marked(w_, h_):
        plot, gather = R.PlotUnit(0, w_, h_), R.GatherUnit(w_, h_)
        plot.upload(np.full((h_, w_, 3), 3.5, np.float32))
        gather.accumulate(plot)
        return gather
    dst = marked(w, h)
    for args in ((None, None, M, dst.handle), (H, None, None, dst.handle), (H, None, M, None)):
        assert L.rl_relight_unit_mix(*args) == RL_E_INVALID and b"null" in _err()
    for other in (marked(w, h + 1), marked(w + 1, h), marked(h, w)):
        assert L.rl_relight_unit_mix(H, None, None, other.handle) == RL_E_INVALID
        assert L.rl_relight_unit_mix(H, None, M, other.handle) == RL_E_STATE and b"does not match" in _err()
        t, c = other._download()
        assert (t == 3.5).all() and not c.any()
    assert L.rl_relight_unit_download(H, None) == RL_E_INVALID and L.rl_relight_unit_upload(H, None) == RL_E_INVALID
    t, c = dst._download()
    assert (t == 3.5).all() and not c.any() and R.relight_launches() == launches
    assert same_bits(unit.download(), film)                                                    # nothing above touched the film
    # create: the order of its checks, and the limits themselves
    for args, word in (((0, 4, 81, 3), "zero"), ((4, 4, 1, 3), "n_nodes"), ((4, 4, 81, 0), "n_groups"), ((4, 4, 81, 17), "n_groups"),
                       ((65536, 65536, 402, 17), "n_nodes"), ((65536, 65536, 2, 17), "n_groups"), ((4096, 4096, 81, 3), "RL_MAX_PIXELS")):
        with pytest.raises(R.RlError) as e:
            R.RelightUnit(*args)
        assert e.value.code == RL_E_INVALID and word in str(e.value), (args, str(e.value))
    for args in ((1, 1, 2, 1), (1, 1, 401, 16), (3, 2, 5, 16)):
        small = R.RelightUnit(*args)
        assert small.download().shape == (args[3], args[2], args[1], args[0]) and not small.download().any()
    with pytest.raises(R.RlError) as e:
        R.RelightUnit(4, 4, 3, 1, device=R.device_count())
    assert e.value.code == RL_E_INVALID


def test_a_unit_gives_back_what_it_took():
    objs, cam, scene = _demo()
    scene.camera_rays(8, 8, 1, 0, 0, 8)                                                          # (the query contexts exist)
    before = R.live_resources() if hasattr(R, "live_resources") else None
    unit = _unit(16, 9, 5, 3, R.relight_groups(objs, 3))
    unit.render(scene, SEED, STREAM, 0, 256)                                                    # takes the scratch
    unit.set_groups(np.resize(R.relight_groups(objs, 3), 5000))                                 # outgrows the table's buffer
    unit.close()
    if before is not None:
        assert R.live_resources() == before


def test_mix_sees_the_splat_and_the_clear_queued_before_it_and_the_film_round_trips():
    w, h, n_nodes, n_groups = 64, 36, 81, 3
    objs, cam, scene = _demo()
    table = R.relight_groups(objs, n_groups)
    samples, results = _rendered(w, h, 4096)
    cie = R.spectral_observer_cie1931(n_nodes)
    gains = RC.gains("signed", n_groups, n_nodes)
    unit, dst = _unit(w, h, n_nodes, n_groups, table), R.GatherUnit(w, h)
    plot = R.PlotUnit(0, w, h)
    plot.upload(np.full((h, w, 3), 7.0, np.float32))
    unit.clear()                                   # (queued on the film)
    unit.plot_results(samples, results)
    dst.accumulate(plot)                           # (queued on dst's stream: the mix comes after it)
    unit.mix(gains, cie, dst)
    got, comp = dst._download()
    film = unit.download()
    assert film.any() and same_bits(got, RO.mix(film, gains, cie)) and not comp.any()
    _held(film, *RO.splat(w, h, n_nodes, n_groups, samples, results, table), "the splat before the mix")
    # download and upload round trip, group-major then node-major
    other = R.RelightUnit(w, h, n_nodes, n_groups)
    other.upload(film)
    assert same_bits(other.download(), film)
    assert same_bits(other.mix(gains, cie, dst)._download()[0], got)
    spectral = R.SpectralUnit(w, h, n_nodes)
    spectral.upload(film[1])                       # plane g * n_nodes + b: group 1's cube is a spectral film
    solo = np.zeros((n_groups, n_nodes), np.float32)
    solo[1] = 1.0
    want = spectral.project(cie, dst)._download()[0].copy()
    # (a gain of 1 leaves the coefficient as it is and the other groups add +0 to the sum: the film and the table are not negative)
    assert same_bits(other.mix(solo, cie, dst)._download()[0], want)
    # a clear queued on the film immediately before the mix is seen too
    unit.clear()
    unit.mix(None, cie, dst)
    assert dst._download()[0].tobytes() == bytes(w * h * 12)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_the_command_line_saves_the_cubes_and_a_relit_image(tmp_path):
    out, cube_path = str(tmp_path / "image.png"), str(tmp_path / "lights.npy")
    CLI.main(["--relight", cube_path, "--light", "0:3200:0.5", "--output", out, "--width", "64", "--height", "36", "--batches", "1",
              "--photons-per-batch", "65536", "--quiet"])
    cube = np.load(cube_path)
    assert cube.shape == (3, 81, 36, 64) and cube.dtype == np.float32
    assert np.isfinite(cube).all() and (cube >= 0).all() and all(cube[g].any() for g in range(3))
    # the cubes are the film of the paths the image shows: paths 0 .. 65535 of stream 0, seed 1
    samples, results = _rendered(64, 36, 65536)
    _held(cube, *RO.splat(64, 36, 81, 3, samples, results, R.relight_groups(_demo()[0], 3)), "the command line's cubes")
    import os
    relit = str(tmp_path / "lights.png")
    assert os.path.getsize(relit) > 100 and open(relit, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
