"""DenoiseUnit.denoise_variance on the device (rl_denoise_unit_denoise_variance) against the CPU restatement
(tests/_denoise_variance_oracle.py) bit for bit: every shape x image class x error class x guide class x parameter set of
tests/_denoise_variance_cases.py, on poisoned LDS and into a prefilled dst, every argument failure in the documented order, the
ordering against work queued on the error unit and on the image's gather unit, the first use of a unit, the quality end to end on
the demo scene, the App's error state and the command line.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import _denoise_oracle as DO
import _denoise_variance_cases as VC
import _denoise_variance_oracle as VO
import _error_oracle as EO
import _lds_poison as LP
from _image_cases import same_bits

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI

RL_E_INVALID, RL_E_STATE = -1, -5


def _err():
    return _lib.lib.rl_last_error()


def _gather_of(xyz, w, h):
    """A fresh gather unit that accumulated `xyz` through a plot unit (0 + x: the buffer holds x), or None for None."""
    if xyz is None:
        return None
    plot, gather = R.PlotUnit(0, w, h), R.GatherUnit(w, h)
    plot.upload(xyz)
    gather.accumulate(plot)
    return gather


def _error_of(state, w, h):
    unit = R.ErrorUnit(w, h)
    unit.upload(*state)
    return unit


@functools.lru_cache(maxsize=None)
def _rig(w, h):
    """(denoise unit, dst gather unit) of a shape: shared by its cases."""
    return R.DenoiseUnit(w, h), R.GatherUnit(w, h)


@functools.lru_cache(maxsize=None)
def _guide_units(kind, w, h):
    """({name: the film the gather unit holds}, {name: the gather unit, or None}) of a guide class and shape: uploaded once."""
    films = VC.guides(kind, w, h)
    units = {k: _gather_of(v, w, h) for k, v in films.items()}
    held = {k: None if u is None else u.tristimulus_buffer.reshape(h, w, 3) for k, u in units.items()}
    return held, units


def _check(unit, dst, image_unit, image, error_unit, state, guide_units, films, params, w, h):
    """One call against the oracle: dst's tristimulus buffer and variance_out bit for bit, dst's compensation buffer all +0, the
    launch counts."""
    plain, mine = R.denoise_launches(), R.denoise_variance_launches()
    got_dst, got_v = unit.denoise_variance(image_unit, error_unit, dst=dst, variance=True, **guide_units, **params)
    assert got_dst is dst
    plain2, mine2 = R.denoise_launches(), R.denoise_variance_launches()
    iterations = params.get("iterations", 0) or DO.ITERATIONS
    assert (plain2[0] - plain[0], plain2[1] - plain[1]) == (1, 0) and (mine2[0] - mine[0], mine2[1] - mine[1]) == (1, iterations)
    got, comp = dst._download()
    want_c, want_v = VO.denoise(image, *state, **films, **params)
    assert same_bits(got, want_c.reshape(h * w, 3)), (params, int((got.view(np.uint32) != want_c.reshape(h * w, 3).view(np.uint32)).sum()))
    assert same_bits(got_v, want_v), (params, int((got_v.view(np.uint32) != want_v.view(np.uint32)).sum()))
    assert comp.tobytes() == bytes(comp.nbytes)


@pytest.mark.parametrize("error", VC.ERRORS)
@pytest.mark.parametrize("kind", VC.IMAGES)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_guide_class_and_parameter_set_matches_the_oracle_bit_for_bit(shape, kind, error):
    w, h = shape
    unit, dst = _rig(w, h)
    image = VC.image(kind, w, h)
    image_unit = _gather_of(image, w, h)
    held = image_unit._download()
    assert same_bits(held[0], image.reshape(-1, 3))
    state = VC.error_state(error, image)
    error_unit = _error_of(state, w, h)
    for guide in VC.GUIDES:
        films, units = _guide_units(guide, w, h)
        inputs = [None if units[k] is None else units[k]._download() for k in ("albedo", "normal", "aux")]
        for name, params in VC.PARAMS.items():
            _check(unit, dst, image_unit, image, error_unit, state, units, films, params, w, h)
        for k, was in zip(("albedo", "normal", "aux"), inputs):
            if was is not None:
                now = units[k]._download()
                assert same_bits(now[0], was[0]) and same_bits(now[1], was[1]), (guide, k)
    # the inputs are left as they were: the image's two buffers, and the error unit's S, Q, k, N
    now = image_unit._download()
    assert same_bits(now[0], held[0]) and same_bits(now[1], held[1])
    s, q, k, n = error_unit.download()
    assert s.tobytes() == state[0].tobytes() and q.tobytes() == state[1].tobytes() and (k, n) == state[2:]


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("shape", VC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_on_poisoned_lds_and_into_a_prefilled_dst(shape, pattern, tmp_path):
    """The C word's fourth component is a variance here, not the live flag: an element outside the image must stage a cleared live
    flag in the albedo word, not only a zero C.  Stale LDS and 0xAA bytes in both of dst's buffers change nothing."""
    w, h = shape
    unit, dst = _rig(w, h)
    path = str(tmp_path / "aa.raw")
    with open(path, "wb") as f:
        f.write(b"\xaa" * (w * h * 24))
    image = VC.image("loguniform", w, h)
    image_unit = _gather_of(image, w, h)
    for guide, error, name in (("random", "matched", "defaults"), ("checker", "checker", "six_passes"), ("no_aux", "huge", "one_pass")):
        films, units = _guide_units(guide, w, h)
        state = VC.error_state(error, image)
        error_unit = _error_of(state, w, h)
        dst.load(path)
        assert dst._download()[1].tobytes() == b"\xaa" * (w * h * 12)
        LP.poison_lds(pattern)
        _check(unit, dst, image_unit, image, error_unit, state, units, films, VC.PARAMS[name], w, h)


def _params(iterations=0, sigmas=(3.0, 0.3, 0.1, 0.2), reserved=(0, 0, 0)):
    return C.byref(_lib.RlDenoiseParams(iterations, *sigmas, (C.c_uint32 * 3)(*reserved)))


def test_every_argument_failure_in_the_documented_order():
    w, h = 9, 8
    fn = _lib.lib.rl_denoise_unit_denoise_variance
    unit = R.DenoiseUnit(w, h)
    mark = np.full((h, w, 3), 3.5, np.float32)
    img, a, n, x, dst = (_gather_of(mark, w, h) for _ in range(5))
    good = _error_of(VC.error_state("matched", mark), w, h)
    s, q, _, paths = VC.error_state("matched", mark)
    k1, k0 = R.ErrorUnit(w, h), R.ErrorUnit(w, h)
    k1.upload(s, q, 1, paths)
    other_g = [R.GatherUnit(w, h + 1), R.GatherUnit(w + 1, h), R.GatherUnit(h, w)]
    other_e = []
    for ow, oh in ((w, h + 1), (w + 1, h), (h, w)):
        e = R.ErrorUnit(ow, oh)
        e.upload(np.ones((oh, ow)), np.ones((oh, ow)), 4, 64)
        other_e.append(e)
    U, I, A, N, X, D, E, E1, E0 = (o.handle for o in (unit, img, a, n, x, dst, good, k1, k0))
    OG, OE = other_g[0].handle, other_e[0].handle
    nan = float("nan")
    out = np.full(w * h, 7.0, np.float32)
    V = out.ctypes.data_as(C.c_void_p)
    counters = (R.denoise_launches(), R.denoise_variance_launches())
    good_state = good.download()

    def refused(args, code, word):
        assert fn(*args) == code and word in _err(), (args, code, word, _err())
        t, c = dst._download()
        assert same_bits(t, mark.reshape(-1, 3)) and not c.any() and (out == 7.0).all()
        assert (R.denoise_launches(), R.denoise_variance_launches()) == counters
    worst = _params(7, (-1.0, nan, 1e-4, 2e3), (1, 0, 0))
    # each failure with everything behind it wrong as well, and alone
    refused((None, I, I, I, I, E1, worst, I, V), RL_E_INVALID, b"null")
    refused((U, None, A, N, X, E, None, D, V), RL_E_INVALID, b"null")
    refused((U, I, A, N, X, E, None, None, V), RL_E_INVALID, b"null")
    refused((U, OG, OG, N, X, None, worst, D, V), RL_E_INVALID, b"null")
    refused((U, I, A, N, X, None, None, D, V), RL_E_INVALID, b"null")
    refused((U, OG, OG, N, X, E1, worst, D, V), RL_E_INVALID, b"iterations")
    refused((U, I, A, N, X, E, _params(7), D, V), RL_E_INVALID, b"iterations")
    refused((U, OG, OG, N, X, E1, _params(6, (3.0, -1.0, 0.1, 0.2), (1, 0, 0)), D, V), RL_E_INVALID, b"sigma_normal")
    for k, name in enumerate((b"sigma_colour", b"sigma_normal", b"sigma_depth", b"sigma_albedo")):
        for bad in (-1.0, nan, 0.99e-3, 1.01e3, float("inf")):
            sig = [3.0, 0.3, 0.1, 0.2]
            sig[k] = bad
            refused((U, I, A, N, X, E, _params(0, sig), D, V), RL_E_INVALID, name)
    refused((U, OG, OG, N, X, E1, _params(reserved=(0, 0, 1)), D, V), RL_E_INVALID, b"reserved")
    refused((U, I, A, N, X, E, _params(reserved=(1, 0, 0)), D, V), RL_E_INVALID, b"reserved")
    refused((U, OG, OG, N, X, E1, None, D, V), RL_E_INVALID, b"distinct")
    for args in ((U, I, I, N, X, E, None, D, V), (U, I, A, A, X, E, None, D, V), (U, I, A, N, N, E, None, D, V), (U, I, A, N, X, E, None, I, V),
                 (U, I, A, N, X, E, None, X, V), (U, I, None, None, None, E, None, I, V)):
        refused(args, RL_E_INVALID, b"distinct")
    # an error unit with fewer than two observations: RL_E_STATE, before any size is looked at
    refused((U, OG, A, N, X, E1, None, D, V), RL_E_STATE, b"observations")
    refused((U, I, A, N, X, E1, None, D, V), RL_E_STATE, b"observations")
    refused((U, I, A, N, X, E0, None, D, V), RL_E_STATE, b"observations")
    # a unit of another size, in every position, the error unit's included: RL_E_STATE
    for o in other_g:
        for pos in range(4):
            args = [U, I, A, N, X, OE, None, D, V]
            args[1 + pos] = o.handle
            refused(tuple(args), RL_E_STATE, b"does not match")
            args[5] = E
            refused(tuple(args), RL_E_STATE, b"does not match")
    for e in other_e:
        refused((U, I, A, N, X, e.handle, None, D, V), RL_E_STATE, b"error unit does not match")
    for o in other_g:
        assert fn(U, I, A, N, X, E, None, o.handle, V) == RL_E_STATE and b"does not match" in _err()
        assert not o.tristimulus_buffer.any() and (R.denoise_launches(), R.denoise_variance_launches()) == counters
    now = good.download()
    assert now[0].tobytes() == good_state[0].tobytes() and now[1].tobytes() == good_state[1].tobytes() and now[2:] == good_state[2:]
    # the limits themselves are accepted, and k = 2
    assert fn(U, I, A, N, X, E, _params(6, (1e-3, 1e3, 0.0, 1e-3)), D, V) == 0 and fn(U, I, None, None, None, E, _params(1, (0.0, 0.0, 0.0, 0.0)), D, None) == 0
    k1.upload(s, q, 2, paths)
    assert fn(U, I, A, N, X, E1, None, D, None) == 0


def test_the_call_waits_for_work_queued_on_the_error_unit_and_on_the_images_gather_unit():
    """Half of the image is observed and accumulated, and the other half is queued -- an observe on the error unit's stream, an
    accumulate on the gather unit's -- immediately before the call: the call sees both sums (halves of floats add up exactly)."""
    w, h = VC.SHAPES[-1]
    unit, dst = _rig(w, h)
    image = VC.image("loguniform", w, h)
    half = image * np.float32(0.5)
    films, units = _guide_units("random", w, h)
    plot, gather, error = R.PlotUnit(0, w, h), R.GatherUnit(w, h), R.ErrorUnit(w, h)
    state = EO.new_state(w, h)
    plot.upload(half)
    error.observe(plot, 4096)
    gather.accumulate(plot)
    plot.upload(half)
    error.observe(plot, 4096)
    gather.accumulate(plot)
    _, got_v = unit.denoise_variance(gather, error, dst=dst, variance=True, **units)
    for _ in range(2):
        state = EO.observe(state, half, 4096)
    want_c, want_v = VO.denoise(image, *state, **films)
    assert same_bits(dst.tristimulus_buffer, want_c.reshape(h * w, 3)) and same_bits(got_v, want_v)
    assert error.download()[2:] == (2, 8192)


def test_the_first_variance_call_of_a_unit_and_a_plain_call_after_it():
    """The two variance planes come with the first variance call, through the unit's ledger, and go with the unit; the plain call
    shares the XYZ scratch and is not disturbed."""
    w, h = 33, 19
    image = VC.image("loguniform", w, h)
    image_unit, dst = _gather_of(image, w, h), R.GatherUnit(w, h)
    films, units = _guide_units("random", w, h)
    state = VC.error_state("matched", image)
    error_unit = _error_of(state, w, h)
    base = R.live_resources()
    unit = R.DenoiseUnit(w, h)
    created = R.live_resources()
    _check(unit, dst, image_unit, image, error_unit, state, units, films, {}, w, h)
    first = R.live_resources()
    assert first[0] - created[0] == 2 and first[1] == created[1]           # two planes, no stream
    unit.denoise(image_unit, dst=dst, **units)
    assert same_bits(dst.tristimulus_buffer, DO.denoise(image, **films).reshape(h * w, 3))
    _check(unit, dst, image_unit, image, error_unit, state, units, films, dict(iterations=2), w, h)
    assert R.live_resources() == first
    assert unit.variance_ms() > 0 and all(ms > 0 for ms in unit.pass_ms()[:3])
    unit.close()
    assert R.live_resources() == base


def _demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return R.Scene(objs, cam)


def test_the_variance_form_lowers_the_error_where_the_plain_filter_raises_it():
    """64 x 36, demo scene, seed 1: n paths of stream 0 as 16 fused renders, each observed, then accumulated; the guides of 2^16
    paths; against 2^23 paths of stream 1 scaled by n / 2^23.  Mean squared error of the XYZ film after the filter over the error
    before it, from numpy on the oracle's photons: variance form 0.346 at n = 2^16 and 0.680 at 2^20, plain filter 0.365 and 1.140.
    The device's photons are the oracle's and the films differ by the order of the atomics only."""
    w, h, n_ref, n_guides = 64, 36, 1 << 23, 1 << 16
    scene = _demo()
    trace = R.TraceUnit(0, w, h, n_photons=64)
    plots = [R.PlotUnit(i, w, h) for i in range(4)]
    albedo, normal, aux, ref, plain, clean = (R.GatherUnit(w, h) for _ in range(6))
    scene.render_features(w, h, 1, 0, 0, n_guides, albedo=plots[1], normal=plots[2], aux=plots[3])
    for g, p in zip((albedo, normal, aux), plots[1:]):
        g.accumulate(p)
    trace.render_fused(scene, plots[0], n_ref, seed=1, stream=1, first_path_index=0)
    ref.accumulate(plots[0])
    reference = ref.tristimulus_buffer.astype(np.float64)
    unit = R.DenoiseUnit(w, h)
    guides = dict(albedo=albedo, normal=normal, aux=aux)
    films = {k: g.tristimulus_buffer.reshape(h, w, 3) for k, g in guides.items()}
    for n in (1 << 16, 1 << 20):
        noisy, error = R.GatherUnit(w, h), R.ErrorUnit(w, h)
        for b in range(16):
            trace.render_fused(scene, plots[0], n // 16, seed=1, stream=0, first_path_index=b * (n // 16))
            error.observe(plots[0], n // 16)
            noisy.accumulate(plots[0])
        unit.denoise(noisy, dst=plain, **guides)
        unit.denoise_variance(noisy, error, dst=clean, **guides)
        want = reference * (n / n_ref)
        mse = [float(((g.tristimulus_buffer - want) ** 2).mean()) for g in (noisy, plain, clean)]
        print("n = 2^%d: mean squared error noisy %.6g, plain filter %.6g (ratio %.4f), variance form %.6g (ratio %.4f)"
              % (n.bit_length() - 1, mse[0], mse[1], mse[1] / mse[0], mse[2], mse[2] / mse[0]))
        assert mse[2] < mse[0]
        if n == 1 << 20:
            assert mse[2] < mse[1]
        # the device's result is the oracle's on rendered films too
        s, q, k, paths = error.download()
        assert (k, paths) == (16, n)
        want_c, _ = VO.denoise(noisy.tristimulus_buffer.reshape(h, w, 3), s, q, k, paths, **films)
        assert same_bits(clean.tristimulus_buffer, want_c.reshape(-1, 3))


APP = dict(concurrency=2, photons_per_batch=1 << 16, tonemap_interval_ms=5, fused=True)


def test_the_app_hands_out_the_error_state_of_its_last_run():
    w, h = 64, 36
    rgb, st, err = R.app_run_to_error(w, h, 12, target_error=0.0, **APP)
    end = err["at_end"]
    s, q, k, n = R.app_error_state()
    assert err["estimates"] >= 1 and (k, n) == (end["observations"], end["paths"]) and n == 12 << 16 and k >= 2
    assert s.shape == q.shape == (w * h,) and s.any() and q.any()
    unit = R.ErrorUnit(w, h)
    unit.upload(s, q, k, n)
    stats = unit.estimate(se=False, tiles=True)
    assert stats[0]["relative_error"] == end["relative_error"] and stats[0]["sum_se"] == end["sum_se"] and stats[0]["sum_y"] == end["sum_y"]
    assert stats[2].tobytes() == err["tiles"].tobytes()
    # the capacity protocol on a state that is there
    cnt = C.c_uint64(0)
    assert _lib.lib.rl_app_error_state(None, None, 0, C.byref(cnt), None, None) == RL_E_INVALID and cnt.value == w * h and b"too small" in _err()
    assert _lib.lib.rl_app_error_state(s.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), w * h - 1, None, None, None) == RL_E_INVALID
    # a run without a target leaves none
    R.app_run_to_error(w, h, 2, target_error=None, **APP)
    assert R.app_error_state()[2:] == (0, 0) and R.app_error_state()[0].size == 0


def _png_pixels(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = struct.unpack(">II", data[16:24])
    pos, idat = 8, b""
    while pos < len(data):
        size, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + size]
        pos += 12 + size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    return w, h, rows[:, 1:]


@pytest.mark.parametrize("mode", [["--direct"], ["--error-map", None]], ids=["direct", "app"])
def test_the_command_line_writes_another_image_with_the_variance_term(mode, tmp_path, capsys):
    out, prefix = str(tmp_path / "image.png"), str(tmp_path / "guides")
    mode = [str(tmp_path / "map.png") if m is None else m for m in mode]
    images = []
    for name, flag in (("plain.png", []), ("variance.png", ["--denoise-variance"])):
        clean = str(tmp_path / name)
        CLI.main(mode + flag + ["--features", prefix, "--denoise", clean, "--output", out, "--width", "64", "--height", "36", "--batches", "32",
                                "--photons-per-batch", "16384", "--quiet"])
        images.append(_png_pixels(clean))
    told = capsys.readouterr().out
    assert "denoised with the variance term" in told
    (w, h, plain), (w2, h2, variance) = images
    assert (w, h) == (w2, h2) == (64, 36) and plain.any() and variance.any() and (plain != variance).any()


def test_the_command_line_refuses_one_batch(capsys):
    for mode in (["--direct"], ["--error-map", "map.png"]):
        with pytest.raises(SystemExit) as e:
            CLI.main(mode + ["--features", "g", "--denoise", "clean.png", "--denoise-variance", "--width", "64", "--height", "36", "--batches", "1",
                             "--photons-per-batch", "4096", "--quiet"])
        told = capsys.readouterr().err
        assert e.value.code == 2 and "two batches" in told and "two observations" in told, told
