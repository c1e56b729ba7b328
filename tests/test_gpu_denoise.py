"""DenoiseUnit.denoise on the device (rl_denoise_unit_denoise) against the CPU restatement (tests/_denoise_oracle.py) bit for bit:
every shape x image class x guide class x parameter set of tests/_denoise_cases.py, on poisoned LDS and into a prefilled dst, every
argument failure in the documented order, the ordering against work queued on a guide's gather unit, the quality of the defaults
end to end on the demo scene, and the command line.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import _denoise_cases as DC
import _denoise_oracle as DO
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


@functools.lru_cache(maxsize=None)
def _rig(w, h):
    """(denoise unit, dst gather unit) of a shape: shared by its cases."""
    return R.DenoiseUnit(w, h), R.GatherUnit(w, h)


@functools.lru_cache(maxsize=None)
def _guide_units(kind, w, h):
    """({name: the film}, {name: the gather unit holding it, or None}) of a guide class and shape: uploaded once, never written.
    The film is what the gather unit holds, which is what the call reads: the upload, but for a -0, which 0 + x makes +0."""
    films = DC.guides(kind, w, h)
    units = {k: _gather_of(v, w, h) for k, v in films.items()}
    held = {k: None if u is None else u.tristimulus_buffer.reshape(h, w, 3) for k, u in units.items()}
    for k, v in films.items():
        assert v is None or (held[k] == v).all()
    return held, units


def _buffers(unit):
    return None if unit is None else unit._download()


def _check(unit, dst, image_unit, image, guide_units, films, params, w, h):
    """One call against the oracle: dst's tristimulus buffer bit for bit, its compensation buffer all +0, the launch counts."""
    before = R.denoise_launches()
    assert unit.denoise(image_unit, dst=dst, **guide_units, **params) is dst
    after = R.denoise_launches()
    iterations = params.get("iterations", 0) or DO.ITERATIONS
    assert (after[0] - before[0], after[1] - before[1]) == (1, iterations)
    got, comp = dst._download()
    want = DO.denoise(image, **films, **params).reshape(h * w, 3)
    assert same_bits(got, want), (params, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert comp.tobytes() == bytes(comp.nbytes)


@pytest.mark.parametrize("kind", DC.IMAGES)
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_guide_class_and_parameter_set_matches_the_oracle_bit_for_bit(shape, kind):
    w, h = shape
    unit, dst = _rig(w, h)
    image = DC.image(kind, w, h)
    image_unit = _gather_of(image, w, h)
    held = image_unit._download()
    assert same_bits(held[0], image.reshape(-1, 3))      # (0 + x = x, NaN and infinities included)
    for guide in DC.GUIDES:
        films, units = _guide_units(guide, w, h)
        inputs = [_buffers(units[k]) for k in ("albedo", "normal", "aux")]
        for name, params in DC.PARAMS.items():
            _check(unit, dst, image_unit, image, units, films, params, w, h)
        # the inputs are left unchanged: both buffers of each
        for k, was in zip(("albedo", "normal", "aux"), inputs):
            if was is not None:
                now = _buffers(units[k])
                assert same_bits(now[0], was[0]) and same_bits(now[1], was[1]) and same_bits(now[0], films[k].reshape(-1, 3)) and not now[1].any(), (guide, k)
    now = image_unit._download()
    assert same_bits(now[0], held[0]) and same_bits(now[1], held[1])


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_on_poisoned_lds_and_into_a_prefilled_dst(shape, pattern, tmp_path):
    """The tile is staged whole before it is read, elements outside the image included, and dst is written whole: stale LDS and
    0xAA bytes in both of dst's buffers change nothing."""
    w, h = shape
    unit, dst = _rig(w, h)
    path = str(tmp_path / "aa.raw")
    with open(path, "wb") as f:
        f.write(b"\xaa" * (w * h * 24))
    image = DC.image("loguniform", w, h)
    image_unit = _gather_of(image, w, h)
    for guide, name in (("random", "defaults"), ("checker", "six_passes"), ("no_aux", "one_pass")):
        films, units = _guide_units(guide, w, h)
        dst.load(path)
        assert dst._download()[1].tobytes() == b"\xaa" * (w * h * 12)
        LP.poison_lds(pattern)
        _check(unit, dst, image_unit, image, units, films, DC.PARAMS[name], w, h)


def _params(iterations=0, sigmas=(0.6, 0.3, 0.1, 0.2), reserved=(0, 0, 0)):
    return C.byref(_lib.RlDenoiseParams(iterations, *sigmas, (C.c_uint32 * 3)(*reserved)))


def test_every_argument_failure_in_the_documented_order():
    w, h = 9, 8
    fn = _lib.lib.rl_denoise_unit_denoise
    unit = R.DenoiseUnit(w, h)
    mark = np.full((h, w, 3), 3.5, np.float32)
    img, a, n, x, dst = (_gather_of(mark, w, h) for _ in range(5))
    other = [R.GatherUnit(w, h + 1), R.GatherUnit(w + 1, h), R.GatherUnit(h, w)]
    U, I, A, N, X, D = (o.handle for o in (unit, img, a, n, x, dst))
    nan = float("nan")
    launches = R.denoise_launches()

    def refused(args, code, word):
        assert fn(*args) == code and word in _err() and len(_err()) > 0, (args, code, word, _err())
        t, c = dst._download()
        assert same_bits(t, mark.reshape(-1, 3)) and not c.any()
        assert R.denoise_launches() == launches
    # each failure with everything behind it wrong as well (a gather unit of another size among them), and alone
    O0 = other[0].handle
    refused((None, I, I, I, I, _params(7, (-1.0, nan, 1e-4, 2e3), (1, 0, 0)), I), RL_E_INVALID, b"null")
    refused((U, None, A, N, X, None, D), RL_E_INVALID, b"null")
    refused((U, I, A, N, X, None, None), RL_E_INVALID, b"null")
    refused((U, O0, O0, N, X, _params(7, (-1.0, nan, 1e-4, 2e3), (1, 0, 0)), D), RL_E_INVALID, b"iterations")
    refused((U, I, A, N, X, _params(7), D), RL_E_INVALID, b"iterations")
    refused((U, O0, O0, N, X, _params(6, (0.6, -1.0, 0.1, 0.2), (1, 0, 0)), D), RL_E_INVALID, b"sigma_normal")
    for k, name in enumerate((b"sigma_colour", b"sigma_normal", b"sigma_depth", b"sigma_albedo")):
        for bad in (-1.0, nan, 0.99e-3, 1.01e3, float("inf")):
            sig = [0.6, 0.3, 0.1, 0.2]
            sig[k] = bad
            refused((U, I, A, N, X, _params(0, sig), D), RL_E_INVALID, name)
    refused((U, O0, O0, N, X, _params(reserved=(0, 0, 1)), D), RL_E_INVALID, b"reserved")
    refused((U, I, A, N, X, _params(reserved=(1, 0, 0)), D), RL_E_INVALID, b"reserved")
    refused((U, O0, O0, N, X, None, D), RL_E_INVALID, b"distinct")
    for args in ((U, I, I, N, X, None, D), (U, I, A, A, X, None, D), (U, I, A, N, N, None, D), (U, I, A, N, X, None, I), (U, I, A, N, X, None, X),
                 (U, I, None, None, None, None, I), (U, I, None, A, A, None, D)):
        refused(args, RL_E_INVALID, b"distinct")
    # a gather unit of another size, in every position: RL_E_STATE, nothing written
    for o in other:
        for pos in range(4):
            args = [U, I, A, N, X, None, D]
            args[1 + pos] = o.handle
            refused(tuple(args), RL_E_STATE, b"does not match")
    refused((U, I, None, None, other[0].handle, None, D), RL_E_STATE, b"does not match")
    # ... and as dst (its own content is what must stay)
    for o in other:
        assert fn(U, I, A, N, X, None, o.handle) == RL_E_STATE and b"does not match" in _err()
        assert not o.tristimulus_buffer.any() and R.denoise_launches() == launches
    # the limits themselves are accepted
    assert fn(U, I, A, N, X, _params(6, (1e-3, 1e3, 0.0, 1e-3)), D) == 0 and fn(U, I, None, None, None, _params(1, (0.0, 0.0, 0.0, 0.0)), D) == 0
    with pytest.raises(R.RlError) as e:
        R.DenoiseUnit(0, 4)
    assert e.value.code == RL_E_INVALID


def test_the_call_waits_for_work_queued_on_the_units_it_reads():
    """Half of each film is accumulated, and the other half queued on the gather units' streams immediately before the call: the
    call sees the sums (halves of floats add up exactly to the floats)."""
    w, h = DC.SHAPES[-1]
    unit, dst = _rig(w, h)
    image = DC.image("loguniform", w, h)
    films = {k: v + np.float32(0) for k, v in DC.guides("random", w, h).items()}      # (a -0 is +0 once accumulated)
    half = {k: v * np.float32(0.5) for k, v in dict(films, image=image).items()}
    plots = {k: R.PlotUnit(i, w, h) for i, k in enumerate(half)}
    gathers = {k: R.GatherUnit(w, h) for k in half}
    for k in half:
        plots[k].upload(half[k])
        gathers[k].accumulate(plots[k])
        plots[k].upload(half[k])
    for k in half:
        gathers[k].accumulate(plots[k])
    unit.denoise(gathers["image"], albedo=gathers["albedo"], normal=gathers["normal"], aux=gathers["aux"], dst=dst)
    want = DO.denoise(image, **films).reshape(h * w, 3)
    assert same_bits(dst.tristimulus_buffer, want)
    assert same_bits(gathers["aux"].tristimulus_buffer, films["aux"].reshape(-1, 3))


def test_the_defaults_lower_the_error_of_a_noisy_render_of_the_demo_scene():
    """64 x 36, seed 1: 2^16 paths of stream 0 and their guides, denoised with the defaults, against 2^23 paths of stream 1 scaled
    by the path ratio.  The mean squared error of the XYZ film must fall."""
    w, h, n, n_ref = 64, 36, 1 << 16, 1 << 23
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    scene = R.Scene(objs, cam)
    trace = R.TraceUnit(0, w, h, n_photons=64)
    plots = [R.PlotUnit(i, w, h) for i in range(4)]
    noisy, albedo, normal, aux, ref, dst = (R.GatherUnit(w, h) for _ in range(6))
    trace.render_fused(scene, plots[0], n, seed=1, stream=0, first_path_index=0)
    noisy.accumulate(plots[0])
    scene.render_features(w, h, 1, 0, 0, n, albedo=plots[1], normal=plots[2], aux=plots[3])
    for g, p in zip((albedo, normal, aux), plots[1:]):
        g.accumulate(p)
    trace.render_fused(scene, plots[0], n_ref, seed=1, stream=1, first_path_index=0)
    ref.accumulate(plots[0])
    R.DenoiseUnit(w, h).denoise(noisy, albedo=albedo, normal=normal, aux=aux, dst=dst)
    want = ref.tristimulus_buffer.astype(np.float64) * (n / n_ref)
    mse_noisy = float(((noisy.tristimulus_buffer - want) ** 2).mean())
    mse_clean = float(((dst.tristimulus_buffer - want) ** 2).mean())
    print("mean squared error: noisy %.6g, denoised %.6g, ratio %.4f" % (mse_noisy, mse_clean, mse_clean / mse_noisy))
    assert mse_clean < mse_noisy
    # the device's result is the oracle's on rendered films too
    got = DO.denoise(noisy.tristimulus_buffer.reshape(h, w, 3), albedo=albedo.tristimulus_buffer.reshape(h, w, 3),
                     normal=normal.tristimulus_buffer.reshape(h, w, 3), aux=aux.tristimulus_buffer.reshape(h, w, 3))
    assert same_bits(dst.tristimulus_buffer, got.reshape(-1, 3))


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


def test_the_command_line_denoises_the_direct_image(tmp_path):
    out, clean, prefix = str(tmp_path / "image.png"), str(tmp_path / "clean.png"), str(tmp_path / "guides")
    CLI.main(["--direct", "--features", prefix, "--denoise", clean, "--output", out, "--width", "64", "--height", "36", "--batches", "1",
              "--photons-per-batch", "65536", "--quiet"])
    w, h, noisy = _png_pixels(out)
    w2, h2, denoised = _png_pixels(clean)
    assert (w, h) == (w2, h2) == (64, 36)
    assert (noisy != denoised).any() and denoised.any()


def test_the_command_line_denoises_the_app_image_through_the_checkpoint(tmp_path):
    out, clean, prefix = str(tmp_path / "image.png"), str(tmp_path / "clean.png"), str(tmp_path / "guides")
    CLI.main(["--features", prefix, "--denoise", clean, "--output", out, "--width", "64", "--height", "36", "--batches", "1",
              "--photons-per-batch", "65536", "--quiet"])
    w, h, noisy = _png_pixels(out)
    w2, h2, denoised = _png_pixels(clean)
    assert (w, h) == (w2, h2) == (64, 36)
    assert (noisy != denoised).any() and denoised.any()
