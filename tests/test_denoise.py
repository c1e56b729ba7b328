"""rl_denoise_unit_denoise without a GPU: the CPU restatement (tests/_denoise_oracle.py) against facts that do not come from the
code, the boundary of the C ABI (layout, defaults, argument checks in the documented order, no CPU fallback), the compiled kernels'
resources (hipcc cross-compiles here) and the command line's --denoise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _denoise_cases as DC
import _denoise_oracle as DO
from _boundary import _Fake, _err
from _device_build import kernels  # noqa: F401  (a fixture)
from _image_cases import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
U = 2.0 ** -24                       # the unit roundoff of f32
OFF = dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)


# ---- the oracle against facts that do not come from the code ----------------------------------------------------------------------

def test_with_every_sigma_off_a_pass_is_the_b3_blur():
    """Every sigma 0 and all pixels live: x = 0, rl_expf(-0) = 1 and wt = h[dy+2] h[dx+2] exactly, sum_w = 1 exactly, so an interior
    pixel of pass 0 is the f32 sum of 25 rounded products: within (25 + 2) 2^-24 of the f64 blur, relative to the sum of |terms|."""
    w, h = 11, 9
    img = DC.image("loguniform", w, h)
    got = DO.denoise(img, iterations=1, **OFF)
    taps = np.array([1, 4, 6, 4, 1], np.float64) / 16
    want, scale = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            shifted = np.roll(img.astype(np.float64), (-dy, -dx), axis=(0, 1))
            want += taps[dy + 2] * taps[dx + 2] * shifted
            scale += taps[dy + 2] * taps[dx + 2] * np.abs(shifted)
    inner = (slice(2, h - 2), slice(2, w - 2))
    err = np.abs(got.astype(np.float64) - want)[inner] / scale[inner]
    print("largest error over the bound: %.3f" % (err.max() / ((25 + 2) * U)))
    assert (err <= (25 + 2) * U).all()
    assert DO.expf(np.array([0.0, -0.0], np.float32)).tolist() == [1.0, 1.0]


def test_an_edge_between_opposite_normals_is_not_crossed():
    """A different power-of-two constant on each side, opposite normals, sigma_normal = 0.1: across the edge e_n = 4 and
    x >= 4 / 0.1^2 = 400, where rl_expf returns exactly 0; within a side x = 0, every weight is a dyadic h h and sum_c = c sum_w
    exactly.  So six passes return the input bit for bit."""
    w, h = 40, 24
    xs = np.arange(w)[None, :, None]
    img = np.where(xs < 20, np.float32(4.0), np.float32(0.125)) * np.ones((h, w, 3), np.float32)
    g = DC.guides("halfplanes", w, h)
    assert DO.expf(np.array([-400.0], np.float32))[0] == 0.0
    passes = []
    got = DO.denoise(img, iterations=6, sigma_normal=0.1, passes=passes, **g)
    assert len(passes) == 6 and all(same_bits(p, img) for p in passes) and same_bits(got, img)
    # the control: without the normal term the edge is crossed
    assert not same_bits(DO.denoise(img, iterations=6, sigma_colour=0.0, sigma_normal=0.0, **g), img)


def test_pixels_that_are_not_live_are_copied_and_never_contribute():
    w, h = 33, 19
    img = DC.image("loguniform", w, h)
    g = DC.guides("checker", w, h)
    dead = g["aux"][..., 0] == 0
    assert dead.any() and (~dead).any()
    got = DO.denoise(img, **g)
    assert same_bits(got[dead], img[dead]) and not same_bits(got[~dead], img[~dead])
    # what a dead pixel holds -- in the image or in the other guides -- changes nothing elsewhere
    img2, g2 = img.copy(), {k: v.copy() for k, v in g.items()}
    img2[dead] = np.array([np.nan, 1e30, -np.inf], np.float32)
    g2["normal"][dead] = np.float32(7.0)
    g2["albedo"][dead] = np.float32(np.inf)
    got2 = DO.denoise(img2, **g2)
    assert same_bits(got2[~dead], got[~dead]) and same_bits(got2[dead], img2[dead])
    # an all-dead frame is returned as it is
    assert same_bits(DO.denoise(img, **DC.guides("dead", w, h)), img)


def test_flipping_image_and_guides_left_to_right_flips_the_result():
    """Each weight is a function of the pair (p, q) and does not change bits when both are mirrored; a mirrored pixel's sums run in
    mirrored tap order.  An f32 sum of 25 non-negative terms in any order is within 24 u of the exact sum, so for a positive image
    each ordering's sum_c / sum_w is within (24 + 24 + 1) u of the exact quotient, and the two orderings within 98 u of each other,
    relative (1 % is left for the second-order terms).  With the colour term off the weights do not depend on C; a pass is then a
    convex combination of positive values, which does not enlarge a relative error, so n passes stay within n times that."""
    w, h = 33, 19
    img = DC.image("loguniform", w, h)
    g = DC.guides("random", w, h)
    flip = lambda a: None if a is None else np.ascontiguousarray(a[:, ::-1])
    for params, passes in ((dict(iterations=1), 1), (dict(iterations=5, sigma_colour=0.0), 5)):
        a = DO.denoise(img, **g, **params)
        b = flip(DO.denoise(flip(img), **{k: flip(v) for k, v in g.items()}, **params))
        rel = np.abs(a.astype(np.float64) - b) / np.abs(a)
        print("%d passes: largest difference over the bound %.3f" % (passes, rel.max() / (passes * 98 * U * 1.01)))
        assert (rel <= passes * 98 * U * 1.01).all()


def test_null_guides_act_as_the_stated_constants():
    w, h = 17, 16
    img = DC.image("loguniform", w, h)
    g = DC.guides("random", w, h)
    ones = np.tile(np.array([1, 0, 0], np.float32), (h, w, 1))
    zeros = np.zeros((h, w, 3), np.float32)
    assert same_bits(DO.denoise(img, albedo=g["albedo"], normal=g["normal"]), DO.denoise(img, albedo=g["albedo"], normal=g["normal"], aux=ones))
    assert same_bits(DO.denoise(img, aux=g["aux"]), DO.denoise(img, albedo=zeros, normal=zeros, aux=g["aux"]))


# ---- the boundary ---------------------------------------------------------------------------------------------------------------

def test_params_layout_and_defaults_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert C.sizeof(_lib.RlDenoiseParams) == 32
    assert [(f, C.sizeof(t)) for f, t in _lib.RlDenoiseParams._fields_] == [("iterations", 4), ("sigma_colour", 4), ("sigma_normal", 4),
                                                                            ("sigma_depth", 4), ("sigma_albedo", 4), ("reserved", 12)]
    assert re.search(r"\} RlDenoiseParams;\s*/\* 32 bytes \*/", header) and re.search(r"pub struct RlDenoiseParams \{.*?\} // 32 bytes", rust, re.S)
    assert re.search(r"#define RL_DENOISE_MAX_ITERATIONS 6\b", header) and re.search(r"pub const RL_DENOISE_MAX_ITERATIONS: u32 = 6;", rust)
    assert re.search(r"#define RL_DENOISE_ITERATIONS 5\b", header) and re.search(r"pub const RL_DENOISE_ITERATIONS: u32 = 5;", rust)
    assert (_lib.RL_DENOISE_ITERATIONS, _lib.RL_DENOISE_MAX_ITERATIONS) == (DO.ITERATIONS, DO.MAX_ITERATIONS) == (5, 6)
    p = _lib.RlDenoiseParams(9, 9.0, 9.0, 9.0, 9.0, (C.c_uint32 * 3)(9, 9, 9))
    assert _lib.lib.rl_denoise_params_default(C.byref(p)) == 0
    assert (p.iterations, list(p.reserved)) == (5, [0, 0, 0])
    got = [np.float32(x) for x in (p.sigma_colour, p.sigma_normal, p.sigma_depth, p.sigma_albedo)]
    assert got == [np.float32(x) for x in (0.6, 0.3, 0.1, 0.2)]
    assert R.denoise_params_default() == {k: (v if k == "iterations" else float(np.float32(v))) for k, v in DO.DEFAULTS.items()}
    assert _lib.lib.rl_denoise_params_default(None) == RL_E_INVALID and _err()
    for name in ("rl_denoise_params_default", "rl_denoise_unit_create", "rl_denoise_unit_destroy", "rl_denoise_unit_denoise"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header)
    assert len(R.denoise_launches()) == 2 and _lib.lib.rl_debug_denoise_launches(None) == RL_E_INVALID
    assert _lib.lib.rl_denoise_unit_destroy(None) == 0


def _params(iterations=0, sigmas=(0.6, 0.3, 0.1, 0.2), reserved=(0, 0, 0)):
    return _lib.RlDenoiseParams(iterations, *sigmas, (C.c_uint32 * 3)(*reserved))


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    """1. null unit, image or dst; 2. iterations; 3. a sigma; 4. reserved; 5. repeated handles: each with everything behind it wrong as
    well, and alone.  None of them reads a handle or touches a device."""
    fn = _lib.lib.rl_denoise_unit_denoise
    u, img, a, n, x, dst = (_Fake().ptr for _ in range(6))
    nan = float("nan")
    worst = _params(7, (-1.0, nan, 1e-4, 2e3), (0, 1, 0))
    ok = _params()
    cases = [((None, img, img, img, img, C.byref(worst), img), b"null"), ((u, None, a, n, x, C.byref(ok), dst), b"null"),
             ((u, img, a, n, x, None, None), b"null"),
             ((u, img, img, img, img, C.byref(worst), img), b"iterations"), ((u, img, a, n, x, C.byref(_params(7)), dst), b"iterations"),
             ((u, img, a, n, x, C.byref(_params(0xFFFFFFFF)), dst), b"iterations")]
    for k, name in enumerate((b"sigma_colour", b"sigma_normal", b"sigma_depth", b"sigma_albedo")):
        for bad in (-1.0, -0.5e-3, nan, 0.99e-3, 1.01e3, float("inf")):
            sig = [0.6, 0.0, 1e-3, 1e3]
            sig[k] = bad
            cases.append(((u, img, a, n, x, C.byref(_params(6, sig)), dst), name))
    cases += [((u, img, img, img, img, C.byref(_params(6, (0.6, 0.3, -1.0, nan), (0, 0, 1))), img), b"sigma_depth"),
              ((u, img, img, img, img, C.byref(_params(1, reserved=(0, 0, 1))), img), b"reserved"),
              ((u, img, a, n, x, C.byref(_params(reserved=(1, 0, 0))), dst), b"reserved")]
    for rep in ((u, img, img, n, x), (u, img, a, a, x), (u, img, a, n, a), (u, img, None, n, n), (u, img, img, None, None)):
        cases.append((rep + (C.byref(ok), dst), b"distinct"))
    cases += [((u, img, a, n, x, C.byref(ok), img), b"distinct"), ((u, img, a, n, dst, None, dst), b"distinct"), ((u, img, None, None, None, None, img), b"distinct")]
    for args, word in cases:
        assert fn(*args) == RL_E_INVALID and word in _err(), (args, word, _err())
    # create: the output handle, the size and RL_MAX_PIXELS before the device
    h = C.c_void_p()
    assert _lib.lib.rl_denoise_unit_create(0, 64, 36, None) == RL_E_INVALID
    assert _lib.lib.rl_denoise_unit_create(0, 0, 36, C.byref(h)) == RL_E_INVALID and b"zero" in _err()
    assert _lib.lib.rl_denoise_unit_create(0, 65536, 32768, C.byref(h)) == RL_E_INVALID and b"RL_MAX_PIXELS" in _err()
    with pytest.raises(TypeError):
        R.DenoiseUnit.denoise(None, None, dst=None, sigma=1.0)


@pytest.mark.skipif(R.device_count() > 0, reason="checks the no-GPU behaviour")
def test_the_denoise_unit_fails_loudly_without_a_device():
    with pytest.raises(R.RlError) as e:
        R.DenoiseUnit(64, 36)
    assert e.value.code == -2  # RL_E_NO_DEVICE: there is no CPU implementation to fall back to


def test_denoise_kernels_use_no_scratch_and_one_tile_of_lds(kernels):
    """Neither kernel uses scratch; the pass kernel's LDS is the 20 x 32-word tile three times (30720 bytes), below 64 KB."""
    mine = {n: k for n, k in kernels.items() if "rl_denoise_" in n}
    guides = [k for n, k in mine.items() if "rl_denoise_guides_kernel" in n]
    passes = [k for n, k in mine.items() if "rl_denoise_pass_kernel" in n]
    assert len(guides) == 1 and len(passes) == 1 and len(mine) == 2, sorted(mine)
    for name, k in sorted(mine.items()):
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                                                                                    k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
    assert guides[0]["group_segment_fixed_size"] == 0
    assert passes[0]["group_segment_fixed_size"] == 3 * 20 * 32 * 16 < 64 * 1024
    assert passes[0]["max_flat_workgroup_size"] == 256
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_denoise.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()


def test_the_command_line_wants_features_with_denoise(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "1", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base + ["--features", "g", "--denoise", "clean.png"])
    assert a.denoise == "clean.png" and a.features == "g" and not a.direct
    assert CLI.parse_args(base + ["--direct", "--features", "g", "--denoise", "clean.png"]).direct
    assert CLI.parse_args(base).denoise is None
    for argv in (["--denoise", "clean.png"], ["--direct", "--denoise", "clean.png"]):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + argv)
        told = capsys.readouterr().err
        assert e.value.code == 2 and "--denoise" in told and "--features" in told, told
