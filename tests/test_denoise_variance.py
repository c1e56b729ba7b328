"""rl_denoise_unit_denoise_variance without a GPU: the CPU restatement (tests/_denoise_variance_oracle.py) against facts that do not
come from the new code, the boundary of the C ABI (defaults in every mirror, the argument checks that need no device in the
documented order, rl_app_error_state's capacity protocol), the compiled kernels' resources and the command line's
--denoise-variance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _denoise_oracle as DO
import _denoise_variance_cases as VC
import _denoise_variance_oracle as VO
import _error_cases as EC
import _error_oracle as EO
from _boundary import _Fake, _err
from _device_build import kernels  # noqa: F401  (a fixture)
from _image_cases import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID, RL_E_STATE = -1, -5
OFF = dict(sigma_colour=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
f32 = np.float32


# ---- the oracle against facts that do not come from the new code -------------------------------------------------------------------

@pytest.mark.parametrize("guide", ["random", "checker"])
def test_an_infinite_or_a_zero_variance_switches_the_colour_term_off(guide):
    """V = +inf: dl * dl / inf is exactly 0 for a finite image; V = 0: m > 0 fails.  Either way e_c = 0, which is what the plain
    filter computes with sigma_colour = 0 (kc = 0 times a finite e_c): the same bits.  With V = 0 every product (wt * wt) * 0 is
    0 and so is V_out."""
    w, h = 33, 19
    img = VC.image("loguniform", w, h)
    g = VC.guides(guide, w, h)
    want = DO.denoise(img, sigma_colour=0.0, **g)
    c_inf, v_inf = VO.denoise_v(img, np.full((h, w), np.inf, f32), **g)
    c_zero, v_zero = VO.denoise_v(img, np.zeros((h, w), f32), **g)
    assert same_bits(c_inf, want) and same_bits(c_zero, want)
    assert not v_zero.any() and not np.signbit(v_zero).any()
    live = g["aux"][..., 0] > 0
    assert np.isinf(v_inf[~live]).all()
    # the control: a finite variance does change the image
    assert not same_bits(VO.denoise_v(img, np.full((h, w), 1e-4, f32), **g)[0], want)


def test_with_every_sigma_off_a_constant_variance_shrinks_by_the_taps_squared():
    """x = 0, wt = h h exactly, sum_w = 1 exactly; sum_v is the f32 sum of 25 products (h h)^2 c.  For a c of few bits each is
    exact, and so is every partial sum: they add up to 4900 / 65536 c.  The bound, 4 ulp, leaves room it does not need."""
    w = h = 9
    img = VC.image("loguniform", w, h)
    for c in (f32(0.75), f32(4.0), f32(2.0 ** -20)):
        C1, V1 = VO.denoise_v(img, np.full((h, w), c, f32), iterations=1, **OFF)
        want = np.float64(c) * (70.0 / 256.0) ** 2
        inner = V1[2:h - 2, 2:w - 2].astype(np.float64)
        ulp = np.spacing(f32(want)).astype(np.float64)
        print("c = %g: largest error %.3f ulp" % (c, (np.abs(inner - want) / ulp).max()))
        assert (np.abs(inner - want) <= 4 * ulp).all()
        assert same_bits(C1, DO.denoise(img, iterations=1, **OFF))


def test_a_dead_pixel_copies_both_image_and_variance():
    w, h = 33, 19
    img = VC.image("loguniform", w, h)
    g = VC.guides("checker", w, h)
    dead = g["aux"][..., 0] == 0
    assert dead.any() and (~dead).any()
    V0 = VO.variance_0(*VC.error_state("matched", img))
    assert (V0 > 0).all()
    C5, V5 = VO.denoise_v(img, V0, **g)
    assert same_bits(C5[dead], img[dead]) and same_bits(V5[dead], V0[dead])
    assert not same_bits(C5[~dead], img[~dead]) and (V5[~dead] < V0[~dead]).any()
    # what a dead pixel holds changes nothing elsewhere
    img2, V2 = img.copy(), V0.copy()
    img2[dead] = np.array([np.nan, 1e30, -np.inf], f32)
    V2[dead] = f32(np.nan)
    C6, V6 = VO.denoise_v(img2, V2, **g)
    assert same_bits(C6[~dead], C5[~dead]) and same_bits(V6[~dead], V5[~dead]) and same_bits(V6[dead], V2[dead])
    # an all-dead frame is returned as it is
    Cd, Vd = VO.denoise_v(img, V0, **VC.guides("dead", w, h))
    assert same_bits(Cd, img) and same_bits(Vd, V0)


def test_flipping_all_inputs_left_to_right_flips_both_outputs():
    """As the plain filter's test: a weight is a function of the pair and keeps its bits under the mirror (dl * dl and V_p + V_q are
    symmetric); only the order of the 25 non-negative terms changes.  C: within 98 u per pass as there.  V: sum_v and sum_w are
    each within 24 u of their exact sums in either order, sum_w * sum_w and the quotient add 2 u: (24 + 2 * 24 + 2) u per order,
    148 u between the two, relative; with the colour term off the weights do not depend on C or V, and a pass maps a relative
    error of V through a ratio of positive sums, which does not enlarge it, so n passes stay within n times that (1 % for the
    second-order terms)."""
    w, h = 33, 19
    u = 2.0 ** -24
    img = VC.image("loguniform", w, h)
    g = VC.guides("random", w, h)
    V0 = VO.variance_0(*VC.error_state("matched", img))
    flip = lambda a: None if a is None else np.ascontiguousarray(a[:, ::-1])
    for params, passes in ((dict(iterations=1), 1), (dict(iterations=5, sigma_colour=0.0), 5)):
        a, va = VO.denoise_v(img, V0, **g, **params)
        b, vb = VO.denoise_v(flip(img), flip(V0), **{k: flip(v) for k, v in g.items()}, **params)
        b, vb = flip(b), flip(vb)
        rel_c = np.abs(a.astype(np.float64) - b) / np.abs(a)
        rel_v = np.abs(va.astype(np.float64) - vb) / np.abs(va)
        print("%d passes: C %.3f and V %.3f of the bound" % (passes, rel_c.max() / (passes * 98 * u * 1.01), rel_v.max() / (passes * 148 * u * 1.01)))
        assert (rel_c <= passes * 98 * u * 1.01).all() and (rel_v <= passes * 148 * u * 1.01).all()


@pytest.mark.parametrize("name", EC.CASES)
def test_the_square_root_of_v0_is_the_error_units_standard_error(name):
    """V_0 is rl_error_unit_estimate's v, so rl_sqrtf(V_0) has the bits of its se: on every state of tests/_error_cases.py."""
    w, h = 33, 47
    case = EC.case(name, w, h)
    state = case["initial"] or EO.new_state(w, h)
    for xyz, n in case["observations"]:
        state = EO.observe(state, xyz, n)
    se = EO.pixels(state)[0]
    with np.errstate(all="ignore"):
        got = np.sqrt(VO.variance_0(*state))
    assert same_bits(got, se)


# ---- the boundary -------------------------------------------------------------------------------------------------------------------

NAMES = ("rl_denoise_variance_params_default", "rl_denoise_unit_denoise_variance", "rl_app_error_state")


def test_defaults_and_entry_points_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    p = _lib.RlDenoiseParams(9, 9.0, 9.0, 9.0, 9.0, (C.c_uint32 * 3)(9, 9, 9))
    assert _lib.lib.rl_denoise_variance_params_default(C.byref(p)) == 0
    assert (p.iterations, list(p.reserved)) == (5, [0, 0, 0])
    assert [f32(x) for x in (p.sigma_colour, p.sigma_normal, p.sigma_depth, p.sigma_albedo)] == [f32(x) for x in (3.0, 0.3, 0.1, 0.2)]
    assert R.denoise_variance_params_default() == {k: (v if k == "iterations" else float(f32(v))) for k, v in VO.DEFAULTS.items()}
    assert "{5, 3.0, 0.3, 0.1, 0.2}" in header
    assert _lib.lib.rl_denoise_variance_params_default(None) == RL_E_INVALID and _err()
    for name in NAMES:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
        assert name in guide, name
    assert len(_lib.SIGNATURES["rl_denoise_unit_denoise_variance"][1]) == 9 and len(_lib.SIGNATURES["rl_app_error_state"][1]) == 6
    for name in ("rl_debug_denoise_variance_launches", "rl_debug_denoise_variance_ms"):
        assert re.search(r"int %s\(" % name, debug) and name in _lib.DEBUG_SIGNATURES and hasattr(_lib.lib, name)
    assert len(R.denoise_variance_launches()) == 2 and _lib.lib.rl_debug_denoise_variance_launches(None) == RL_E_INVALID
    assert "DOES NOT CHECK" in header      # the units of `image` are the caller's to get right, and the header says so


def _params(iterations=0, sigmas=(3.0, 0.3, 0.1, 0.2), reserved=(0, 0, 0)):
    return _lib.RlDenoiseParams(iterations, *sigmas, (C.c_uint32 * 3)(*reserved))


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    """1. null unit, image, dst or error; 2. iterations; 3. a sigma; 4. reserved; 5. repeated handles; 6. an error unit with k < 2
    (the stand-in handle's zero bytes read as k = 0): each with everything behind it wrong as well, and alone.  None touches a
    device."""
    fn = _lib.lib.rl_denoise_unit_denoise_variance
    u, img, a, n, x, dst, err = (_Fake().ptr for _ in range(7))
    nan = float("nan")
    worst = C.byref(_params(7, (-1.0, nan, 1e-4, 2e3), (0, 1, 0)))
    ok = C.byref(_params())
    out = (C.c_float * 4)(7, 7, 7, 7)
    cases = [((None, img, img, img, img, err, worst, img, out), RL_E_INVALID, b"null"),
             ((u, None, a, n, x, err, ok, dst, out), RL_E_INVALID, b"null"),
             ((u, img, a, n, x, err, None, None, out), RL_E_INVALID, b"null"),
             ((u, img, img, img, img, None, worst, img, out), RL_E_INVALID, b"null"),
             ((u, img, a, n, x, None, None, dst, None), RL_E_INVALID, b"null"),
             ((u, img, img, img, img, err, worst, img, out), RL_E_INVALID, b"iterations"),
             ((u, img, a, n, x, err, C.byref(_params(7)), dst, out), RL_E_INVALID, b"iterations")]
    for k, name in enumerate((b"sigma_colour", b"sigma_normal", b"sigma_depth", b"sigma_albedo")):
        for bad in (-1.0, nan, 0.99e-3, 1.01e3, float("inf")):
            sig = [3.0, 0.0, 1e-3, 1e3]
            sig[k] = bad
            cases.append(((u, img, a, n, x, err, C.byref(_params(6, sig)), dst, out), RL_E_INVALID, name))
    cases += [((u, img, img, img, img, err, C.byref(_params(6, (3.0, 0.3, -1.0, nan), (0, 0, 1))), img, out), RL_E_INVALID, b"sigma_depth"),
              ((u, img, img, img, img, err, C.byref(_params(1, reserved=(0, 0, 1))), img, out), RL_E_INVALID, b"reserved"),
              ((u, img, a, n, x, err, C.byref(_params(reserved=(1, 0, 0))), dst, out), RL_E_INVALID, b"reserved")]
    for rep in ((u, img, img, n, x), (u, img, a, a, x), (u, img, a, n, a), (u, img, None, n, n), (u, img, img, None, None)):
        cases.append((rep + (err, ok, dst, out), RL_E_INVALID, b"distinct"))
    cases += [((u, img, a, n, x, err, ok, img, out), RL_E_INVALID, b"distinct"), ((u, img, None, None, None, err, None, img, out), RL_E_INVALID, b"distinct"),
              ((u, img, a, n, x, err, ok, dst, out), RL_E_STATE, b"observations"), ((u, img, None, None, None, err, None, dst, None), RL_E_STATE, b"observations")]
    for args, code, word in cases:
        assert fn(*args) == code and word in _err(), (args, code, word, _err())
        assert b"rl_denoise_unit_denoise_variance" in _err()
    assert list(out) == [7, 7, 7, 7]
    with pytest.raises(TypeError):
        R.DenoiseUnit.denoise_variance(None, None, None, dst=None, sigma=1.0)


def test_the_app_error_state_is_empty_before_any_run_and_follows_the_capacity_protocol():
    n, k, paths = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    assert _lib.lib.rl_app_error_state(None, None, 0, C.byref(n), C.byref(k), C.byref(paths)) == 0
    assert (n.value, k.value, paths.value) == (0, 0, 0)
    assert _lib.lib.rl_app_error_state(None, None, 0, None, None, None) == 0
    s, q, k2, n2 = R.app_error_state()
    assert s.size == 0 and q.size == 0 and (k2, n2) == (0, 0)
    # a run that is refused before any device work leaves it empty as well
    with pytest.raises(R.RlError):
        R.app_run_to_error(0, 0, 1, target_error=0.1)
    assert R.app_error_state()[2:] == (0, 0)


# ---- the compiled kernels -----------------------------------------------------------------------------------------------------------

def test_variance_kernels_keep_to_their_registers_and_the_one_tile_of_lds(kernels):
    """The V_0 kernel may run beside a resident open trace kernel, as the error unit's kernels do: at most 32 VGPRs, no LDS, no
    scratch.  The variance form of the pass kernel has the plain form's LDS: the 20 x 32-word tile three times."""
    v0 = [(n, k) for n, k in kernels.items() if "rl_variance_denoise_kernel" in n]
    passes = [(n, k) for n, k in kernels.items() if "rl_variance_denoise_pass_kernel" in n]
    assert len(v0) == 1 and len(passes) == 1, sorted(kernels)
    for name, k in v0 + passes:
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                                                                                    k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
    assert v0[0][1]["vgpr_count"] <= 32 and v0[0][1]["group_segment_fixed_size"] == 0
    assert passes[0][1]["group_segment_fixed_size"] == 3 * 20 * 32 * 16 == 30720
    assert passes[0][1]["max_flat_workgroup_size"] == 256


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_the_command_line_refuses_denoise_variance_without_what_it_needs(capsys):
    base = ["--width", "64", "--height", "36", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base + ["--batches", "2", "--direct", "--features", "g", "--denoise", "c.png", "--denoise-variance"])
    assert a.denoise_variance and a.direct
    assert CLI.parse_args(base + ["--batches", "2", "--features", "g", "--denoise", "c.png", "--denoise-variance", "--error-map", "e.png"]).denoise_variance
    assert CLI.parse_args(base + ["--batches", "2", "--features", "g", "--denoise", "c.png", "--denoise-variance", "--target-error", "0.1"]).denoise_variance
    assert not CLI.parse_args(base + ["--features", "g", "--denoise", "c.png"]).denoise_variance
    for argv, words in ((["--batches", "2", "--direct", "--features", "g", "--denoise-variance"], ("--denoise-variance", "--denoise PATH")),
                        (["--batches", "2", "--denoise-variance"], ("--denoise-variance", "--denoise PATH")),
                        (["--batches", "2", "--features", "g", "--denoise", "c.png", "--denoise-variance"], ("--target-error", "--error-map")),
                        (["--batches", "2", "--features", "g", "--denoise", "c.png", "--denoise-variance", "--error-map", "e.png", "--resume"], ("--resume",)),
                        (["--batches", "1", "--direct", "--features", "g", "--denoise", "c.png", "--denoise-variance"], ("two batches", "two observations")),
                        (["--batches", "1", "--features", "g", "--denoise", "c.png", "--denoise-variance", "--error-map", "e.png"], ("two batches",))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + argv)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), told
