"""The noise estimate (rl_error_unit_*, rl_app_run_to_error) without a GPU: the CPU restatement (tests/_error_oracle.py) against
facts that do not come from the code, the boundary of the C ABI (struct layouts in every mirror, argument checks in the documented
order, no CPU fallback), the compiled kernels' resources (hipcc cross-compiles here) and the command line's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _error_cases as EC
import _error_oracle as EO
from _boundary import _Fake, _err
from _device_build import device_build, kernels  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID, RL_E_STATE = -1, -5
FUNCTIONS = ("rl_error_unit_create", "rl_error_unit_destroy", "rl_error_unit_clear", "rl_error_unit_observe", "rl_error_unit_estimate",
             "rl_error_unit_download", "rl_error_unit_upload", "rl_app_run_to_error", "rl_app_error_tiles")


def _run(name, w, h):
    c = EC.case(name, w, h)
    state = c["initial"] if c["initial"] is not None else EO.new_state(w, h)
    for xyz, n in c["observations"]:
        state = EO.observe(state, xyz, n)
    return state


# ---- the oracle against facts that do not come from the code ----------------------------------------------------------------------

@pytest.mark.parametrize("power", [-20, 3, 40])
def test_scaling_by_a_power_of_two_scales_the_estimate_exactly(power):
    """y -> 2^p y: S, Q, d and v scale exactly by 2^p, 4^p, 4^p, 4^p (no rounding changes away from overflow and underflow), so
    every se, t_se and t_y scales by 2^p exactly and relative_error and the worst tile's are unchanged."""
    w, h = 33, 47
    c = EC.case("n_unequal", w, h)
    a, b = EO.new_state(w, h), EO.new_state(w, h)
    for xyz, n in c["observations"]:
        a = EO.observe(a, xyz, n)
        b = EO.observe(b, xyz * np.float32(2.0 ** power), n)
    sa, se_a, ta = EO.estimate(a)
    sb, se_b, tb = EO.estimate(b)
    assert (se_a > 0).sum() > w * h // 2
    assert (se_b == se_a * np.float32(2.0 ** power)).all() and (tb == ta * 2.0 ** power).all()
    assert sb["relative_error"] == sa["relative_error"] and sb["worst_tile_error"] == sa["worst_tile_error"]
    assert (sb["worst_tile_x"], sb["worst_tile_y"]) == (sa["worst_tile_x"], sa["worst_tile_y"])


@pytest.mark.parametrize("shape", EC.SHAPES, ids=lambda s: "%dx%d" % s)
def test_proportional_observations_give_exactly_zero(shape):
    w, h = shape
    stats, se, tiles = EO.estimate(_run("proportional", w, h))
    assert se.tobytes() == bytes(se.nbytes) and tiles[:, :, 0].tobytes() == bytes(tiles[:, :, 0].nbytes)    # +0, not -0
    assert stats["sum_se"] == 0.0 and stats["paths"] == 14 and stats["observations"] == 4


def test_the_clamp_case_rounds_negative_and_is_clamped():
    s, q, k, n = EC.case("clamp", 33, 47)["initial"]
    d = q - (s * s) / np.float64(n)
    assert (d < 0).sum() > 700 and (d > 0).sum() > 700
    se = EO.estimate((s, q, k, n))[1]
    assert (se[d < 0] == 0).all() and not np.signbit(se[d < 0]).any() and (se[d > 0] > 0).all()


def test_the_tile_tree_is_the_stated_one():
    """Against a loop written from the header's words, on values whose sum depends on the order; positions outside are +0."""
    rng = np.random.default_rng(5)
    for w, h in EC.PARTIAL + [(16, 16)]:
        values = rng.random((h, w)) * 10.0 ** rng.integers(-8, 8, size=(h, w))
        got = EO.tile_tree(values)
        for ty in range(got.shape[0]):
            for tx in range(got.shape[1]):
                v = [np.float64(0)] * 256
                for i in range(256):
                    y, x = ty * 16 + i // 16, tx * 16 + i % 16
                    if y < h and x < w:
                        v[i] = values[y, x]
                stride = 128
                while stride:
                    for i in range(stride):
                        v[i] = v[i] + v[i + stride]
                    stride //= 2
                assert got[ty, tx] == v[0]


def test_the_estimate_recovers_the_true_standard_error_of_compound_poisson_pixels():
    """144 pixels, k = 64 observations of 4096 .. 8192 paths, fixed seed: sum(se) / sum(true se) within 10 % of 1.  The true
    variance of S is N times one path's.  A wrong normalisation is off by a factor, not by percents."""
    rng = np.random.default_rng(20261020)
    w, h, k = 12, 12, 64
    rates = rng.uniform(0.0005, 0.004, size=(h, w))
    state = EO.new_state(w, h)
    per_path = None
    for _ in range(k):
        n = int(rng.integers(4096, 8193))
        sums, per_path = EC.compound_poisson(rng, h * w, n, rates)
        xyz = np.zeros((h, w, 3), np.float32)
        xyz[:, :, 1] = sums
        state = EO.observe(state, xyz, n)
    stats, se, tiles = EO.estimate(state)
    true_se = np.sqrt(state[3] * per_path)
    ratio = float(se.astype(np.float64).sum() / true_se.sum())
    print("sum(se) / sum(true se) = %.4f over %d pixels, k = %d, N = %d" % (ratio, w * h, k, state[3]))
    assert 0.9 <= ratio <= 1.1
    assert stats["observations"] == k and abs(stats["sum_se"] - float(se.astype(np.float64).sum())) <= 1e-9 * stats["sum_se"]


def test_the_host_statistics_measure_a_dark_tile_against_the_mean():
    tiles = np.array([[[1.0, 100.0], [1.0, 1.0], [3.0, 60.0], [0.5, 39.0]]])       # mean t_y = 50
    stats = EO.host_stats(tiles, 4, 40)
    assert stats["sum_se"] == 5.5 and stats["sum_y"] == 200.0 and stats["relative_error"] == 5.5 / 200.0
    assert EO.tile_rel(tiles).tolist() == [[0.01, 0.02, 0.05, 0.01]] and R.error_tile_rel(tiles).tolist() == [[0.01, 0.02, 0.05, 0.01]]
    assert (stats["worst_tile_x"], stats["worst_tile_y"], stats["worst_tile_error"]) == (2, 0, 0.05)
    black = EO.host_stats(np.zeros((2, 2, 2)), 2, 2)
    assert np.isnan(black["relative_error"]) and np.isnan(black["worst_tile_error"]) and (black["worst_tile_x"], black["worst_tile_y"]) == (0, 0)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------

def test_structs_constants_and_entry_points_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert re.search(r"#define RL_ERROR_TILE 16\b", header) and re.search(r"pub const RL_ERROR_TILE: u32 = 16;", rust)
    assert _lib.RL_ERROR_TILE == R.RL_ERROR_TILE == EO.TILE == 16
    assert re.search(r"typedef struct RlErrorUnit RlErrorUnit;", header) and re.search(r"pub enum RlErrorUnit \{\}", rust)
    # the layouts: x86-64 / LP64, no padding anywhere
    assert C.sizeof(_lib.RlErrorStats) == 64 and C.sizeof(_lib.RlErrorTarget) == 24 and C.sizeof(_lib.RlAppErrorStats) == 136
    offsets = {n: getattr(_lib.RlErrorStats, n).offset for n, _ in _lib.RlErrorStats._fields_}
    assert offsets == {"observations": 0, "paths": 8, "tiles_x": 16, "tiles_y": 20, "worst_tile_x": 24, "worst_tile_y": 28, "sum_y": 32,
                       "sum_se": 40, "relative_error": 48, "worst_tile_error": 56}
    assert [n for n, _ in _lib.RlErrorTarget._fields_] == ["relative_error", "worst_tile_error", "min_observations", "reserved"]
    assert [n for n, _ in _lib.RlAppErrorStats._fields_] == ["at_stop", "at_end", "reached", "estimates"]
    for name in ("RlErrorStats", "RlErrorTarget", "RlAppErrorStats"):
        assert re.search(r"typedef struct %s \{" % name, header) and re.search(r"#\[repr\(C\)\][^\n]*pub struct %s \{" % name, rust), name
    for name in FUNCTIONS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
        c_args = re.search(r"int %s\(([^;]*)\);" % name, header).group(1).split(",")
        rust_args = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rust, re.S).group(1).split(",")
        assert len(c_args) == len(rust_args) == len(_lib.SIGNATURES[name][1]), name
    for name in ("rl_debug_error_launches", "rl_debug_error_ms"):
        assert re.search(r"int %s\(" % name, debug) and name in _lib.DEBUG_SIGNATURES
    assert len(R.error_launches()) == 2 and _lib.lib.rl_debug_error_launches(None) == RL_E_INVALID
    assert _lib.lib.rl_debug_error_ms(None, None) == RL_E_INVALID
    assert _lib.lib.rl_error_unit_destroy(None) == 0
    # the header states the rules the tests hold the unit to
    for rule in (r"S = S \+ yd", r"Q = Q \+ \(yd \* yd\) / \(double\)n_paths", r"d = d < 0 \? 0 : d", r"stride = 128, 64", "RL_E_STATE",
                 r"rl_sqrtf\(\(float\)v\)", "One user per error unit", "overstates the error of the resumed image"):
        assert re.search(rule, header), rule


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    """Every failure that comes before a handle is used or a device is touched, each with everything behind it wrong as well."""
    L = _lib.lib
    u, plot, buf = _Fake().ptr, _Fake().ptr, _Fake().ptr
    h = C.c_void_p()
    # create: a NULL out; a zero size; the size limit -- before the device (an index no machine has)
    assert L.rl_error_unit_create(99, 0, 0, None) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_create(99, 0, 36, C.byref(h)) == RL_E_INVALID and b"zero" in _err()
    assert L.rl_error_unit_create(99, 64, 0, C.byref(h)) == RL_E_INVALID and b"zero" in _err()
    for w_, h_ in [(46341, 46341), (65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 1)]:
        assert L.rl_error_unit_create(99, w_, h_, C.byref(h)) == RL_E_INVALID and b"RL_MAX_PIXELS" in _err(), (w_, h_)
    assert not h.value
    assert L.rl_error_unit_clear(None) == RL_E_INVALID and b"null" in _err()
    # observe: a NULL unit or plot, n_paths == 0, N overflowing -- then the size (a stand-in of another size: RL_E_STATE)
    assert L.rl_error_unit_observe(None, None, 0) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_observe(None, plot, 5) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_observe(u, None, 5) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_observe(u, plot, 0) == RL_E_INVALID and b"n_paths" in _err()
    # estimate: a NULL unit or stats, then fewer than two observations (a zeroed stand-in has none)
    stats = _lib.RlErrorStats()
    assert L.rl_error_unit_estimate(None, None, None, None) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_estimate(None, C.byref(stats), buf, buf) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_estimate(u, None, buf, buf) == RL_E_INVALID and b"null" in _err()
    assert L.rl_error_unit_estimate(u, C.byref(stats), None, None) == RL_E_STATE and b"at least 2" in _err()
    # download / upload
    assert L.rl_error_unit_download(None, buf, buf, None, None) == RL_E_INVALID and b"null" in _err()
    for args in ((None, buf, buf), (u, None, buf), (u, buf, None)):
        assert L.rl_error_unit_upload(*args, 2, 2) == RL_E_INVALID and b"null" in _err(), args


def test_the_stand_in_units_of_other_sizes_are_refused_with_state():
    """The size check of observe reads only the handles' first words: stand-ins that differ there are RL_E_STATE before any device
    work, and N overflowing 64 bits is RL_E_INVALID before that."""
    L = _lib.lib
    u, plot = _Fake(), _Fake()
    C.cast(u.buf, C.POINTER(C.c_uint32))[1] = 64        # width (the device index comes first)
    assert L.rl_error_unit_observe(u.ptr, plot.ptr, 5) == RL_E_STATE and b"does not match" in _err()
    C.cast(u.buf, C.POINTER(C.c_uint32))[1] = 0
    C.cast(plot.buf, C.POINTER(C.c_int32))[0] = 3       # another device
    assert L.rl_error_unit_observe(u.ptr, plot.ptr, 5) == RL_E_STATE and b"does not match" in _err()


def test_the_app_checks_the_target_before_any_device_work():
    for kwargs, word in ((dict(target_error=-0.5), "relative_error"), (dict(target_error=float("nan")), "relative_error"),
                         (dict(target_error=0.1, worst_tile_error=-1.0), "worst_tile_error"),
                         (dict(target_error=0.1, worst_tile_error=float("nan")), "worst_tile_error"),
                         (dict(target_error=0.1, reserved=1), "reserved")):
        with pytest.raises(R.RlError) as e:
            R.app_run_to_error(64, 36, 1, device=99, **kwargs)
        assert e.value.code == RL_E_INVALID and word in str(e.value), (kwargs, str(e.value))
    with pytest.raises(R.RlError) as e:      # rl_app_run's own checks come first
        R.app_run_to_error(0, 36, 1, target_error=-1.0)
    assert "zero" in str(e.value)
    n = C.c_uint32(7)
    assert _lib.lib.rl_app_error_tiles(None, 0, C.byref(n)) == 0 and n.value == 0       # no run on this thread has estimated


@pytest.mark.skipif(R.device_count() > 0, reason="checks the no-GPU behaviour")
def test_the_error_unit_fails_loudly_without_a_device():
    with pytest.raises(R.RlError) as e:
        R.ErrorUnit(64, 36)
    assert e.value.code == -2  # RL_E_NO_DEVICE: there is no CPU implementation to fall back to
    with pytest.raises(R.RlError) as e:
        R.app_run_to_error(64, 36, 1, target_error=0.1)
    assert e.value.code == -2


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def test_error_kernels_use_no_scratch_and_no_more_lds_than_the_two_trees(kernels):
    mine = {n: k for n, k in kernels.items() if "rl_error_" in n}
    observe = [k for n, k in mine.items() if "rl_error_observe_kernel" in n]
    estimate = [k for n, k in mine.items() if "rl_error_estimate_kernel" in n]
    assert len(observe) == 1 and len(estimate) == 1 and len(mine) == 2, sorted(mine)
    for name, k in sorted(mine.items()):
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                                                                                    k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k["max_flat_workgroup_size"] == 256
        # both run while the App's open trace kernel is resident: four of its waves per SIMD leave 32 VGPRs, and a kernel that
        # needs more waits behind its workgroups (measured: 275 us an observation at 58 VGPRs, profiles/error_bench.txt)
        assert k["vgpr_count"] <= 32, (name, k)
    assert observe[0]["group_segment_fixed_size"] == 0
    assert 0 < estimate[0]["group_segment_fixed_size"] <= 2 * 256 * 8
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_error.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()


def _body(text, kernel):
    name = re.search(r"^(\S*%s\S*):" % kernel, text, re.M).group(1)
    start = text.index("\n%s:" % name)
    return text[start:text.index(".Lfunc_end", start)]


def test_the_kernels_instructions_are_the_contracts(kernels):
    """Observe moves its state 16 bytes per access and reads the two Y dwords of its pair of pixels; the f64 divide is the
    correctly rounded sequence; neither kernel uses an atomic."""
    text = device_build()[0]
    observe, estimate = _body(text, "rl_error_observe_kernel"), _body(text, "rl_error_estimate_kernel")
    assert len(re.findall(r"\bglobal_load_dwordx4\b", observe)) >= 2 and len(re.findall(r"\bglobal_store_dwordx4\b", observe)) >= 2
    assert re.search(r"\bv_add_f64\b", observe) and re.search(r"\bv_mul_f64\b", observe) and re.search(r"\bv_div_fixup_f64\b", observe)
    assert re.search(r"\bv_div_fixup_f64\b", estimate) and re.search(r"\bv_cvt_f32_f64", estimate)
    assert "atomic" not in observe and "atomic" not in estimate


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_the_command_lines_rules_for_the_target(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "8", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base)
    assert a.target_error is None and a.min_observations is None and a.error_map is None
    a = CLI.parse_args(base + ["--target-error", "0.02"])
    assert a.target_error == 0.02 and a.min_observations is None and a.error_map is None and a.batches == 8
    a = CLI.parse_args(base + ["--target-error", "0.02", "--min-observations", "32", "--error-map", "map.png"])
    assert (a.target_error, a.min_observations, a.error_map) == (0.02, 32, "map.png")
    a = CLI.parse_args(base + ["--error-map", "map.png"])       # without a target: one estimate at the end
    assert a.target_error is None and a.error_map == "map.png"
    for args, words in ((["--min-observations", "32"], ("--min-observations", "--target-error")),
                        (["--target-error", "-1"], ("--target-error",)),
                        (["--target-error", "nan"], ("--target-error",)),
                        (["--target-error", "0.1", "--min-observations", "1"], ("--min-observations",)),
                        (["--direct", "--target-error", "0.1"], ("--target-error", "--direct")),
                        (["--direct", "--error-map", "m.png"], ("--error-map", "--direct"))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + args)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), (args, told)
