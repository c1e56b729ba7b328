"""The boundary of the adaptive sampler's C ABI without a GPU: struct layouts and entry points in every mirror, argument checks in
the documented order before any device work, no CPU fallback, and the command line's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
from _boundary import _Fake, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID, RL_E_STATE = -1, -5
FUNCTIONS = ("rl_adaptive_unit_create", "rl_adaptive_unit_destroy", "rl_adaptive_unit_plan", "rl_adaptive_unit_download_plan",
             "rl_adaptive_unit_samples", "rl_adaptive_unit_samples_device", "rl_plot_unit_render_adaptive")


def test_structs_and_entry_points_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert re.search(r"typedef struct RlAdaptiveUnit RlAdaptiveUnit;", header) and re.search(r"pub enum RlAdaptiveUnit \{\}", rust)
    assert C.sizeof(_lib.RlAdaptiveStats) == 40 and C.sizeof(_lib.RlCameraSample) == 48 and C.sizeof(_lib.RlPathResult) == 16
    offsets = {n: getattr(_lib.RlAdaptiveStats, n).offset for n, _ in _lib.RlAdaptiveStats._fields_}
    assert offsets == {"n_paths": 0, "tiles_x": 8, "tiles_y": 12, "min_count": 16, "max_count": 20, "min_weight": 24, "max_weight": 28,
                       "importance_sum": 32}
    assert re.search(r"typedef struct RlAdaptiveStats \{", header) and re.search(r"#\[repr\(C\)\][^\n]*pub struct RlAdaptiveStats \{", rust)
    for name in FUNCTIONS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
        c_args = re.search(r"int %s\(([^;]*)\);" % name, header).group(1).split(",")
        rust_args = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rust, re.S).group(1).split(",")
        assert len(c_args) == len(rust_args) == len(_lib.SIGNATURES[name][1]), name
    for name in ("rl_debug_adaptive_launches", "rl_debug_adaptive_ms"):
        assert re.search(r"int %s\(" % name, debug) and name in _lib.DEBUG_SIGNATURES
    assert len(R.adaptive_launches()) == 3 and _lib.lib.rl_debug_adaptive_launches(None) == RL_E_INVALID
    assert _lib.lib.rl_debug_adaptive_ms(None, None) == RL_E_INVALID
    assert _lib.lib.rl_adaptive_unit_destroy(None) == 0
    # the header states the rules the tests hold the unit to
    for rule in (r"q_t = u \* \(a_t / A\) \+ \(1 - u\) \* \(g_t / G\)", r"e_t = \(double\)n_paths \* q_t", "ties to the lower tile index",
                 r"w_t = \(float\)\(\(\(double\)n_paths \* a_t\) / \(A \* \(double\)c_t\)\)", r"px = x_lo \+ \(x_hi - x_lo\) \* u",
                 "independent but not identically distributed", "One user per adaptive unit"):
        assert re.search(rule, header), rule


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    """Every failure that comes before a device is touched, each with everything behind it wrong as well."""
    L = _lib.lib
    u, scene, plot, buf = _Fake().ptr, _Fake().ptr, _Fake().ptr, _Fake().ptr
    h = C.c_void_p()
    # create: a NULL out; a size below 2; the size limit -- before the device (an index no machine has)
    assert L.rl_adaptive_unit_create(99, 0, 0, None) == RL_E_INVALID and b"null" in _err()
    for w_, h_ in [(0, 36), (64, 0), (1, 36), (64, 1), (1, 1)]:
        assert L.rl_adaptive_unit_create(99, w_, h_, C.byref(h)) == RL_E_INVALID and b"at least 2" in _err(), (w_, h_)
    for w_, h_ in [(46341, 46341), (65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF)]:
        assert L.rl_adaptive_unit_create(99, w_, h_, C.byref(h)) == RL_E_INVALID and b"RL_MAX_PIXELS" in _err(), (w_, h_)
    assert not h.value
    # plan: a NULL unit, the share, the number of paths
    assert L.rl_adaptive_unit_plan(None, None, 0.0, 0, None) == RL_E_INVALID and b"null" in _err()
    for share in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert L.rl_adaptive_unit_plan(u, None, share, 0, None) == RL_E_INVALID and b"uniform_share" in _err(), share
    for n in (0, 1 << 32, (1 << 64) - 1):
        assert L.rl_adaptive_unit_plan(u, None, 0.5, n, None) == RL_E_INVALID and b"n_paths" in _err(), n
    # download_plan: a NULL unit, then no plan (a zeroed stand-in has none)
    assert L.rl_adaptive_unit_download_plan(None, buf, buf) == RL_E_INVALID and b"null" in _err()
    assert L.rl_adaptive_unit_download_plan(u, buf, buf) == RL_E_STATE and b"no plan" in _err()
    # samples: a NULL unit, a NULL scene, a NULL buffer -- then no plan
    for fn in (L.rl_adaptive_unit_samples, L.rl_adaptive_unit_samples_device):
        assert fn(None, None, 1, 0, (1 << 64) - 1, 0, 5, None) == RL_E_INVALID and b"adaptive unit" in _err()
        assert fn(u, None, 1, 0, (1 << 64) - 1, 0, 5, None) == RL_E_INVALID and b"scene" in _err()
        assert fn(u, scene, 1, 0, (1 << 64) - 1, 0, 5, None) == RL_E_INVALID and b"sample buffer" in _err()
        assert fn(u, scene, 1, 0, (1 << 64) - 1, 0, 5, buf) == RL_E_STATE and b"no plan" in _err()
        assert fn(u, scene, 1, 0, 0, 0, 0, None) == RL_E_STATE and b"no plan" in _err()          # (n = 0 is checked like any other)
    # render: NULL plot unit, NULL adaptive unit, NULL scene, the fetch mode, max_segments -- then no plan
    f = L.rl_plot_unit_render_adaptive
    assert f(None, None, None, 7, 1, 0, (1 << 64) - 1, 1 << 20) == RL_E_INVALID and b"plot unit" in _err()
    assert f(plot, None, None, 7, 1, 0, (1 << 64) - 1, 1 << 20) == RL_E_INVALID and b"adaptive unit" in _err()
    assert f(plot, u, None, 7, 1, 0, (1 << 64) - 1, 1 << 20) == RL_E_INVALID and b"scene" in _err()
    assert f(plot, u, scene, 7, 1, 0, (1 << 64) - 1, 1 << 20) == RL_E_INVALID and b"fetch" in _err()
    assert f(plot, u, scene, 0, 1, 0, (1 << 64) - 1, 1 << 20) == RL_E_INVALID and b"max_segments" in _err()
    assert f(plot, u, scene, 0, 1, 0, (1 << 64) - 1, 0) == RL_E_STATE and b"no plan" in _err()


def test_a_stand_in_with_a_plan_is_checked_for_its_range_size_and_device():
    """The checks behind the plan read the handles' first words only: a stand-in that says it has a plan of 1000 paths."""
    L = _lib.lib
    u, scene, plot, buf = _Fake(), _Fake(), _Fake(), _Fake().ptr
    words = C.cast(u.buf, C.POINTER(C.c_uint32))
    words[1], words[2] = 64, 36                                   # width, height (the device index comes first)
    # (RlAdaptiveUnit's first fields; rl_api.hip holds these offsets with static_asserts that name this test)
    C.cast(u.buf, C.POINTER(C.c_uint8))[20] = 1                    # planned
    C.cast(u.buf, C.POINTER(C.c_uint64))[3] = 1000                # n_paths
    for fn in (L.rl_adaptive_unit_samples, L.rl_adaptive_unit_samples_device):
        assert fn(u.ptr, scene.ptr, 1, 0, 0, 990, 11, buf) == RL_E_INVALID and b"past the end" in _err()
        assert fn(u.ptr, scene.ptr, 1, 0, 0, 1001, 0, buf) == RL_E_INVALID and b"past the end" in _err()
        assert fn(u.ptr, scene.ptr, 1, 0, (1 << 64) - 1000, 0, 1000, buf) == RL_E_INVALID and b"2^64" in _err()
        C.cast(scene.buf, C.POINTER(C.c_int32))[0] = 3            # another device
        assert fn(u.ptr, scene.ptr, 1, 0, 0, 0, 1000, buf) == RL_E_STATE and b"different devices" in _err()
        C.cast(scene.buf, C.POINTER(C.c_int32))[0] = 0
    f = L.rl_plot_unit_render_adaptive
    assert f(plot.ptr, u.ptr, scene.ptr, 0, 1, 0, (1 << 64) - 1000, 0) == RL_E_INVALID and b"2^64" in _err()
    assert f(plot.ptr, u.ptr, scene.ptr, 0, 1, 0, 0, 0) == RL_E_STATE and b"does not match" in _err()       # a plot unit of another size
    pw = C.cast(plot.buf, C.POINTER(C.c_uint32))
    pw[2], pw[3] = 64, 36                                         # (device, id, width, height)
    C.cast(scene.buf, C.POINTER(C.c_int32))[0] = 3
    assert f(plot.ptr, u.ptr, scene.ptr, 0, 1, 0, 0, 0) == RL_E_STATE and b"different devices" in _err()


@pytest.mark.skipif(R.device_count() > 0, reason="checks the no-GPU behaviour")
def test_the_adaptive_unit_fails_loudly_without_a_device():
    with pytest.raises(R.RlError) as e:
        R.AdaptiveUnit(64, 36)
    assert e.value.code == -2  # RL_E_NO_DEVICE: there is no CPU implementation to fall back to


def test_the_makefile_and_the_build_know_the_new_files():
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    assert "rl_adaptive.hip.h" in hdrs and "rl_adaptive_plan.h" in hdrs
    assert "tests/adaptive_host" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_command_lines_rules_for_adaptive(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "16", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base)
    assert a.adaptive is False and a.uniform_share is None
    a = CLI.parse_args(base + ["--target-error", "0.02", "--adaptive"])
    assert a.adaptive is True and a.uniform_share is None
    a = CLI.parse_args(base + ["--target-error", "0.02", "--adaptive", "--uniform-share", "0.5", "--error-map", "m.png"])
    assert (a.adaptive, a.uniform_share, a.error_map) == (True, 0.5, "m.png")
    a = CLI.parse_args(["--batches", "8", "--target-error", "0.02", "--adaptive", "--min-observations", "8"])
    assert a.min_observations == 8
    for args, words in ((["--adaptive"], ("--adaptive", "--target-error")),
                        (["--batches", "8", "--target-error", "0.1", "--adaptive"], ("--batches", "--min-observations")),
                        (["--target-error", "0.1", "--adaptive", "--min-observations", "17"], ("--batches", "--min-observations")),
                        (["--target-error", "0.1", "--uniform-share", "0.5"], ("--uniform-share", "--adaptive")),
                        (["--target-error", "0.1", "--adaptive", "--uniform-share", "0"], ("--uniform-share",)),
                        (["--target-error", "0.1", "--adaptive", "--uniform-share", "1.5"], ("--uniform-share",)),
                        (["--target-error", "0.1", "--adaptive", "--uniform-share", "nan"], ("--uniform-share",))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + args)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), (args, told)
