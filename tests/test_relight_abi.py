"""The relight film's C ABI without a GPU: every argument check that comes before the device, in the header's order and with its
message; the constants and the argument order of the bindings; and the compiled kernels' resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _device_build import kernels  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402

lib = _lib.lib
RL_E_INVALID, RL_E_NO_DEVICE, RL_E_STATE = -1, -2, -5
POISON = 0xDEAD0


def last():
    return lib.rl_last_error().decode()


def test_constants_and_the_argument_order_of_the_bindings():
    assert (_lib.RL_RELIGHT_MAX_GROUPS, _lib.RL_RELIGHT_DROP) == (16, 0xFF) == (R.RL_RELIGHT_MAX_GROUPS, R.RL_RELIGHT_DROP)
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    assert re.search(r"#define RL_RELIGHT_MAX_GROUPS 16\b", header) and re.search(r"#define RL_RELIGHT_DROP 0xff\b", header)
    vp, u32, u64, i, f = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
    S = _lib.SIGNATURES
    assert S["rl_relight_unit_create"] == (i, [i, u32, u32, u32, u32, C.POINTER(C.c_void_p)])       # device, width, height, nodes, groups, out
    assert S["rl_relight_unit_set_groups"] == (i, [vp, vp, u32])
    assert S["rl_relight_unit_plot_results"] == S["rl_relight_unit_plot_results_device"] == (i, [vp, vp, vp, u64])
    assert S["rl_relight_unit_render"] == (i, [vp, vp, i, u64, u32, u64, u64, u32])                   # unit, scene, fetch, seed, stream, first, n, max
    assert S["rl_relight_unit_mix"] == (i, [vp, vp, vp, vp])                                         # unit, gains, matrix, dst
    assert S["rl_relight_gains_black_body"] == (i, [u32, f, f, f, f, vp])
    assert _lib.DEBUG_SIGNATURES["rl_debug_relight_launches"] == (i, [vp])
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert "int rl_debug_relight_launches(uint64_t out[3]);" in debug and "rl_debug_relight" not in header
    assert "rl_debug_relight" not in open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    out = (C.c_uint64 * 3)(7, 7, 7)
    assert lib.rl_debug_relight_launches(out) == 0 and 7 not in list(out)
    assert lib.rl_debug_relight_launches(None) == RL_E_INVALID
    assert "rl_relight.hip.h" in re.search(r"^HDRS = (.*)$", open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read(), re.M).group(1)
    for name in ("set_groups", "plot_results", "render", "clear", "download", "upload", "mix", "launch_ms"):
        assert callable(getattr(R.RelightUnit, name))


def test_create_checks_its_arguments_in_order_before_the_device():
    """Null output, zero size, the node count, the group count, pixels x nodes x groups, and only then the device; the handle is
    left null."""
    def create(w, h, nodes, groups, out):
        return lib.rl_relight_unit_create(0, w, h, nodes, groups, out)

    def refused(w, h, nodes, groups, message):
        handle = C.c_void_p(POISON)
        assert create(w, h, nodes, groups, C.byref(handle)) == RL_E_INVALID, (message, w, h, nodes, groups, last())
        assert message in last() and handle.value is None, (message, w, h, nodes, groups, last(), handle.value)

    for args in ((4, 4, 81, 3), (0, 0, 81, 3), (4, 4, 1, 3), (4, 4, 81, 0), (65536, 65536, 81, 3)):   # the null output comes first
        assert create(*args, None) == RL_E_INVALID and last() == "null output handle"
    for nodes, groups in ((81, 3), (1, 3), (81, 17), (0, 0)):                                          # ... then the zero size
        for w, h in [(0, 4), (4, 0), (0, 0), (0, 0xFFFFFFFF)]:
            refused(w, h, nodes, groups, "zero-sized relight unit")
    for nodes in (0, 1, 402, 0xFFFFFFFF):                                                              # ... then the node count
        for groups, (w, h) in ((3, (4, 4)), (0, (4, 4)), (17, (65536, 65536))):
            refused(w, h, nodes, groups, "relight unit: n_nodes %d outside 2 .. RL_SPECTRAL_MAX_NODES = 401" % nodes)
    for groups in (0, 17, 255, 0xFFFFFFFF):                                                            # ... then the group count
        for w, h in ((4, 4), (65536, 65536)):
            refused(w, h, 81, groups, "relight unit: n_groups %d outside 1 .. RL_RELIGHT_MAX_GROUPS = 16" % groups)
    for w, h, nodes, groups in [(46341, 46341, 2, 1), (4096, 4096, 81, 3), (1280, 720, 401, 16), (0xFFFFFFFF, 0xFFFFFFFF, 401, 16),
                                (1 << 20, 1, 128, 16), (65536, 32768, 2, 1)]:                          # ... then the size, in 64 bits
        refused(w, h, nodes, groups, "relight unit: %d x %d pixels x %d nodes x %d groups exceed RL_MAX_PIXELS = 2^31 - 1" % (w, h, nodes, groups))
    if R.device_count() == 0:                                                                          # what comes next is the device
        for nodes, groups in ((2, 1), (81, 3), (401, 16)):
            handle = C.c_void_p(POISON)
            assert create(4, 4, nodes, groups, C.byref(handle)) == RL_E_NO_DEVICE and handle.value is None, last()
        with pytest.raises(R.RlError) as e:
            R.RelightUnit(64, 36, 81, 3)
        assert e.value.code == RL_E_NO_DEVICE


class _StandIn(C.Structure):
    """The first fields of a relight unit's handle, as the checks that come before any device work read them."""
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("n_nodes", C.c_uint32), ("n_groups", C.c_uint32),
                ("n_objects", C.c_uint32), ("rest", C.c_uint8 * 512)]


def test_the_null_checks_of_every_call():
    unit, other = C.byref(_StandIn(0, 4, 4, 5, 3, 0)), C.byref(_StandIn())
    table = np.zeros(4, np.uint8)
    T = table.ctypes.data_as(C.c_void_p)
    assert lib.rl_relight_unit_destroy(None) == 0
    assert lib.rl_relight_unit_clear(None) == RL_E_INVALID and "null relight unit" in last()
    for u, t in ((None, T), (unit, None), (None, None)):
        assert lib.rl_relight_unit_set_groups(u, t, 4) == RL_E_INVALID and "null relight unit or table" in last()
    for fn in (lib.rl_relight_unit_plot_results, lib.rl_relight_unit_plot_results_device):
        assert fn(None, other, other, 5) == RL_E_INVALID and "null relight unit" in last()
        assert fn(None, None, None, 0) == RL_E_INVALID and "null relight unit" in last()
        for s, r in ((None, other), (other, None), (None, None)):
            assert fn(unit, s, r, 5) == RL_E_INVALID and "null sample or result buffer" in last()
    assert lib.rl_relight_unit_render(None, other, 0, 1, 0, 0, 1, 0) == RL_E_INVALID and "null relight unit" in last()
    assert lib.rl_relight_unit_render(unit, None, 0, 1, 0, 0, 1, 0) == RL_E_INVALID and "null scene" in last()
    for u, o in ((None, other), (unit, None)):
        assert lib.rl_relight_unit_download(u, o) == RL_E_INVALID and lib.rl_relight_unit_upload(u, o) == RL_E_INVALID
    for u, m, d in ((None, other, other), (unit, None, other), (unit, other, None)):
        assert lib.rl_relight_unit_mix(u, None, m, d) == RL_E_INVALID and "null relight unit, matrix or dst" in last()
    assert lib.rl_debug_relight_ms(None, None) == RL_E_INVALID


def test_a_stand_in_handle_is_checked_in_the_stated_order():
    """The checks that read a handle before any device work, on a stand-in for one (no device here, none needed)."""
    s = _StandIn(device=0, width=4, height=4, n_nodes=5, n_groups=3, n_objects=0)
    unit = C.byref(s)
    # set_groups: n_objects == 0, then every entry; a refused table changes nothing
    ok = np.array([0, 2, 255, 1], np.uint8)
    assert lib.rl_relight_unit_set_groups(unit, ok.ctypes.data_as(C.c_void_p), 0) == RL_E_INVALID and "n_objects is 0" in last()
    for where, value in ((0, 3), (3, 16), (2, 254), (1, 128)):
        bad = ok.copy()
        bad[where] = value
        assert lib.rl_relight_unit_set_groups(unit, bad.ctypes.data_as(C.c_void_p), 4) == RL_E_INVALID
        assert "object %d has group %d" % (where, value) in last() and "n_groups = 3" in last()
    assert s.n_objects == 0
    # without a table: RL_E_STATE, after the null checks and before anything else
    scene = C.byref((C.c_uint8 * 8192)())
    for fn in (lib.rl_relight_unit_plot_results, lib.rl_relight_unit_plot_results_device):
        for n in (0, 5):
            assert fn(unit, scene, scene, n) == RL_E_STATE and "has no table" in last()
    assert lib.rl_relight_unit_render(unit, scene, 7, 1, 0, 0, 1, 0) == RL_E_INVALID and "fetch" in last()          # the fetch mode first
    assert lib.rl_relight_unit_render(unit, scene, 0, 1, 0, 0, 1, 65537) == RL_E_INVALID and "max_segments" in last()
    assert lib.rl_relight_unit_render(unit, scene, 0, 1, 0, 2 ** 64 - 2, 1, 0) == RL_E_STATE and "has no table" in last()  # before the range
    # with one: the path range, then the scene's object count (the stand-in scene is all zero bytes: no object)
    s.n_objects = 4
    for first, n in ((2 ** 64 - 2, 1), (2 ** 64 - 1, 0), (1, 2 ** 64 - 2), (2 ** 63, 2 ** 63)):
        assert lib.rl_relight_unit_render(unit, scene, 0, 1, 0, first, n, 0) == RL_E_INVALID and "2^64 - 1" in last()
    assert lib.rl_relight_unit_render(unit, scene, 0, 1, 0, 0, 0, 0) == RL_E_STATE and "4 objects and the scene 0" in last()   # n_paths = 0 too
    # mix: a dst of another size or device is RL_E_STATE before the device
    class Gather(C.Structure):
        _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("rest", C.c_uint8 * 512)]
    matrix = np.zeros((5, 3), np.float32)
    for dst in (Gather(0, 9, 9), Gather(0, 4, 5), Gather(1, 4, 4)):
        assert lib.rl_relight_unit_mix(unit, None, matrix.ctypes.data_as(C.c_void_p), C.byref(dst)) == RL_E_STATE
        assert "gather unit does not match the relight unit" in last()


def test_the_new_kernels_keep_to_32_vgprs_without_scratch_or_lds_and_the_mix_is_the_projection_kernel(kernels):
    splat = [k for n, k in kernels.items() if "rl_relight_splat_kernel" in n]
    rays = [k for n, k in kernels.items() if "rl_relight_rays_kernel" in n]
    assert len(splat) == 1 and len(rays) == 1, sorted(kernels)
    assert sorted(n for n in kernels if "relight" in n) == sorted(n for n in kernels if "rl_relight_splat_kernel" in n or "rl_relight_rays_kernel" in n)
    for what, k in (("splat", splat[0]), ("rays", rays[0])):
        print("rl_relight_%s_kernel: %d VGPRs, %d SGPRs, %d SGPRs spilled, %d VGPRs spilled, %d bytes of scratch, %d bytes of static LDS"
              % (what, k["vgpr_count"], k["sgpr_count"], k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"],
                 k["group_segment_fixed_size"]))
        assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0, (what, k)
        assert k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0 and k["group_segment_fixed_size"] == 0, (what, k)
        assert k.get("agpr_count", 0) == 0 and k["vgpr_count"] <= 32, (what, k)
    # the mix launches rl_spectral_project_kernel on the composed matrix: there is no mix kernel of its own
    source = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "rl_api.hip")).read()
    body = source[source.index("int rl_relight_unit_mix("):source.index("int rl_relight_gains_black_body(")]
    assert "rl_spectral_project_kernel" in body
