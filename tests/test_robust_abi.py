"""The robust film's C ABI without a GPU: every argument check that comes before the device, in the header's order and with its
message; rl_robust_params_default; the struct sizes; and the compiled kernels' resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _robust_cases as RC
from _device_build import kernels  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402

lib = _lib.lib
RL_E_INVALID, RL_E_NO_DEVICE, RL_E_STATE = -1, -2, -5
POISON = 0xDEAD0


def last():
    return lib.rl_last_error().decode()


def test_struct_sizes_constants_and_defaults():
    assert C.sizeof(_lib.RlRobustParams) == 16 and C.sizeof(_lib.RlRobustStats) == 48
    assert (_lib.RL_ROBUST_MAX_BUCKETS, _lib.RL_ROBUST_NEXT) == (32, 0xFFFFFFFF) == (R.RL_ROBUST_MAX_BUCKETS, R.RL_ROBUST_NEXT)
    assert (RC.NEXT, RC.NO_LIMIT) == (0xFFFFFFFF, 0xFFFFFFFF)
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    assert re.search(r"#define RL_ROBUST_MAX_BUCKETS 32\b", header) and re.search(r"#define RL_ROBUST_NEXT 0xffffffffu\b", header)
    p = _lib.RlRobustParams(-1.0, 7, 9)
    assert lib.rl_robust_params_default(C.byref(p)) == 0
    assert (p.gain, p.max_trim, p.reserved) == (1.0, 0xFFFFFFFF, 0)
    assert lib.rl_robust_params_default(None) == RL_E_INVALID


def test_create_checks_its_arguments_in_order_before_the_device():
    """Null output, zero size, RL_MAX_PIXELS, the bucket count, and only then the device; the handle is left null."""
    def create(w, h, m, out):
        return lib.rl_robust_unit_create(0, w, h, m, out)

    def refused(w, h, m, message):
        handle = C.c_void_p(POISON)
        assert create(w, h, m, C.byref(handle)) == RL_E_INVALID, (message, w, h, m, last())
        assert message in last() and handle.value is None, (message, w, h, m, last(), handle.value)

    for m in (15, 0, 2, 33):                                            # the null output comes first, whatever else is wrong
        assert create(4, 4, m, None) == RL_E_INVALID and last() == "null output handle"
        assert create(0, 0, m, None) == RL_E_INVALID and last() == "null output handle"
        assert create(46341, 46341, m, None) == RL_E_INVALID and last() == "null output handle"
    for m in (15, 0, 2, 33, 0xFFFFFFFF):                                # ... then the zero size, before RL_MAX_PIXELS and the buckets
        for w, h in [(0, 4), (4, 0), (0, 0), (0, 0xFFFFFFFF)]:
            refused(w, h, m, "zero-sized robust unit")
        for w, h in [(46341, 46341), (65536, 32768), (32768, 65536), (0xFFFFFFFF, 0xFFFFFFFF), (0x80000000, 1)]:
            refused(w, h, m, "robust unit: %d x %d pixels" % (w, h))
            assert "exceed RL_MAX_PIXELS = 2^31 - 1" in last()
    for m in (0, 1, 2, 33, 34, 0xFFFFFFFF):                             # ... then the bucket count
        refused(4, 4, m, "robust unit: n_buckets %d outside 3 .. RL_ROBUST_MAX_BUCKETS = 32" % m)
    if R.device_count() == 0:                                           # what comes next is the device
        for m in (3, 15, 32):
            handle = C.c_void_p(POISON)
            assert create(4, 4, m, C.byref(handle)) == RL_E_NO_DEVICE and handle.value is None, last()
        with pytest.raises(R.RlError) as e:
            R.RobustUnit(64, 36)
        assert e.value.code == RL_E_NO_DEVICE


class _StandIn(C.Structure):
    """The first fields of a robust unit's handle, as the checks that come before any device work read them."""
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("n_buckets", C.c_uint32), ("stride", C.c_uint64),
                ("sums", C.c_void_p), ("trim", C.c_void_p), ("bucket_paths", C.c_uint64 * 32), ("observations", C.c_uint64),
                ("rest", C.c_uint8 * 512)]


def test_the_null_checks_of_every_call():
    params = _lib.RlRobustParams(1.0, 0xFFFFFFFF, 0)
    unit, other = C.byref(_StandIn()), C.byref(_StandIn())
    assert lib.rl_robust_unit_destroy(None) == 0
    assert lib.rl_robust_unit_clear(None) == RL_E_INVALID and "null robust unit" in last()
    for u, plot in ((None, other), (unit, None), (None, None)):
        assert lib.rl_robust_unit_observe(u, plot, 1, 0) == RL_E_INVALID and "null robust unit or plot unit" in last()
    for u, p, dst in ((None, C.byref(params), other), (unit, None, other), (unit, C.byref(params), None)):
        assert lib.rl_robust_unit_resolve(u, p, dst, None, None) == RL_E_INVALID and "null robust unit, params or dst" in last()
    assert lib.rl_robust_unit_download(None, None, None, None) == RL_E_INVALID and "null robust unit" in last()
    sums, paths = np.zeros(9 * 16), np.ones(3, np.uint64)
    for u, s, n in ((None, sums, paths), (unit, None, paths), (unit, sums, None)):
        assert lib.rl_robust_unit_upload(u, s.ctypes.data_as(C.c_void_p) if s is not None else None,
                                         n.ctypes.data_as(C.c_void_p) if n is not None else None, 3) == RL_E_INVALID
        assert "null robust unit, sums or bucket_paths" in last()


def test_a_stand_in_handle_is_checked_in_the_stated_order():
    """The checks that read a handle before any device work, on a stand-in for one (no device here, none needed): observe's
    n_paths, bucket and overflow, in this order, before the plot unit is looked at; resolve's gain, then the empty bucket; upload's
    observations."""
    s = _StandIn(device=0, width=4, height=4, n_buckets=5, stride=16)
    unit, other = C.byref(s), C.byref(_StandIn(device=0, width=9, height=9))
    assert lib.rl_robust_unit_observe(unit, other, 0, 99) == RL_E_INVALID and "n_paths is 0" in last()      # n_paths before the bucket
    for bucket in (5, 6, 32, 0xFFFFFFFE):
        assert lib.rl_robust_unit_observe(unit, other, 1, bucket) == RL_E_INVALID and "bucket %d of 5" % bucket in last()
    s.bucket_paths[2] = 0xFFFFFFFFFFFFFFFF
    assert lib.rl_robust_unit_observe(unit, other, 1, 2) == RL_E_INVALID and "overflows 64 bits" in last()   # n[j] itself
    assert lib.rl_robust_unit_observe(unit, other, 1, 1) == RL_E_INVALID and "overflows 64 bits" in last()   # the total
    s.observations = 7                                                                                       # RL_ROBUST_NEXT: 7 mod 5 = 2
    assert lib.rl_robust_unit_observe(unit, other, 1, 0xFFFFFFFF) == RL_E_INVALID and "overflows 64 bits" in last()
    s.bucket_paths[2] = 0x8000000000000000
    s.bucket_paths[4] = 0x7FFFFFFFFFFFFFFF
    assert lib.rl_robust_unit_observe(unit, other, 1, 0) == RL_E_INVALID and "overflows 64 bits" in last()   # the total alone
    s.bucket_paths[2] = s.bucket_paths[4] = 0
    # the overflow check is passed: a plot unit of another size is RL_E_STATE, still before the device (the stand-in for the plot
    # unit is read for its device and size only: id sits between them)
    class Plot(C.Structure):
        _fields_ = [("device", C.c_int), ("id", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("rest", C.c_uint8 * 512)]
    assert lib.rl_robust_unit_observe(unit, C.byref(Plot(0, 0, 9, 9)), 1, 0) == RL_E_STATE and "plot unit does not match the robust unit" in last()
    # ... and so is one of the same size on another device
    assert lib.rl_robust_unit_observe(unit, C.byref(Plot(1, 0, 4, 4)), 1, 0) == RL_E_STATE and "plot unit does not match the robust unit" in last()
    assert list(s.bucket_paths) == [0] * 32 and s.observations == 7                                          # nothing was counted

    class Gather(C.Structure):
        _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("rest", C.c_uint8 * 512)]
    dst = C.byref(Gather(0, 9, 9))
    for gain in (float("nan"), -1.0, -0.5, -float("inf")):
        assert lib.rl_robust_unit_resolve(unit, C.byref(_lib.RlRobustParams(gain, 0, 0)), dst, None, None) == RL_E_INVALID
        assert "gain is negative or not a number" in last()
    for gain in (0.0, 1.0, float("inf")):                               # legal gains reach the next check: the empty buckets
        assert lib.rl_robust_unit_resolve(unit, C.byref(_lib.RlRobustParams(gain, 0, 0)), dst, None, None) == RL_E_STATE
        assert "bucket 0 holds no paths: every bucket needs an observation" in last()
    for j in range(5):
        s.bucket_paths[j] = 1 if j != 3 else 0
    assert lib.rl_robust_unit_resolve(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), dst, None, None) == RL_E_STATE
    assert "bucket 3 holds no paths" in last()
    s.bucket_paths[3] = 1                                               # every bucket filled: now the dst of another size
    assert lib.rl_robust_unit_resolve(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), dst, None, None) == RL_E_STATE
    assert "gather unit does not match the robust unit" in last()
    assert lib.rl_robust_unit_resolve(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), C.byref(Gather(1, 4, 4)), None, None) == RL_E_STATE
    assert "gather unit does not match the robust unit" in last()                                            # the same size, another device

    sums = np.zeros(5 * 3 * 16)
    paths = np.array([1, 0, 2, 0, 3], np.uint64)
    for k in (0, 1, 2):                                                 # three buckets are filled: at least three observations
        assert lib.rl_robust_unit_upload(unit, sums.ctypes.data_as(C.c_void_p), paths.ctypes.data_as(C.c_void_p), k) == RL_E_INVALID
        assert "%d observations cannot have filled 3 buckets" % k in last()
    paths = np.array([1 << 63, 1 << 63, 0, 0, 0], np.uint64)
    assert lib.rl_robust_unit_upload(unit, sums.ctypes.data_as(C.c_void_p), paths.ctypes.data_as(C.c_void_p), 2) == RL_E_INVALID
    assert "overflows 64 bits" in last()
    assert list(s.bucket_paths)[:5] == [1] * 5 and s.observations == 7  # a refused upload changes nothing


def test_the_python_class_follows_the_error_units():
    for name in ("observe", "resolve", "download", "upload", "clear", "launch_ms"):
        assert callable(getattr(R.RobustUnit, name))
    assert "rl_robust.hip.h" in re.search(r"^HDRS = (.*)$", open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read(), re.M).group(1)


def test_both_kernels_are_free_of_scratch_and_spills_and_observe_keeps_to_32_vgprs(kernels):
    observe = [k for n, k in kernels.items() if "rl_robust_observe_kernel" in n]
    resolve = [k for n, k in kernels.items() if "rl_robust_resolve_kernel" in n]
    assert len(observe) == 1 and len(resolve) == 1, sorted(kernels)
    for what, k in (("observe", observe[0]), ("resolve", resolve[0])):
        print("rl_robust_%s_kernel: %d VGPRs, %d SGPRs, %d SGPRs spilled, %d VGPRs spilled, %d bytes of scratch, %d bytes of static LDS"
              % (what, k["vgpr_count"], k["sgpr_count"], k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"],
                 k["group_segment_fixed_size"]))
        assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0, (what, k)
        assert k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0, (what, k)
        assert k.get("agpr_count", 0) == 0, (what, k)
    # what four resident waves per SIMD of an open trace kernel leave free: the observation runs beside it, not behind it
    assert observe[0]["vgpr_count"] <= 32, observe[0]
    assert resolve[0]["max_flat_workgroup_size"] == 64 and resolve[0]["group_segment_fixed_size"] == 0   # one wave; the LDS is the launch's
