"""rl_robust_unit_estimate's C ABI without a GPU: the argument checks that come before the device, in the header's order and with
their messages, on a stand-in handle; RlErrorStats reused unchanged; the header, the ctypes table and the Rust binding in step; and
the compiled kernel's resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

from _device_build import kernels  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402

lib = _lib.lib
RL_E_INVALID, RL_E_NO_DEVICE, RL_E_STATE = -1, -2, -5


def last():
    return lib.rl_last_error().decode()


class _StandIn(C.Structure):
    """The first fields of a robust unit's handle, as the checks that come before any device work read them."""
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("n_buckets", C.c_uint32), ("stride", C.c_uint64),
                ("sums", C.c_void_p), ("trim", C.c_void_p), ("bucket_paths", C.c_uint64 * 32), ("observations", C.c_uint64),
                ("rest", C.c_uint8 * 512)]


def test_the_declarations_are_in_step_and_the_stats_struct_is_the_error_units():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    assert ("int rl_robust_unit_estimate(RlRobustUnit* unit, const RlRobustParams* params, RlErrorStats* stats, float* se, double* tiles, "
            "uint8_t* trim);") in header
    assert len(re.findall(r"typedef struct RlErrorStats \{", header)) == 1 and C.sizeof(_lib.RlErrorStats) == 64
    assert header.index("} RlErrorStats;") < header.index("int rl_robust_unit_estimate(")
    assert [n for n, _ in _lib.RlErrorStats._fields_] == ["observations", "paths", "tiles_x", "tiles_y", "worst_tile_x", "worst_tile_y", "sum_y",
                                                         "sum_se", "relative_error", "worst_tile_error"]
    assert "rl_robust_unit_estimate" in _lib.SIGNATURES and len(_lib.SIGNATURES["rl_robust_unit_estimate"][1]) == 6
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert re.search(r"pub fn rl_robust_unit_estimate\(unit: \*mut RlRobustUnit, params: \*const RlRobustParams, stats: \*mut RlErrorStats", rust)
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert "int rl_debug_robust_estimate_launches(uint64_t* out);" in debug and "int rl_debug_robust_launches(uint64_t out[2]);" in debug
    assert "rl_debug_robust_estimate_launches" in _lib.DEBUG_SIGNATURES
    for name in ("estimate", "estimate_ms"):
        assert callable(getattr(R.RobustUnit, name))
    assert callable(R.robust_estimate_launches) and callable(R.render_robust_to_error)


def test_the_null_checks_come_first():
    params, stats = _lib.RlRobustParams(1.0, 0xFFFFFFFF, 0), _lib.RlErrorStats()
    bad = _lib.RlRobustParams(float("nan"), 0, 0)
    unit = C.byref(_StandIn())                                           # (no bucket holds a path: the null check still comes first)
    for u, p, s in ((None, C.byref(params), C.byref(stats)), (unit, None, C.byref(stats)), (unit, C.byref(params), None),
                    (None, None, None), (None, C.byref(bad), C.byref(stats)), (unit, C.byref(bad), None)):
        assert lib.rl_robust_unit_estimate(u, p, s, None, None, None) == RL_E_INVALID and "null robust unit, params or stats" in last()
    assert lib.rl_debug_robust_estimate_launches(None) == RL_E_INVALID
    assert lib.rl_debug_robust_estimate_ms(None, None) == RL_E_INVALID
    before = C.c_uint64(99)
    assert lib.rl_debug_robust_estimate_launches(C.byref(before)) == 0 and before.value == R.robust_estimate_launches()


def test_a_stand_in_handle_is_checked_in_the_stated_order():
    """gain, then the empty buckets, and only then the device; nothing is written to the stats."""
    s = _StandIn(device=0, width=4, height=4, n_buckets=5, stride=16)
    unit = C.byref(s)
    stats = _lib.RlErrorStats()
    stats.observations, stats.relative_error = 77, 0.5
    for gain in (float("nan"), -1.0, -0.5, -float("inf")):              # before the empty buckets
        assert lib.rl_robust_unit_estimate(unit, C.byref(_lib.RlRobustParams(gain, 0, 0)), C.byref(stats), None, None, None) == RL_E_INVALID
        assert "rl_robust_unit_estimate: gain is negative or not a number" in last()
    for gain in (0.0, 1.0, float("inf")):                               # legal gains reach the next check
        assert lib.rl_robust_unit_estimate(unit, C.byref(_lib.RlRobustParams(gain, 0, 0)), C.byref(stats), None, None, None) == RL_E_STATE
        assert "rl_robust_unit_estimate: bucket 0 holds no paths: every bucket needs an observation" in last()
    for j in range(5):
        s.bucket_paths[j] = 1 if j != 3 else 0
    assert lib.rl_robust_unit_estimate(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), C.byref(stats), None, None, None) == RL_E_STATE
    assert "bucket 3 holds no paths" in last()
    s.bucket_paths[3] = 1
    s.bucket_paths[0] = 0xFFFFFFFFFFFFFFFF                              # every bucket filled, and N past 64 bits
    assert lib.rl_robust_unit_estimate(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), C.byref(stats), None, None, None) == RL_E_STATE
    assert "overflows 64 bits" in last()
    s.bucket_paths[0] = 1
    if R.device_count() == 0:                                           # what comes next is the device
        assert lib.rl_robust_unit_estimate(unit, C.byref(_lib.RlRobustParams(1.0, 0, 0)), C.byref(stats), None, None, None) == RL_E_NO_DEVICE
    assert (stats.observations, stats.relative_error) == (77, 0.5)
    assert list(s.bucket_paths)[:5] == [1] * 5 and s.observations == 0


def test_the_estimate_kernel_is_free_of_scratch_and_spills(kernels):
    estimate = [k for n, k in kernels.items() if "rl_robust_estimate_kernel" in n]
    assert len(estimate) == 1, sorted(kernels)
    k = estimate[0]
    print("rl_robust_estimate_kernel: %d VGPRs, %d SGPRs, %d SGPRs spilled, %d VGPRs spilled, %d bytes of scratch, %d bytes of static LDS"
          % (k["vgpr_count"], k["sgpr_count"], k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"],
             k["group_segment_fixed_size"]))
    assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0, k
    assert k.get("agpr_count", 0) == 0, k
    assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 0       # one tile; the LDS is the launch's
    # four workgroups of 256 threads per CU at M = 15 (34,560 B of LDS each) are four waves per SIMD: 128 VGPRs leave room for them
    assert k["vgpr_count"] <= 128, k
    # the resolve and the error estimate are still there, one of each
    for name in ("rl_robust_resolve_kernel", "rl_robust_observe_kernel", "rl_error_estimate_kernel"):
        assert len([n for n in kernels if name in n]) == 1, name
