"""Scene.occluded at the boundary, without a GPU: the two entry points (exported, bound in the ctypes mirror, declared in the Rust
binding), their argument checks -- rl_scene_intersect's, in its order, before any device work -- and the compiled occlusion
kernel's resources (hipcc cross-compiles here): six instantiations, each free of scratch memory and vector-register spills, at
four waves per SIMD, with no more spilled scalar registers than the query kernel's variant of the same stage; and the other ray
kernels still counted as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from _device_build import kernels, variant_of_name  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
VARIANTS = 6   # (nothing / the tables / the whole scene staged in LDS) x prisms with / without a second bound
NAMES = ("rl_scene_occluded", "rl_scene_occluded_device")


def test_both_entry_points_are_exported_bound_and_in_the_rust_binding():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("occluded", "intersect")]   # (pointers are void* in the mirror)
        assert re.search(r"\bint %s\(const RlScene\* scene, int primitive_fetch, const RlRay\* \w+, uint32_t n_rays,\s+uint8_t\* \w+\);" % name, header)
        assert re.search(r"pub fn %s\(" % name, rust)
    assert hasattr(R.Scene, "occluded") and hasattr(R.Scene, "occluded_device")
    assert hasattr(_lib.lib, "rl_debug_occlusion_launches") and "rl_debug_occlusion_launches" in _lib.DEBUG_SIGNATURES
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert "int rl_debug_occlusion_launches(uint64_t* out);" in debug
    assert "rl_debug_" not in rust


@pytest.mark.parametrize("name", NAMES)
def test_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    rays, out = np.zeros(4, R.RAY_DTYPE), np.full(4 + 64, 0xAA, np.uint8)
    rp, op = rays.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    before = R.occlusion_launches()
    # an unknown fetch mode comes first, then the NULL arrays, then the NULL scene: rl_scene_intersect's order
    assert fn(None, 7, None, 4, None) == RL_E_INVALID and b"fetch" in _lib.lib.rl_last_error()
    assert fn(None, -1, rp, 4, op) == RL_E_INVALID and b"fetch" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_GLOBAL, None, 4, op) == RL_E_INVALID and b"buffer" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_LDS, rp, 4, None) == RL_E_INVALID and b"buffer" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_LDS, rp, 4, op) == RL_E_INVALID and b"scene" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_LDS, None, 0, None) == RL_E_INVALID and b"scene" in _lib.lib.rl_last_error()
    assert (out == 0xAA).all()   # nothing written
    assert R.occlusion_launches() == before and len(before) == VARIANTS   # nothing launched
    assert _lib.lib.rl_debug_occlusion_launches(None) == RL_E_INVALID


def test_six_occlusion_kernels_free_of_scratch_and_vector_spills(kernels):
    mine = {n: k for n, k in kernels.items() if "rl_occlusion_kernel" in n}
    assert len(mine) == VARIANTS, sorted(mine)
    assert sorted(variant_of_name(n, "rl_occlusion_kernel") for n in mine) == [(s, c) for s in "012" for c in "01"]
    query = {variant_of_name(n, "rl_query_kernel"): k for n, k in kernels.items() if "rl_query_kernel" in n}
    for name, k in mine.items():
        # the other *_abi.py tests count their kernels by these substrings
        for other in ("rl_query_kernel", "rl_step_kernel", "rl_ray_paths_kernel", "rl_film_", "rl_trace_kernel"):
            assert other not in name, name
        assert k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0, (name, k)   # no scratch memory
        assert k["vgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)             # four waves per SIMD, no AGPRs
        q = query[variant_of_name(name, "rl_occlusion_kernel")]
        assert k["sgpr_spill_count"] <= q["sgpr_spill_count"], (name, k["sgpr_spill_count"], q["sgpr_spill_count"])


def test_occlusion_header_is_part_of_the_build_id():
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HDRS = .*\brl_occlusion\.hip\.h\b", make, re.M)


def test_the_other_ray_kernels_are_counted_as_before(kernels):
    count = lambda sub: sum(1 for n in kernels if sub in n)
    assert count("rl_trace_kernel") == 24
    assert count("rl_query_kernel") == 6 and count("rl_ray_paths_kernel") == 6 and count("rl_film_paths_kernel") == 6 and count("rl_step_kernel") == 6
