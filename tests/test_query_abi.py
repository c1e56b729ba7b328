"""Scene.intersect at the boundary, without a GPU: the frozen layouts of RlRay / RlIntersection / RlRayHit (header, ctypes mirror,
numpy dtypes), the two entry points and their argument checks, and the compiled query kernel's resources (hipcc cross-compiles
here): every instantiation free of scratch memory and spills."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from _device_build import device_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robigo_luculenta_amd", "csrc")
RL_E_INVALID = -1
QUERY_VARIANTS = 6   # (nothing / the tables / the whole scene staged in LDS) x prisms with / without a second bound


def test_query_records_have_their_frozen_layouts():
    assert C.sizeof(_lib.RlRay) == 32 and C.sizeof(_lib.RlIntersection) == 40 and C.sizeof(_lib.RlRayHit) == 48
    assert [(f, getattr(_lib.RlRay, f).offset) for f, _ in _lib.RlRay._fields_] == [("origin", 0), ("t_max", 12), ("direction", 16),
                                                                                      ("reserved", 28)]
    assert [(f, getattr(_lib.RlIntersection, f).offset) for f, _ in _lib.RlIntersection._fields_] == [
        ("position", 0), ("normal", 12), ("tangent", 24), ("distance", 36)]
    assert [(f, getattr(_lib.RlRayHit, f).offset) for f, _ in _lib.RlRayHit._fields_] == [("isect", 0), ("object", 40), ("reserved", 44)]
    assert R.RAY_DTYPE.itemsize == 32 and R.HIT_DTYPE.itemsize == 48
    assert [(n, R.RAY_DTYPE.fields[n][1]) for n in R.RAY_DTYPE.names] == [("origin", 0), ("t_max", 12), ("direction", 16), ("reserved", 28)]
    assert [(n, R.HIT_DTYPE.fields[n][1]) for n in R.HIT_DTYPE.names] == [("position", 0), ("normal", 12), ("tangent", 24), ("distance", 36),
                                                                          ("object", 40), ("reserved", 44)]
    assert R.RL_OBJECT_NONE == 0xffffffff
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    assert re.search(r"#define RL_OBJECT_NONE 0xffffffffu\b", header)


def test_both_entry_points_are_exported():
    for name in ("rl_scene_intersect", "rl_scene_intersect_device"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.lib, "rl_debug_query_launches") and "rl_debug_query_launches" in _lib.DEBUG_SIGNATURES


@pytest.mark.parametrize("name", ["rl_scene_intersect", "rl_scene_intersect_device"])
def test_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    rays, hits = np.zeros(4, R.RAY_DTYPE), np.zeros(4, R.HIT_DTYPE)
    rp, hp = rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    assert fn(None, R.FETCH_LDS, rp, 4, hp) == RL_E_INVALID and b"scene" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_LDS, None, 0, None) == RL_E_INVALID and b"scene" in _lib.lib.rl_last_error()
    assert fn(None, 7, rp, 4, hp) == RL_E_INVALID and b"fetch" in _lib.lib.rl_last_error()
    assert fn(None, -1, rp, 4, hp) == RL_E_INVALID and b"fetch" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_GLOBAL, None, 4, hp) == RL_E_INVALID and b"buffer" in _lib.lib.rl_last_error()
    assert fn(None, R.FETCH_GLOBAL, rp, 4, None) == RL_E_INVALID and b"buffer" in _lib.lib.rl_last_error()
    assert hits.tobytes() == bytes(hits.nbytes)   # nothing written
    launches = R.query_launches()
    assert len(launches) == QUERY_VARIANTS
    assert _lib.lib.rl_debug_query_launches(None) == RL_E_INVALID


@pytest.fixture(scope="module")
def query_kernels():
    """Metadata of every rl_query_kernel instantiation from the device-only -S compile with the library's own flags."""
    text, metadata, _ = device_build()
    return {n: k for n, k in metadata.items() if "rl_query_kernel" in n}, text



def test_every_query_kernel_variant_is_free_of_scratch_and_spills(query_kernels):
    kernels, text = query_kernels
    assert len(kernels) == QUERY_VARIANTS, sorted(kernels)
    for name, k in kernels.items():
        assert "rl_trace_kernel" not in name                         # tests/test_kernel_resources.py counts those by that substring
        assert k["private_segment_fixed_size"] == 0, (name, k)        # no scratch memory
        assert k["vgpr_spill_count"] == 0, (name, k)
        # (scalar registers may spill to lanes of a vector register -- not to memory -- where the scene's addresses are 64-bit
        # global ones, as in the trace kernel's variants of those stages: tests/test_kernel_resources.py)
        stage = int(re.search(r"rl_query_kernelILi([012])E", name).group(1))
        assert k["sgpr_spill_count"] == 0 if stage == 2 else k["sgpr_spill_count"] <= 32, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)   # four waves per SIMD, as the trace kernel
    stages = sorted(re.search(r"rl_query_kernelILi([012])ELb([01])E", n).groups() for n in kernels)
    assert stages == [(s, c) for s in "012" for c in "01"]
