"""rl_plot_unit_plot_photons* / rl_plot_unit_render_samples* at the boundary, without a GPU: the entry points and their
argument checks (in the order include/robigo_luculenta.h gives, every one before a handle is read or a device is touched), the Rust
declarations, and the compiled film kernels' resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from _boundary import _err, _Fake
from _device_build import device_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robigo_luculenta_amd", "csrc")
RL_E_INVALID = -1
FILM_VARIANTS = 6   # (nothing / the tables / the whole scene staged in LDS) x prisms with / without a second bound
ENTRY_POINTS = ("rl_plot_unit_plot_photons", "rl_plot_unit_plot_photons_device", "rl_plot_unit_render_samples",
                "rl_plot_unit_render_samples_device")
# the kernel-count tests of the other kernels pick them out of the module by these substrings
TAKEN = ("rl_trace_kernel", "rl_query_kernel", "rl_ray_paths_kernel", "rl_camera_rays_kernel", "rl_plot_kernel", "rl_gather_kernel",
         "rl_add_kernel", "rl_tonemap_kernel")


def test_every_entry_point_is_exported_bound_and_declared_for_rust():
    ffi = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header)
        assert re.search(r"pub fn %s\(" % name, ffi)
    assert hasattr(_lib.lib, "rl_debug_film_launches") and "rl_debug_film_launches" in _lib.DEBUG_SIGNATURES
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert debug.index("rl_debug_path_launches(") < debug.index("rl_debug_film_launches(")
    assert "rl_debug_film_launches" not in ffi   # diagnostics are not part of the Rust binding
    assert len(R.film_launches()) == FILM_VARIANTS and len(R.path_launches()) == 6
    assert _lib.lib.rl_debug_film_launches(None) == RL_E_INVALID
    for method in ("plot_photons", "plot_photons_device", "render_samples", "render_samples_device"):
        assert callable(getattr(R.PlotUnit, method))


@pytest.mark.parametrize("name", ["rl_plot_unit_plot_photons", "rl_plot_unit_plot_photons_device"])
def test_plot_photons_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    photons = np.zeros(4, R.PHOTON_DTYPE)
    pp = photons.ctypes.data_as(C.c_void_p)
    unit = _Fake()
    assert fn(None, pp, 4) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(None, None, 0) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(unit.ptr, None, 4) == RL_E_INVALID and b"photon" in _err()
    assert fn(unit.ptr, None, 1 << 40) == RL_E_INVALID and b"photon" in _err()
    assert fn(unit.ptr, pp, 0) == 0 and fn(unit.ptr, None, 0) == 0   # n = 0 does nothing
    assert bytes(unit.buf) == bytes(256) and photons.tobytes() == bytes(photons.nbytes)


@pytest.mark.parametrize("name", ["rl_plot_unit_render_samples", "rl_plot_unit_render_samples_device"])
def test_render_samples_bad_arguments_are_invalid_in_the_documented_order(name):
    fn = getattr(_lib.lib, name)
    samples, res = np.zeros(4, R.CAMERA_SAMPLE_DTYPE), np.zeros(4, R.PATH_RESULT_DTYPE)
    sp, op = samples.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    unit, scene = _Fake(), _Fake()
    u, s = unit.ptr, scene.ptr
    # each check with every later one failing too: the earlier one is the one reported
    assert fn(None, None, 7, 1, 0, (1 << 64) - 2, 65537, None, 4, op) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(None, s, R.FETCH_LDS, 1, 0, 0, 0, sp, 4, op) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(None, s, R.FETCH_LDS, 1, 0, 0, 0, None, 0, None) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(u, None, 7, 1, 0, (1 << 64) - 2, 65537, None, 4, op) == RL_E_INVALID and b"scene" in _err()
    assert fn(u, None, R.FETCH_LDS, 1, 0, 0, 0, None, 0, None) == RL_E_INVALID and b"scene" in _err()
    assert fn(u, s, 7, 1, 0, (1 << 64) - 2, 65537, None, 4, op) == RL_E_INVALID and b"fetch" in _err()
    assert fn(u, s, -1, 1, 0, 0, 0, sp, 4, op) == RL_E_INVALID and b"fetch" in _err()
    assert fn(u, s, R.FETCH_GLOBAL, 1, 0, (1 << 64) - 2, 65537, None, 4, op) == RL_E_INVALID and b"max_segments" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, 0, 0xffffffff, sp, 4, op) == RL_E_INVALID and b"max_segments" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, 0, 65537, None, 0, None) == RL_E_INVALID and b"max_segments" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, (1 << 64) - 4, 65536, None, 4, op) == RL_E_INVALID and b"2^64" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, (1 << 64) - 5, 0, sp, 4, op) == RL_E_INVALID and b"2^64" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, (1 << 64) - 1, 0, None, 0, None) == RL_E_INVALID and b"2^64" in _err()
    assert fn(u, s, R.FETCH_LDS, 1, 0, 0, 0, None, 4, op) == RL_E_INVALID and b"sample" in _err()
    assert fn(u, s, R.FETCH_GLOBAL, 1, 0, 0, 1, None, 4, None) == RL_E_INVALID and b"sample" in _err()
    for ms in (0, 1, 65536):
        assert fn(u, s, R.FETCH_LDS, 1, 0, 0, ms, None, 0, None) == 0   # n = 0 does nothing
        assert fn(u, s, R.FETCH_GLOBAL, 1, 0, (1 << 64) - 2, ms, sp, 0, op) == 0
    assert res.tobytes() == bytes(res.nbytes) and samples.tobytes() == bytes(samples.nbytes)
    assert bytes(unit.buf) == bytes(256) and bytes(scene.buf) == bytes(256)


@pytest.fixture(scope="module")
def film_kernels():
    """Metadata of every kernel of the module from the device-only -S compile with the library's own flags."""
    return device_build()[1]



def test_film_kernels_are_free_of_scratch_and_spills(film_kernels):
    paths = {n: k for n, k in film_kernels.items() if "rl_film_paths_kernel" in n}
    photons = {n: k for n, k in film_kernels.items() if "rl_film_photons_kernel" in n}
    assert len(paths) == FILM_VARIANTS and len(photons) == 1, sorted(film_kernels)
    for name, k in list(paths.items()) + list(photons.items()):
        for taken in TAKEN:
            assert taken not in name
        assert k["private_segment_fixed_size"] == 0, (name, k)   # no scratch memory
        assert k["vgpr_spill_count"] == 0, (name, k)
    for name, k in paths.items():   # the path kernel's own bounds (tests/test_path_query_abi.py)
        stage = int(re.search(r"rl_film_paths_kernelILi([012])E", name).group(1))
        assert k["sgpr_spill_count"] == 0 if stage == 2 else k["sgpr_spill_count"] <= 32, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)   # four waves per SIMD
    stages = sorted(re.search(r"rl_film_paths_kernelILi([012])ELb([01])E", n).groups() for n in paths)
    assert stages == [(s, c) for s in "012" for c in "01"]
    k = photons[next(iter(photons))]
    assert k["vgpr_count"] <= 32 and k["sgpr_spill_count"] == 0, k   # fits beside a resident trace kernel, as the other small kernels


def test_the_other_kernels_keep_their_counts(film_kernels):
    """The new kernels' names contain none of the substrings the existing resource tests count by."""
    count = lambda sub: sum(1 for n in film_kernels if sub in n)
    assert count("rl_ray_paths_kernel") == 6 and count("rl_camera_rays_kernel") == 1 and count("rl_trace_kernel") == 24
    for sub in ("rl_plot_kernel", "rl_gather_kernel", "rl_add_kernel", "rl_tonemap_kernel"):
        assert count(sub) == 1, sub


def test_film_header_is_part_of_the_build_id():
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HDRS = .*\brl_film\.hip\.h\b", make, re.M)
