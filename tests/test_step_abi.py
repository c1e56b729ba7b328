"""rl_scene_begin_paths* / rl_scene_step_paths* at the boundary, without a GPU: the frozen layout of RlPathState (header, ctypes
mirror, numpy dtype, Rust block), the entry points and their argument checks in the documented order, the compiled kernels'
resources (hipcc cross-compiles here), and the Python restatement of one loop turn (tests/_step_oracle.py) iterated against the
restatement of the whole loop (tests/_path_oracle.py), which test_path_query_abi.py holds against the oracle's own render."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from _boundary import _err, _FakeScene
from _device_build import device_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robigo_luculenta_amd", "csrc")
RL_E_INVALID = -1
STEP_VARIANTS = 6   # (nothing / the tables / the whole scene staged in LDS) x prisms with / without a second bound
ENTRY_POINTS = ("rl_scene_begin_paths", "rl_scene_begin_paths_device", "rl_scene_step_paths", "rl_scene_step_paths_device")
LAYOUT = [("origin", 0), ("wavelength", 12), ("direction", 16), ("intensity", 28), ("continue_chance", 32), ("segments", 36), ("end", 40),
          ("value", 44), ("path_index", 48), ("object", 56), ("reserved", 60)]


def test_path_state_has_its_frozen_layout():
    assert C.sizeof(_lib.RlPathState) == 64 and R.PATH_STATE_DTYPE.itemsize == 64
    assert [(f, getattr(_lib.RlPathState, f).offset) for f, _ in _lib.RlPathState._fields_] == LAYOUT
    assert [(n, R.PATH_STATE_DTYPE.fields[n][1]) for n in R.PATH_STATE_DTYPE.names] == LAYOUT
    assert R.PATH_STATE_DTYPE.fields["path_index"][0] == np.dtype("<u8") and _lib.RlPathState.path_index.size == 8
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    assert re.search(r"#define RL_PATH_LIVE 0xffffffffu\b", header) and R.RL_PATH_LIVE == 0xffffffff
    assert re.search(r"#define RL_STEP_NO_ROULETTE 1u\b", header) and R.RL_STEP_NO_ROULETTE == 1
    import _step_oracle as S
    assert S.STATE_DTYPE == R.PATH_STATE_DTYPE and S.HIT_DTYPE == R.HIT_DTYPE and S.LIVE == R.RL_PATH_LIVE


def test_every_entry_point_is_exported_bound_and_in_the_rust_block():
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    for name in ENTRY_POINTS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert re.search(r"pub struct RlPathState\b", rust)
    assert re.search(r"pub const RL_PATH_LIVE: u32 = 0xffff_ffff;", rust) and re.search(r"pub const RL_STEP_NO_ROULETTE: u32 = 1;", rust)
    assert hasattr(_lib.lib, "rl_debug_step_launches") and "rl_debug_step_launches" in _lib.DEBUG_SIGNATURES
    assert len(R.step_launches()) == STEP_VARIANTS
    assert _lib.lib.rl_debug_step_launches(None) == RL_E_INVALID
    for method in ("begin_paths", "begin_paths_device", "step_paths", "step_paths_device"):
        assert callable(getattr(R.Scene, method))


@pytest.mark.parametrize("name", ["rl_scene_step_paths", "rl_scene_step_paths_device"])
def test_step_paths_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    st, hits = np.zeros(4, R.PATH_STATE_DTYPE), np.zeros(4, R.HIT_DTYPE)
    st["end"] = R.RL_PATH_LIVE
    before = st.tobytes()
    sp, hp = st.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
    fake = _FakeScene().ptr
    assert fn(None, R.FETCH_LDS, 1, 0, 0, sp, 4, hp) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, R.FETCH_LDS, 1, 0, 0, None, 0, None) == RL_E_INVALID and b"scene" in _err()
    for scene in (None, fake):
        assert fn(scene, 7, 1, 0, 0, sp, 4, hp) == RL_E_INVALID and b"fetch" in _err()
        assert fn(scene, -1, 1, 0, 0, sp, 4, None) == RL_E_INVALID and b"fetch" in _err()
        for flags in (2, 3, 0x80000000, 0xfffffffe):
            assert fn(scene, R.FETCH_LDS, 1, 0, flags, sp, 4, hp) == RL_E_INVALID and b"flag" in _err()
        assert fn(scene, R.FETCH_GLOBAL, 1, 0, 0, None, 4, hp) == RL_E_INVALID and b"state buffer" in _err()
        assert fn(scene, R.FETCH_GLOBAL, 1, 0, R.RL_STEP_NO_ROULETTE, None, 4, None) == RL_E_INVALID and b"state buffer" in _err()
    # the documented order: fetch, flags, buffers, scene
    assert fn(None, 7, 1, 0, 2, None, 4, None) == RL_E_INVALID and b"fetch" in _err()
    assert fn(None, R.FETCH_LDS, 1, 0, 2, None, 4, None) == RL_E_INVALID and b"flag" in _err()
    assert fn(None, R.FETCH_LDS, 1, 0, 0, None, 4, None) == RL_E_INVALID and b"state buffer" in _err()
    for flags in (0, R.RL_STEP_NO_ROULETTE):
        assert fn(fake, R.FETCH_LDS, 1, 0, flags, None, 0, None) == 0   # n = 0 does nothing
    assert st.tobytes() == before and hits.tobytes() == bytes(hits.nbytes)   # nothing written


@pytest.mark.parametrize("name", ["rl_scene_begin_paths", "rl_scene_begin_paths_device"])
def test_begin_paths_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    rays, st = np.zeros(4, R.SPECTRAL_RAY_DTYPE), np.zeros(4, R.PATH_STATE_DTYPE)
    rp, sp = rays.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p)
    fake = _FakeScene().ptr
    assert fn(None, 0, rp, 4, sp) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, 0, None, 0, None) == RL_E_INVALID and b"scene" in _err()
    for scene in (None, fake):
        assert fn(scene, 0, None, 4, sp) == RL_E_INVALID and b"buffer" in _err()
        assert fn(scene, 0, rp, 4, None) == RL_E_INVALID and b"state buffer" in _err()
    assert fn(fake, (1 << 64) - 4, rp, 4, sp) == RL_E_INVALID and b"2^64" in _err()
    assert fn(fake, (1 << 64) - 5, rp, 4, sp) == RL_E_INVALID and b"2^64" in _err()
    assert fn(fake, (1 << 64) - 1, None, 0, None) == RL_E_INVALID and b"2^64" in _err()
    assert fn(fake, 0, None, 0, None) == 0   # n = 0 does nothing
    assert st.tobytes() == bytes(st.nbytes)


@pytest.fixture(scope="module")
def step_kernels():
    """Metadata of the step and begin kernels from the device-only -S compile with the library's own flags."""
    metadata = device_build()[1]
    return {n: k for n, k in metadata.items() if any(sub in n for sub in ("rl_step_kernel", "rl_begin_paths_kernel", "rl_ray_paths_kernel"))}



def test_step_and_begin_kernels_are_free_of_scratch_and_spills(step_kernels):
    step = {n: k for n, k in step_kernels.items() if "rl_step_kernel" in n}
    begin = {n: k for n, k in step_kernels.items() if "rl_begin_paths_kernel" in n}
    paths = {n: k for n, k in step_kernels.items() if "rl_ray_paths_kernel" in n}
    assert len(step) == STEP_VARIANTS and len(begin) == 1 and len(paths) == 6, sorted(step_kernels)
    for name, k in list(step.items()) + list(begin.items()):
        for taken in ("rl_trace_kernel", "rl_query_kernel", "rl_ray_paths_kernel", "rl_camera_rays_kernel", "rl_film", "rl_plot_kernel",
                      "rl_gather_kernel", "rl_add_kernel", "rl_tonemap_kernel"):
            assert taken not in name   # the resource tests of the other kernels pick them out by these substrings
        assert k["private_segment_fixed_size"] == 0, (name, k)   # no scratch memory
        assert k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
    variant = lambda n, kernel: re.search(kernel + r"ILi([012])ELb([01])E", n).groups()
    path_spills = {variant(n, "rl_ray_paths_kernel"): k["sgpr_spill_count"] for n, k in paths.items()}
    for name, k in step.items():
        v = variant(name, "rl_step_kernel")
        assert k["sgpr_spill_count"] <= path_spills[v], (name, k, path_spills[v])   # no higher than the path kernel's, per variant
        assert k["sgpr_spill_count"] == 0 if v[0] == "2" else k["sgpr_spill_count"] <= 32, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)   # four waves per SIMD, as the query kernel
    assert begin[next(iter(begin))]["sgpr_spill_count"] == 0
    assert sorted(variant(n, "rl_step_kernel") for n in step) == [(s, c) for s in "012" for c in "01"]


def test_step_oracle_iterated_reproduces_the_path_oracle():
    """tests/_step_oracle.py, begun and stepped until nothing is live, against PathOracle.render_ray on the camera rays of the
    built-in scene and the glass scene (the seeds and counts of test_path_query_abi.py): {value, segments, object, end} bit for bit.
    The longest path is asserted too: the GPU identity test steps at most RL_PATH_MAX_SEGMENTS times, which must leave out nothing."""
    import _mirror as M
    import _path_oracle as P
    import _step_oracle as S
    longest = {}
    for which, param in ((0, 0), (1, 0)):   # the demo scene and the glass stress scene
        objs, cam = M.builtin_desc(which, param)
        W, H, seed, stream, first, n = 320, 180, 11, 2, 1000, 300
        ms = M.Scene(objs, cam)
        dump = M.lib().mirror_dump_rays   # (the first ray of a path: rl_begin_path)
        dump.restype = C.c_uint64
        dump.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
        rays6 = np.zeros((n, 6), np.float32)
        for i in range(n):
            assert dump(ms.h, W, H, seed, stream, first + i, 1, rays6[i].ctypes.data, 1) == 1
        rays = np.zeros(n, R.SPECTRAL_RAY_DTYPE)
        rays["origin"], rays["direction"] = rays6[:, :3], rays6[:, 3:]
        rays["wavelength"] = np.random.default_rng(which).uniform(380.0, 780.0, n).astype(np.float32)
        rays["wavelength"][::37] = [np.nan, np.inf, -np.inf][which]
        want = P.PathOracle(objs, cam).render_rays(rays["origin"], rays["direction"], rays["wavelength"], seed, stream, first)
        got, steps = S.StepOracle(objs, cam).run(rays, seed, stream, first, max_steps=R.RL_PATH_MAX_SEGMENTS)
        assert (got["end"] != S.LIVE).all()
        for f in ("value", "segments", "object", "end"):
            assert got[f].tobytes() == want[f].tobytes(), (which, f)
        assert (got["path_index"] == first + np.arange(n)).all() and (got["reserved"] == 0).all()
        assert (want["end"] != P.LIMIT).all() and (want["end"] == P.INVALID).sum() == len(rays[::37])
        assert (want["value"] != 0).any()
        assert steps == int(want["segments"].max())
        longest[which] = steps
    assert 1 < max(longest.values()) < R.RL_PATH_MAX_SEGMENTS, longest
