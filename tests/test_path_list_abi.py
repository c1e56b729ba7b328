"""rl_scene_step_path_list* at the boundary, without a GPU: the entry points (exported, bound, in the Rust block), their argument
checks in the documented order with nothing written, n_list == 0, the compiled kernels' resources (hipcc cross-compiles here), and
the numpy restatement of the listed step (tests/_path_list_oracle.py) run as the wavefront loop against the restatement of the
whole path (tests/_path_oracle.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from _boundary import _err, _FakeScene
from _device_build import kernels, variant_of_name  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robigo_luculenta_amd", "csrc")
RL_E_INVALID = -1
ENTRY_POINTS = ("rl_scene_step_path_list", "rl_scene_step_path_list_device")
# the substrings the resource tests of the other kernels count them by
TAKEN = ("rl_step_kernel", "rl_query_kernel", "rl_ray_paths_kernel", "rl_film_", "rl_trace_kernel", "rl_occlusion_kernel", "rl_begin_paths_kernel",
         "rl_camera_rays_kernel", "rl_plot_kernel", "rl_gather_kernel", "rl_add_kernel", "rl_tonemap_kernel")
# kernels of each existing family in the device build: the counts the parent commit has
FAMILIES = {"rl_step_kernel": 6, "rl_query_kernel": 6, "rl_ray_paths_kernel": 6, "rl_film_": 7, "rl_occlusion_kernel": 6,
            "rl_trace_kernel": 24, "rl_begin_paths_kernel": 1, "rl_camera_rays_kernel": 1}


def test_both_entry_points_are_exported_bound_and_in_the_rust_block():
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert header.index("int rl_scene_step_paths_device(") < header.index("int rl_scene_step_path_list(") < header.index("#define RL_MAX_PIXELS")
    assert hasattr(_lib.lib, "rl_debug_path_list_launches") and "rl_debug_path_list_launches" in _lib.DEBUG_SIGNATURES
    assert len(R.path_list_launches()) == 6
    assert _lib.lib.rl_debug_path_list_launches(None) == RL_E_INVALID
    for method in ("step_path_list", "step_path_list_device"):
        assert callable(getattr(R.Scene, method))


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_bad_arguments_are_invalid_with_a_message_in_the_documented_order(name):
    fn = getattr(_lib.lib, name)
    st, hits = np.zeros(4, R.PATH_STATE_DTYPE), np.zeros(4, R.HIT_DTYPE)
    st["end"] = R.RL_PATH_LIVE
    lst, live = np.arange(4, dtype=np.uint32), np.full(8, 0xAAAAAAAA, np.uint32)
    n_live = C.c_uint32(0xAAAAAAAA)
    before = st.tobytes()
    sp, hp, lp, vp, np_ = (st.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), lst.ctypes.data_as(C.c_void_p),
                           live.ctypes.data_as(C.c_void_p), C.byref(n_live))
    fake = _FakeScene().ptr
    LDS = R.FETCH_LDS
    assert fn(None, LDS, 1, 0, 0, sp, 4, lp, 4, hp, vp, np_) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, LDS, 1, 0, 0, None, 0, None, 0, None, None, np_) == RL_E_INVALID and b"scene" in _err()
    for scene in (None, fake):
        assert fn(scene, 7, 1, 0, 0, sp, 4, lp, 4, hp, vp, np_) == RL_E_INVALID and b"fetch" in _err()
        assert fn(scene, -1, 1, 0, 0, sp, 4, None, 4, None, None, None) == RL_E_INVALID and b"fetch" in _err()
        for flags in (2, 3, 0x80000000, 0xfffffffe):
            assert fn(scene, LDS, 1, 0, flags, sp, 4, lp, 4, hp, vp, np_) == RL_E_INVALID and b"flag" in _err()
        assert fn(scene, R.FETCH_GLOBAL, 1, 0, 0, None, 4, lp, 4, hp, vp, np_) == RL_E_INVALID and b"state buffer" in _err()
        assert fn(scene, R.FETCH_GLOBAL, 1, 0, R.RL_STEP_NO_ROULETTE, None, 0, lp, 1, None, None, None) == RL_E_INVALID and b"state buffer" in _err()
    # the identity list must fit the states; a given list may be longer than they are
    assert fn(fake, LDS, 1, 0, 0, sp, 4, None, 5, hp, vp, np_) == RL_E_INVALID and b"identity list" in _err()
    assert fn(fake, LDS, 1, 0, 0, sp, 0, None, 1, None, None, np_) == RL_E_INVALID and b"identity list" in _err()
    # the documented order: fetch, flags, states, scene, identity list
    assert fn(None, 7, 1, 0, 2, None, 4, None, 5, None, None, np_) == RL_E_INVALID and b"fetch" in _err()
    assert fn(None, LDS, 1, 0, 2, None, 4, None, 5, None, None, np_) == RL_E_INVALID and b"flag" in _err()
    assert fn(None, LDS, 1, 0, 0, None, 4, None, 5, None, None, np_) == RL_E_INVALID and b"state buffer" in _err()
    assert fn(None, LDS, 1, 0, 0, sp, 4, None, 5, None, None, np_) == RL_E_INVALID and b"scene" in _err()
    assert fn(fake, LDS, 1, 0, 0, sp, 4, None, 5, None, None, np_) == RL_E_INVALID and b"identity list" in _err()
    # nothing written by any of them
    assert st.tobytes() == before and hits.tobytes() == bytes(hits.nbytes) and (live == 0xAAAAAAAA).all() and (lst == np.arange(4)).all()
    assert n_live.value == 0xAAAAAAAA


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_an_empty_list_does_nothing_but_report_zero(name):
    fn = getattr(_lib.lib, name)
    st = np.zeros(4, R.PATH_STATE_DTYPE)
    st["end"] = R.RL_PATH_LIVE
    before = st.tobytes()
    live = np.full(4, 0xAAAAAAAA, np.uint32)
    sp, vp = st.ctypes.data_as(C.c_void_p), live.ctypes.data_as(C.c_void_p)
    fake = _FakeScene().ptr
    for flags in (0, R.RL_STEP_NO_ROULETTE):
        for states, n_states in ((sp, 4), (None, 0), (sp, 0)):
            for lst in (None, vp):
                n_live = C.c_uint32(0xAAAAAAAA)
                assert fn(fake, R.FETCH_LDS, 1, 0, flags, states, n_states, lst, 0, None, vp, C.byref(n_live)) == 0
                assert n_live.value == 0
                assert fn(fake, R.FETCH_GLOBAL, 1, 0, flags, states, n_states, lst, 0, None, None, None) == 0
    assert st.tobytes() == before and (live == 0xAAAAAAAA).all()


def test_list_kernels_resources_names_and_the_existing_families(kernels):
    lists = {n: k for n, k in kernels.items() if "rl_list_step_kernel" in n}
    pack = {n: k for n, k in kernels.items() if "rl_list_scan_kernel" in n or "rl_list_pack_kernel" in n}
    steps = {n: k for n, k in kernels.items() if "rl_step_kernel" in n}
    assert len(lists) == 6 and len(pack) == 2 and len(steps) == 6, sorted(kernels)
    assert sorted(variant_of_name(n, "rl_list_step_kernel") for n in lists) == [(s, c) for s in "012" for c in "01"]
    new = {n: k for n, k in kernels.items() if "rl_list_" in n}
    assert len(new) == 8
    for name, k in new.items():
        for taken in TAKEN:
            assert taken not in name, (name, taken)
        assert k["private_segment_fixed_size"] == 0, (name, k)          # no scratch memory
        assert k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)
    step_spills = {variant_of_name(n, "rl_step_kernel"): k["sgpr_spill_count"] for n, k in steps.items()}
    for name, k in lists.items():
        v = variant_of_name(name, "rl_list_step_kernel")
        assert k["sgpr_spill_count"] <= step_spills[v], (name, k["sgpr_spill_count"], step_spills[v])
        if v[0] == "2":                                                   # the whole scene staged
            assert k["sgpr_spill_count"] == 0, (name, k)
    for name, k in pack.items():
        assert k["sgpr_spill_count"] == 0, (name, k)
    # the existing families are counted as before: the new names match none of their substrings
    for sub, count in FAMILIES.items():
        assert sum(1 for n in kernels if sub in n) == count, (sub, sorted(n for n in kernels if sub in n))


def test_the_new_header_is_part_of_the_build_and_of_the_build_id():
    make = open(os.path.join(CSRC, "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    assert "rl_path_list.hip.h" in hdrs and os.path.exists(os.path.join(CSRC, "rl_path_list.hip.h"))
    api = open(os.path.join(CSRC, "rl_api.hip")).read()
    assert api.index('#include "rl_step.hip.h"') < api.index('#include "rl_path_list.hip.h"')
    text = open(os.path.join(CSRC, "rl_path_list.hip.h")).read()
    m = re.search(r"void rl_list_step_kernel\(", text)
    assert m and "rl_stage_scene<STAGE>(scene, lay)" in text[m.end():m.end() + 1500]


def test_path_list_oracle_looped_reproduces_the_path_oracle():
    """tests/_path_list_oracle.py from the identity list, its survivors fed back until none is left, against PathOracle on the
    scenes and rays of test_step_abi.py's test_step_oracle_iterated_reproduces_the_path_oracle: {value, segments, object, end}
    bit for bit, and as many steps as the longest path has segments (that test shows it is below RL_PATH_MAX_SEGMENTS)."""
    import _mirror as M
    import _path_list_oracle as L
    import _path_oracle as P
    import _step_oracle as S
    for which, param in ((0, 0), (1, 0)):
        objs, cam = M.builtin_desc(which, param)
        W, H, seed, stream, first, n = 320, 180, 11, 2, 1000, 300
        ms = M.Scene(objs, cam)
        dump = M.lib().mirror_dump_rays
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
        so = S.StepOracle(objs, cam)
        got, steps = L.run(so, rays, seed, stream, first, max_steps=R.RL_PATH_MAX_SEGMENTS)
        assert (got["end"] != S.LIVE).all()
        for f in ("value", "segments", "object", "end"):
            assert got[f].tobytes() == want[f].tobytes(), (which, f)
        assert steps == int(want["segments"].max()) < R.RL_PATH_MAX_SEGMENTS, (which, steps)
        # the restatement's own edges: skipped entries, ended and unlisted states, a stable order
        st = S.begin(rays, first)
        lst = np.array([5, n, 0xffffffff, 3, 37, 4, n + 7, 1], np.uint32)      # 37: not live (its wavelength is not finite)
        ref = st.copy()
        live = L.step_list(so, st, seed, stream, list=lst)
        named = [5, 3, 4, 1]
        sub = ref[named]
        so.step(sub, seed, stream)
        ref[named] = sub
        assert st.tobytes() == ref.tobytes()
        assert live.tolist() == [i for i in named if st["end"][i] == S.LIVE] and live.dtype == np.uint32
