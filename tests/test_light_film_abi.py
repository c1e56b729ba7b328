"""rl_plot_unit_light_paths* and rl_plot_unit_render_samples_direct* at the boundary, without a GPU: the entry points and their
argument checks in the documented order, the numpy statement of the drop rule and the byte protocol (tests/_light_film_oracle.py)
on cases worked by hand, and the compiled kernels' resources (hipcc cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
import _light_film_oracle as FO
from _boundary import _err
from _device_build import device_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
LIGHT = ("rl_plot_unit_light_paths", "rl_plot_unit_light_paths_device")
DIRECT = ("rl_plot_unit_render_samples_direct", "rl_plot_unit_render_samples_direct_device")
# rl_light_kernel's spilled SGPRs per variant (stage, cylinders), DESIGN.md section 4: the new kernel may not spill more
LIGHT_KERNEL_SGPR_SPILLS = {("0", "0"): 22, ("0", "1"): 23, ("1", "0"): 14, ("1", "1"): 15, ("2", "0"): 0, ("2", "1"): 0}


class _Fake:
    """A handle for the checks that come before the handle is read or a device is touched (device 0 if it is read)."""

    def __init__(self):
        self.buf = (C.c_uint8 * 512)()
        self.ptr = C.cast(self.buf, C.c_void_p)


def test_every_new_symbol_is_exported_and_bound():
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    for name in LIGHT + DIRECT:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
    assert hasattr(_lib.lib, "rl_debug_light_film_launches") and "rl_debug_light_film_launches" in _lib.DEBUG_SIGNATURES
    assert "rl_debug_light_film_launches" in open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert len(R.light_film_launches()) == 6 and _lib.lib.rl_debug_light_film_launches(None) == RL_E_INVALID
    for name in ("light_paths", "light_paths_device", "render_samples_direct", "render_samples_direct_device"):
        assert callable(getattr(R.PlotUnit, name)), name


@pytest.mark.parametrize("name", LIGHT)
def test_light_paths_arguments_are_checked_in_the_documented_order_with_no_device(name):
    fn = getattr(_lib.lib, name)
    st, hits, cam = np.zeros(4, R.PATH_STATE_DTYPE), np.zeros(4, R.HIT_DTYPE), np.zeros(4, R.CAMERA_SAMPLE_DTYPE)
    sm, by, lst = np.full(4 * 8, 0xAAAAAAAA, np.uint32), np.full(4, 0xAA, np.uint8), np.arange(4, dtype=np.uint32)
    sp, hp, cp, mp, bp, lp = (a.ctypes.data_as(C.c_void_p) for a in (st, hits, cam, sm, by, lst))
    unit, scene = _Fake().ptr, _Fake().ptr
    LDS = R.FETCH_LDS
    good = (sp, 4, lp, 4, hp, cp, bp, mp)
    # 1. unit, 2. scene, 3. fetch, 4. buffers, 5. identity list: each with everything behind it wrong as well
    assert fn(None, None, 7, 1, 0, None, 4, None, 5, None, None, None, None) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(None, scene, LDS, 1, 0, *good) == RL_E_INVALID and b"plot unit" in _err()
    assert fn(unit, None, 7, 1, 0, None, 4, None, 5, None, None, None, None) == RL_E_INVALID and b"scene" in _err()
    assert fn(unit, None, LDS, 1, 0, *good) == RL_E_INVALID and b"scene" in _err()
    assert fn(unit, scene, 7, 1, 0, None, 4, None, 5, None, None, None, None) == RL_E_INVALID and b"fetch" in _err()
    assert fn(unit, scene, -1, 1, 0, *good) == RL_E_INVALID and b"fetch" in _err()
    for args in ((None, 4, lp, 4, hp, cp, bp, mp), (sp, 4, lp, 4, None, cp, bp, mp), (sp, 4, lp, 4, hp, None, bp, mp), (None, 4, None, 5, None, None, None, None)):
        assert fn(unit, scene, LDS, 1, 0, *args) == RL_E_INVALID and b"buffer" in _err(), args
    assert fn(unit, scene, LDS, 1, 0, sp, 4, None, 5, hp, cp, bp, mp) == RL_E_INVALID and b"identity list" in _err()
    # samples and sampled may be NULL; an empty list does nothing, whatever else is given
    for args in ((sp, 4, lp, 0, hp, cp, bp, mp), (None, 0, None, 0, None, None, None, None), (sp, 4, None, 0, hp, cp, None, None)):
        for fetch in (LDS, R.FETCH_GLOBAL):
            assert fn(unit, scene, fetch, 1, 0, *args) == 0, args
    assert (sm == 0xAAAAAAAA).all() and (by == 0xAA).all() and st.tobytes() == bytes(st.nbytes) and (lst == np.arange(4)).all()


@pytest.mark.parametrize("name", DIRECT)
def test_render_samples_direct_arguments_are_render_samples(name):
    fn, ref = getattr(_lib.lib, name), getattr(_lib.lib, name.replace("_direct", ""))
    cam, res = np.zeros(4, R.CAMERA_SAMPLE_DTYPE), np.full(4 * 4, 0xAAAAAAAA, np.uint32)
    cp, rp = cam.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    unit, scene = _Fake().ptr, _Fake().ptr
    cases = [((None, None, 7, 1, 0, 0, 70000, None, 4, None), b"plot unit"), ((unit, None, 7, 1, 0, 0, 70000, None, 4, None), b"scene"),
             ((unit, scene, 7, 1, 0, 0, 70000, None, 4, None), b"fetch"), ((unit, scene, 0, 1, 0, 0, 70000, None, 4, None), b"max_segments"),
             ((unit, scene, 0, 1, 0, 2 ** 64 - 2, 5, None, 4, None), b"path ind"), ((unit, scene, 0, 1, 0, 0, 5, None, 4, rp), b"sample buffer")]
    for args, word in cases:
        assert ref(*args) == RL_E_INVALID
        told = _err()
        assert fn(*args) == RL_E_INVALID and _err() == told and word in told.lower().replace(b"indices", b"ind"), (args, told)
    assert fn(unit, scene, 0, 1, 0, 0, 5, cp, 0, rp) == 0 and fn(unit, scene, 1, 1, 0, 0, 0, None, 0, None) == 0
    assert (res == 0xAAAAAAAA).all()


def _case():
    """Six states worked by hand: emitters are objects 1 and 2; object 5 is an emitter that is never sampled (a plane)."""
    st = np.zeros(6, R.PATH_STATE_DTYPE)
    st["wavelength"] = [500, 510, 520, 530, 540, 550]
    st["end"] = [R.RL_PATH_LIVE, R.RL_PATH_END_EMITTER, R.RL_PATH_END_EMITTER, R.RL_PATH_END_EMITTER, R.RL_PATH_END_ROULETTE, R.RL_PATH_END_EMITTER]
    st["value"] = [0, 2.0, 3.0, 4.0, 0, 0.0]
    st["object"] = [R.RL_OBJECT_NONE, 1, 5, 2, R.RL_OBJECT_NONE, 1]
    sm = np.zeros(6, R.LIGHT_SAMPLE_DTYPE)
    sm["status"] = [R.RL_LIGHT_VISIBLE, 0, 0, 0, R.RL_LIGHT_OCCLUDED, 0]
    sm["value"] = [0.5, 0, 0, 0, 0, 0]
    cam = np.zeros(6, R.CAMERA_SAMPLE_DTYPE)
    cam["x"], cam["y"] = np.arange(6) * 0.1, -np.arange(6) * 0.1
    return st, sm, cam, np.array([1, 2], np.uint32)


def test_the_oracle_states_the_drop_rule_and_the_byte_protocol():
    st, sm, cam, em = _case()
    before = np.array([7, 1, 1, 0, 0, 1], np.uint8)
    # state 0: a visible sample.  1: ended on emitter 1 after a sampled vertex: dropped.  2: on a plane emitter: kept.  3: on emitter 2 after
    # a vertex that was not sampled (a mirror, the camera): kept.  4: a blocked sample: nothing.  5: an ending without a value: nothing.
    ph, after = FO.film_photons(st, sm, em, cam, before)
    assert ph["probability"].tolist() == [0.5, 3.0, 4.0] and ph["wavelength"].tolist() == [500, 520, 530]
    assert np.allclose(ph["x"], [0, 0.2, 0.3]) and np.allclose(ph["y"], [0, -0.2, -0.3])
    assert after.tolist() == [1, 0, 0, 0, 1, 0] and before.tolist() == [7, 1, 1, 0, 0, 1]    # pure: the input is not written
    # sampled = None: nothing is dropped, nothing is recorded
    ph, after = FO.film_photons(st, sm, em, cam, None)
    assert ph["probability"].tolist() == [0.5, 2.0, 3.0, 4.0] and after is None
    # a list: states that are not listed add nothing and keep their byte; entries past the end and duplicates are skipped
    ph, after = FO.film_photons(st, sm, em, cam, before, list=[3, 9, 0, 3, 0xffffffff])
    assert ph["probability"].tolist() == [0.5, 4.0] and after.tolist() == [1, 1, 1, 0, 0, 1]
    ph, after = FO.film_photons(st, sm, em, cam, before, n_list=2)
    assert ph["probability"].tolist() == [0.5] and after.tolist() == [1, 0, 1, 0, 0, 1]
    # a position that is not finite is left out, the byte is still written
    cam["x"][0], cam["y"][2] = np.nan, np.inf
    ph, after = FO.film_photons(st, sm, em, cam, before)
    assert ph["probability"].tolist() == [4.0] and after.tolist() == [1, 0, 0, 0, 1, 0]
    # drop=False: the estimator that counts twice
    value, _ = FO.kept_values(st, sm, em, before, drop=False)
    assert value.tolist() == [0.5, 2.0, 3.0, 4.0, 0, 0]


@pytest.fixture(scope="module")
def kernels():
    return device_build()[1]


def test_light_film_kernels_compile_without_scratch_and_within_the_light_kernels_registers(kernels):
    pattern = r"rl_light_film_kernelILi([012])ELb([01])E"
    film = {re.search(pattern, n).groups(): k for n, k in kernels.items() if "rl_light_film_kernel" in n}
    assert sorted(film) == [(s, c) for s in "012" for c in "01"]
    for v, k in film.items():
        print("rl_light_film_kernel<%s, %s>: %d VGPRs, %d SGPRs spilled" % (v[0], v[1], k["vgpr_count"], k["sgpr_spill_count"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (v, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (v, k)
        assert k["sgpr_spill_count"] <= LIGHT_KERNEL_SGPR_SPILLS[v], (v, k["sgpr_spill_count"])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "now 22 / 23, 14 / 15 and 0" in design     # where the bound above is taken from
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_light_film.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
