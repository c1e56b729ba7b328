"""rl_scene_camera_rays* / rl_scene_render_rays* at the boundary, without a GPU: the frozen layouts of RlSpectralRay /
RlCameraSample / RlPathResult (header, ctypes mirror, numpy dtypes), the entry points and their argument checks, the compiled
kernels' resources (hipcc cross-compiles here), and the Python restatement of render_ray (tests/_path_oracle.py) against the
oracle's own render on camera rays of the host build of the kernel's per-path header."""
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
PATH_VARIANTS = 6   # (nothing / the tables / the whole scene staged in LDS) x prisms with / without a second bound
ENTRY_POINTS = ("rl_scene_camera_rays", "rl_scene_camera_rays_device", "rl_scene_render_rays", "rl_scene_render_rays_device")


def _offsets(struct):
    return [(f, getattr(struct, f).offset) for f, _ in struct._fields_]


def _dtype_offsets(dt):
    return [(n, dt.fields[n][1]) for n in dt.names]


def test_path_records_have_their_frozen_layouts():
    assert C.sizeof(_lib.RlSpectralRay) == 32 and C.sizeof(_lib.RlCameraSample) == 48 and C.sizeof(_lib.RlPathResult) == 16
    assert _offsets(_lib.RlSpectralRay) == [("origin", 0), ("wavelength", 12), ("direction", 16), ("reserved", 28)]
    assert _offsets(_lib.RlCameraSample) == [("ray", 0), ("x", 32), ("y", 36), ("reserved0", 40), ("reserved1", 44)]
    assert _offsets(_lib.RlPathResult) == [("value", 0), ("segments", 4), ("object", 8), ("end", 12)]
    assert R.SPECTRAL_RAY_DTYPE.itemsize == 32 and R.CAMERA_SAMPLE_DTYPE.itemsize == 48 and R.PATH_RESULT_DTYPE.itemsize == 16
    assert _dtype_offsets(R.SPECTRAL_RAY_DTYPE) == _offsets(_lib.RlSpectralRay)
    assert _dtype_offsets(R.CAMERA_SAMPLE_DTYPE) == _offsets(_lib.RlCameraSample)
    assert _dtype_offsets(R.PATH_RESULT_DTYPE) == _offsets(_lib.RlPathResult)
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    ends = dict((k, int(v)) for k, v in re.findall(r"(RL_PATH_END_[A-Z]+) = (\d)", header))
    assert ends == {"RL_PATH_END_VOID": R.RL_PATH_END_VOID, "RL_PATH_END_EMITTER": R.RL_PATH_END_EMITTER,
                    "RL_PATH_END_ROULETTE": R.RL_PATH_END_ROULETTE, "RL_PATH_END_LIMIT": R.RL_PATH_END_LIMIT,
                    "RL_PATH_END_INVALID": R.RL_PATH_END_INVALID}
    assert re.search(r"#define RL_PATH_MAX_SEGMENTS 4096\b", header) and R.RL_PATH_MAX_SEGMENTS == 4096
    assert re.search(r"#define RL_PATH_MAX_SEGMENTS_CAP 65536\b", header) and R.RL_PATH_MAX_SEGMENTS_CAP == 65536


def test_every_entry_point_is_exported_and_bound():
    for name in ENTRY_POINTS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.lib, "rl_debug_path_launches") and "rl_debug_path_launches" in _lib.DEBUG_SIGNATURES
    assert len(R.path_launches()) == PATH_VARIANTS
    assert _lib.lib.rl_debug_path_launches(None) == RL_E_INVALID


@pytest.mark.parametrize("name", ["rl_scene_render_rays", "rl_scene_render_rays_device"])
def test_render_rays_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    rays, res = np.zeros(4, R.SPECTRAL_RAY_DTYPE), np.zeros(4, R.PATH_RESULT_DTYPE)
    rp, op = rays.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    assert fn(None, R.FETCH_LDS, 1, 0, 0, 0, rp, 4, op) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, R.FETCH_LDS, 1, 0, 0, 0, None, 0, None) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, 7, 1, 0, 0, 0, rp, 4, op) == RL_E_INVALID and b"fetch" in _err()
    assert fn(None, -1, 1, 0, 0, 0, rp, 4, op) == RL_E_INVALID and b"fetch" in _err()
    assert fn(None, R.FETCH_GLOBAL, 1, 0, 0, 0, None, 4, op) == RL_E_INVALID and b"buffer" in _err()
    assert fn(None, R.FETCH_GLOBAL, 1, 0, 0, 0, rp, 4, None) == RL_E_INVALID and b"result buffer" in _err()
    assert res.tobytes() == bytes(res.nbytes)   # nothing written


@pytest.mark.parametrize("name", ["rl_scene_camera_rays", "rl_scene_camera_rays_device"])
def test_camera_rays_bad_arguments_are_invalid_with_a_message(name):
    fn = getattr(_lib.lib, name)
    s = np.zeros(4, R.CAMERA_SAMPLE_DTYPE)
    sp = s.ctypes.data_as(C.c_void_p)
    assert fn(None, 64, 36, 1, 0, 0, 4, sp) == RL_E_INVALID and b"scene" in _err()
    assert fn(None, 64, 36, 1, 0, 0, 0, None) == RL_E_INVALID and b"scene" in _err()
    assert s.tobytes() == bytes(s.nbytes)


def test_bad_arguments_after_the_scene_check():
    scene = _FakeScene().ptr
    rays, res = np.zeros(4, R.SPECTRAL_RAY_DTYPE), np.zeros(4, R.PATH_RESULT_DTYPE)
    rp, op = rays.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p)
    s = np.zeros(4, R.CAMERA_SAMPLE_DTYPE)
    sp = s.ctypes.data_as(C.c_void_p)
    for fn in (_lib.lib.rl_scene_render_rays, _lib.lib.rl_scene_render_rays_device):
        assert fn(scene, R.FETCH_LDS, 1, 0, 0, 65537, rp, 4, op) == RL_E_INVALID and b"max_segments" in _err()
        assert fn(scene, R.FETCH_LDS, 1, 0, 0, 0xffffffff, rp, 4, op) == RL_E_INVALID and b"max_segments" in _err()
        assert fn(scene, R.FETCH_LDS, 1, 0, 0, 65537, None, 0, None) == RL_E_INVALID and b"max_segments" in _err()
        assert fn(scene, R.FETCH_LDS, 1, 0, (1 << 64) - 4, 0, rp, 4, op) == RL_E_INVALID and b"2^64" in _err()
        assert fn(scene, R.FETCH_LDS, 1, 0, 0, 0, None, 4, op) == RL_E_INVALID and b"buffer" in _err()
        for ms in (0, 1, 65536):
            assert fn(scene, R.FETCH_LDS, 1, 0, 0, ms, None, 0, None) == 0   # n = 0 does nothing
    for fn in (_lib.lib.rl_scene_camera_rays, _lib.lib.rl_scene_camera_rays_device):
        assert fn(scene, 0, 36, 1, 0, 0, 4, sp) == RL_E_INVALID and b"zero" in _err()
        assert fn(scene, 64, 0, 1, 0, 0, 4, sp) == RL_E_INVALID and b"zero" in _err()
        assert fn(scene, 65536, 32768, 1, 0, 0, 4, sp) == RL_E_INVALID and b"RL_MAX_PIXELS" in _err()
        assert fn(scene, 64, 36, 1, 0, (1 << 64) - 2, 4, sp) == RL_E_INVALID and b"2^64" in _err()
        assert fn(scene, 64, 36, 1, 0, 0, 4, None) == RL_E_INVALID and b"buffer" in _err()
        assert fn(scene, 64, 36, 1, 0, 0, 0, None) == 0
    assert res.tobytes() == bytes(res.nbytes) and s.tobytes() == bytes(s.nbytes)


@pytest.fixture(scope="module")
def path_kernels():
    """Metadata of the path and camera kernels from the device-only -S compile with the library's own flags."""
    metadata = device_build()[1]
    return {n: k for n, k in metadata.items() if "rl_ray_paths_kernel" in n or "rl_camera_rays_kernel" in n}



def test_path_and_camera_kernels_are_free_of_scratch_and_spills(path_kernels):
    kernels = path_kernels
    paths = {n: k for n, k in kernels.items() if "rl_ray_paths_kernel" in n}
    camera = {n: k for n, k in kernels.items() if "rl_camera_rays_kernel" in n}
    assert len(paths) == PATH_VARIANTS and len(camera) == 1, sorted(kernels)
    for name, k in kernels.items():
        for taken in ("rl_trace_kernel", "rl_query_kernel", "rl_plot_kernel", "rl_gather_kernel", "rl_add_kernel", "rl_tonemap_kernel"):
            assert taken not in name   # the resource tests of the other kernels pick them out by these substrings
        assert k["private_segment_fixed_size"] == 0, (name, k)   # no scratch memory
        assert k["vgpr_spill_count"] == 0, (name, k)
    for name, k in paths.items():
        stage = int(re.search(r"rl_ray_paths_kernelILi([012])E", name).group(1))
        assert k["sgpr_spill_count"] == 0 if stage == 2 else k["sgpr_spill_count"] <= 32, (name, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (name, k)   # four waves per SIMD, as the query kernel
    assert camera[next(iter(camera))]["sgpr_spill_count"] == 0
    stages = sorted(re.search(r"rl_ray_paths_kernelILi([012])ELb([01])E", n).groups() for n in paths)
    assert stages == [(s, c) for s in "012" for c in "01"]


def test_path_oracle_reproduces_the_oracle_render_on_camera_rays():
    """tests/_path_oracle.py against the oracle's render (trace_unit.rs:151-168): fed the camera rays of the same paths -- from the
    host build of rl_begin_path (tests/host_mirror) -- it returns every photon's probability bit for bit and the same segment
    count.  This is what makes it a yardstick for rays no camera makes."""
    import _mirror as M
    import _oracle as O
    import _path_oracle as P
    for which, param in ((0, 0), (1, 0)):   # the demo scene and the glass stress scene
        objs, cam = M.builtin_desc(which, param)
        W, H, seed, stream, first, n = 320, 180, 11, 2, 1000, 300
        want, segs = O.Scene(objs, cam).render(W, H, seed, stream, first, n)
        ms = M.Scene(objs, cam)
        dump = M.lib().mirror_dump_rays   # (the first ray of a path: rl_begin_path)
        dump.restype = C.c_uint64
        dump.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
        rays = np.zeros((n, 6), np.float32)
        for i in range(n):
            assert dump(ms.h, W, H, seed, stream, first + i, 1, rays[i].ctypes.data, 1) == 1
        got = P.PathOracle(objs, cam).render_rays(rays[:, :3], rays[:, 3:], want["wavelength"], seed, stream, first)
        assert got["value"].tobytes() == want["probability"].tobytes(), which
        assert int(got["segments"].sum()) == segs
        assert (got["value"] != 0).any() and ((got["end"] == P.EMITTER) == (got["object"] != P.NONE)).all()
        assert ((got["end"] == P.EMITTER) | (got["value"] == 0)).all()


def _prologue(text, start):
    """The statements from the dynamic LDS declaration to the scene view's last field, comments and blank space dropped."""
    a = text.index("extern __shared__", start)
    b = text.index("sv.records = big;", a)
    body = re.sub(r"//[^\n]*", "", text[a:b])
    return re.sub(r"\s+", " ", body).strip()


def test_the_scene_is_staged_in_one_place():
    """The staging prologue is rl_stage_scene (rl_kernels.hip.h) and every persistent kernel beside the trace kernel calls it.  The
    trace body keeps the statements as its own text (calling the function changed its instructions): the one other place they
    appear, and it must not drift from the function."""
    headers = {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".h", ".hip"))}
    code = {n: re.sub(r"//[^\n]*", "", t) for n, t in headers.items()}
    for needle in ("extern __shared__ __attribute__((aligned(512)))", "sv.records = big"):
        assert {n: t.count(needle) for n, t in code.items() if needle in t} == {"rl_kernels.hip.h": 2}, needle
    kernels = headers["rl_kernels.hip.h"]
    first, second = kernels.index("RlStagedScene rl_stage_scene("), kernels.index("void rl_trace_body(")
    assert first < second
    a, b = _prologue(kernels, first), _prologue(kernels, second)
    assert a == b and len(a) > 1000
    assert kernels.index("extern __shared__", first) < second   # (the first copy is the function's, the second the trace body's)
    for name, kernel in (("rl_query.hip.h", "void rl_query_kernel("), ("rl_paths.hip.h", "void rl_paths_body("), ("rl_step.hip.h", "void rl_step_kernel(")):
        text = headers[name]
        start = text.index(kernel)
        assert "rl_stage_scene<STAGE>(scene, lay)" in text[start:start + 1500], name
    paths = headers["rl_paths.hip.h"]
    for wrapper in ("void rl_ray_paths_kernel(", "void rl_film_paths_kernel("):
        start = paths.index(wrapper)
        assert "rl_paths_body<STAGE, CYL," in paths[start:start + 800], wrapper
