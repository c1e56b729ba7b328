"""rl_plot_unit_render_direct at the boundary, without a GPU: the entry points and their bindings, the argument checks in the
documented order, the branches the GPU tests' inputs reach (on the CPU statement of the contract, tests/_direct_oracle.py), the
compiled kernels' resources (hipcc cross-compiles here) and the command line's direct mode."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _direct_oracle as DO
import _oracle as O
from _boundary import _Fake, _err
from _device_build import kernels, variant_of_name  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
# the GPU tests' smallest inputs (tests/test_gpu_direct.py)
PATHS = dict(w=320, h=180, seed=4, stream=2, first=1 << 33, n=4097)


def test_both_symbols_are_exported_and_bound():
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    name = "rl_plot_unit_render_direct"
    assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header)
    assert hasattr(_lib.lib, "rl_debug_direct_launches") and "rl_debug_direct_launches" in _lib.DEBUG_SIGNATURES
    assert re.search(r"int rl_debug_direct_launches\(uint64_t out\[6\]\);", open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read())
    # RlDirectStats, field by field: seven uint64_t, 56 bytes, in the header's order in all three places
    fields = ["paths", "segments", "light_samples", "shadow_rays", "visible", "endings_kept", "endings_dropped"]
    assert [f for f, _ in _lib.RlDirectStats._fields_] == fields and all(t is C.c_uint64 for _, t in _lib.RlDirectStats._fields_)
    assert C.sizeof(_lib.RlDirectStats) == 56
    body = re.search(r"typedef struct RlDirectStats \{(.*?)\} RlDirectStats;\s*/\* 56 bytes \*/", header, re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", body) == fields
    body = re.search(r"pub struct RlDirectStats \{(.*?)\} // 56 bytes", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): u64", body) == fields and len(re.findall(r"pub \w+:", body)) == 7
    assert callable(R.PlotUnit.render_direct)
    assert len(R.direct_launches()) == 6 and _lib.lib.rl_debug_direct_launches(None) == RL_E_INVALID
    assert tuple(DO.STATS) == tuple(fields)


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    fn = _lib.lib.rl_plot_unit_render_direct
    unit, scene = _Fake().ptr, _Fake().ptr
    res = np.full(4 * 4 + 8, 0xAAAAAAAA, np.uint32)
    rp = C.c_void_p(res.ctypes.data + (-res.ctypes.data) % 16)
    odd = C.c_void_p(rp.value + 8)
    stats = _lib.RlDirectStats(*([0xAA] * 7))
    sp = C.byref(stats)
    LDS, TOP = R.FETCH_LDS, 2 ** 64 - 2
    # 1. unit, 2. scene, 3. fetch, 4. max_segments, 5. path range, 6. alignment: each with everything behind it wrong as well
    cases = [((None, None, 7, 1, 0, TOP, 5, 70000, odd, sp), b"plot unit"), ((None, scene, LDS, 1, 0, 0, 4, 0, rp, sp), b"plot unit"),
             ((unit, None, 7, 1, 0, TOP, 5, 70000, odd, sp), b"scene"), ((unit, None, LDS, 1, 0, 0, 4, 0, rp, sp), b"scene"),
             ((unit, scene, 7, 1, 0, TOP, 5, 70000, odd, sp), b"fetch"), ((unit, scene, -1, 1, 0, 0, 4, 0, rp, sp), b"fetch"),
             ((unit, scene, LDS, 1, 0, TOP, 5, 70000, odd, sp), b"max_segments"), ((unit, scene, LDS, 1, 0, 0, 4, 65537, rp, sp), b"max_segments"),
             ((unit, scene, LDS, 1, 0, TOP, 5, 65536, odd, sp), b"path indices"), ((unit, scene, LDS, 1, 0, TOP, 1, 0, rp, sp), b"path indices"),
             ((unit, scene, LDS, 1, 0, 2 ** 63, 2 ** 63, 0, rp, sp), b"path indices"),
             ((unit, scene, LDS, 1, 0, 0, 4, 0, odd, sp), b"aligned"), ((unit, scene, R.FETCH_GLOBAL, 1, 0, TOP - 4, 4, 65536, odd, None), b"aligned")]
    for args, word in cases:
        assert fn(*args) == RL_E_INVALID and word in _err(), (args, _err())
        assert all(getattr(stats, f) == 0xAA for f, _ in stats._fields_), args      # a refused call writes nothing
    assert (res == 0xAAAAAAAA).all()
    # n_paths == 0: nothing but *stats, which becomes all zero; results and stats may be NULL
    for fetch in (LDS, R.FETCH_GLOBAL):
        stats = _lib.RlDirectStats(*([0xAA] * 7))
        assert fn(unit, scene, fetch, 1, 0, TOP, 0, 65536, rp, C.byref(stats)) == 0
        assert all(getattr(stats, f) == 0 for f, _ in stats._fields_)
        assert fn(unit, scene, fetch, 1, 0, 0, 0, 0, None, None) == 0
    assert (res == 0xAAAAAAAA).all()


@pytest.fixture(scope="module")
def cpu_demo():
    """{max_segments: the contract on the CPU for the GPU tests' smallest inputs}."""
    objs, cam = O.demo_scene_desc()
    return {ms: DO.cpu_direct(objs, cam, PATHS["w"], PATHS["h"], PATHS["seed"], PATHS["stream"], PATHS["first"], PATHS["n"], ms) for ms in (0, 3)}


def test_the_gpu_tests_inputs_reach_every_branch(cpu_demo):
    """demo, seed 4, stream 2, 320x180, 4097 paths from 2^33: on the CPU oracles alone, every counter moves, endings are kept and
    dropped, every sample status occurs, and the segment limit ends paths at max_segments = 3 and none at 0."""
    for ms, direct in cpu_demo.items():
        results, photons, stats = direct.prefix(PATHS["n"])
        print("max_segments %d: %s, %d photons, statuses %s" % (ms, stats, len(photons), sorted(direct.statuses)))
        assert stats["paths"] == PATHS["n"] and all(stats[f] > 0 for f in DO.STATS), stats
        assert stats["endings_kept"] > 0 and stats["endings_dropped"] > 0
        assert stats["segments"] == int(results["segments"].sum())
        assert stats["light_samples"] >= stats["shadow_rays"] >= stats["visible"]
        assert direct.statuses == {R.RL_LIGHT_SKIPPED, R.RL_LIGHT_BACKFACING, R.RL_LIGHT_OCCLUDED, R.RL_LIGHT_VISIBLE}
        assert (results["end"] == R.RL_PATH_END_LIMIT).any() == (ms == 3)
        assert {R.RL_PATH_END_EMITTER, R.RL_PATH_END_ROULETTE} <= set(results["end"].tolist())      # (the scene is closed: no path leaves it)
        assert len(photons) > 1000
        # additive over a split that is no multiple of 64, and a prefix is the run of that prefix
        a, b = direct.span(0, 1000), direct.span(1000, PATHS["n"])
        assert all(a[f] + b[f] == stats[f] for f in DO.STATS)
    assert cpu_demo[0].prefix(65)[2]["segments"] >= cpu_demo[3].prefix(65)[2]["segments"]


def test_direct_kernels_hold_the_persistent_ray_kernels_bar(kernels):
    """Occupancy 4 under the path kernels' launch bounds: at most 128 VGPRs and no AGPRs; no scratch, no VGPR spills, no dynamic
    stack; no spilled SGPRs where the whole scene is staged and at most 32 elsewhere."""
    direct = {variant_of_name(n, "rl_direct_paths_kernel"): k for n, k in kernels.items() if "rl_direct_paths_kernel" in n}
    assert sorted(direct) == [(s, c) for s in "012" for c in "01"]
    for v, k in sorted(direct.items()):
        print("rl_direct_paths_kernel<%s, %s>: %d VGPRs, %d AGPRs, %d SGPRs spilled, %d bytes of scratch"
              % (v[0], v[1], k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_spill_count"], k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (v, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (v, k)
        assert k["sgpr_spill_count"] <= (0 if v[0] == "2" else 32), (v, k["sgpr_spill_count"])
        assert k["max_flat_workgroup_size"] == 1024, (v, k)
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_direct.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()


def test_the_command_line_parses_direct_and_refuses_what_it_cannot_combine(capsys):
    a = CLI.parse_args(["--direct", "--width", "64", "--height", "36", "--batches", "2", "--photons-per-batch", "4096", "--seed", "3",
                        "--output", "out.ppm", "--quiet"])
    assert a.direct and (a.width, a.height, a.batches, a.photons_per_batch, a.seed, a.output, a.quiet) == (64, 36, 2, 4096, 3, "out.ppm", True)
    assert a.max_segments is None and CLI.parse_args(["--direct", "--max-segments", "5"]).max_segments == 5
    for extra in (["--unfused"], ["--concurrency", "2"], ["--resume"]):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(["--direct"] + extra)
        told = capsys.readouterr().err
        assert e.value.code == 2 and extra[0] in told and "--direct" in told, told
    # without --direct the program reads its arguments as before
    plain = CLI.parse_args([])
    assert not plain.direct and plain.concurrency == 2 and not plain.unfused and not plain.resume and plain.output == "output.png"
    assert CLI.parse_args(["--concurrency", "3", "--unfused", "--resume"]).concurrency == 3


def test_write_image_makes_a_ppm_and_a_png(tmp_path):
    import struct
    import zlib
    w, h = 5, 3
    rgb = (np.arange(w * h * 3) % 251).astype(np.uint8).reshape(-1, 3)
    CLI.write_image(str(tmp_path / "a.ppm"), rgb, w, h)
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n5 3\n255\n" + rgb.tobytes()
    CLI.write_image(str(tmp_path / "a.png"), rgb, w, h)
    png = (tmp_path / "a.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR" and struct.unpack(">IIBBBBB", png[16:29]) == (w, h, 8, 2, 0, 0, 0)
    at, data = 8, b""
    while at < len(png):
        n, kind = struct.unpack(">I", png[at:at + 4])[0], png[at + 4:at + 8]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(png[at + 4:at + 8 + n]) & 0xffffffff
        data += png[at + 8:at + 8 + n] if kind == b"IDAT" else b""
        at += 12 + n
    rows = zlib.decompress(data)
    assert rows == b"".join(b"\x00" + rgb.tobytes()[y * w * 3:(y + 1) * w * 3] for y in range(h))
