"""rl_scene_render_features at the boundary, without a GPU: the entry points and their bindings field by field, the argument checks
in the documented order, the kinds the GPU tests' inputs reach (on the CPU statement of the contract, tests/_feature_oracle.py),
the compiled kernels' resources (hipcc cross-compiles here) and the command line's --features."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _direct_oracle as DO
import _feature_oracle as FO
import _oracle as O
import _random_scene as RS
from _boundary import _Fake, _err
from _device_build import kernels, variant_of_name  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
# the GPU tests' smallest inputs (tests/test_gpu_features.py)
PATHS = dict(w=320, h=180, seed=4, stream=2, first=1 << 33, n=4097)
# (VOID, EMITTER, DIFFUSE, LIMIT) of those paths, per scene and max_segments
TABLE = {("demo", 1): (0, 121, 2410, 1566), ("demo", 2): (0, 143, 2862, 1092), ("demo", 3): (0, 156, 3361, 580), ("demo", 64): (0, 171, 3925, 1),
         ("random-1", 3): (5, 98, 3285, 709), ("random-1", 64): (6, 274, 3817, 0)}


def test_the_symbols_are_exported_and_bound_field_by_field():
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    name = "rl_scene_render_features"
    assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header)
    assert len(_lib.SIGNATURES[name][1]) == 14
    assert hasattr(_lib.lib, "rl_debug_feature_launches") and "rl_debug_feature_launches" in _lib.DEBUG_SIGNATURES
    assert re.search(r"int rl_debug_feature_launches\(uint64_t out\[6\]\);", open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read())
    # RlFeatureStats: 48 bytes, paths, segments and four kinds in all three places
    assert [(f, C.sizeof(t)) for f, t in _lib.RlFeatureStats._fields_] == [("paths", 8), ("segments", 8), ("kinds", 32)]
    assert C.sizeof(_lib.RlFeatureStats) == 48
    assert re.search(r"typedef struct RlFeatureStats \{\s*uint64_t paths, segments, kinds\[4\];.*?\} RlFeatureStats;\s*/\* 48 bytes \*/", header, re.S)
    body = re.search(r"pub struct RlFeatureStats \{(.*?)\} // 48 bytes", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,\n]+),", body) == [("paths", "u64"), ("segments", "u64"), ("kinds", "[u64; 4]")]
    # RlFeatureSample: 48 bytes, twelve words in the header's order in all four places
    fields = ["x", "y", "wavelength", "albedo", "normal", "depth", "object", "segments", "kind", "reserved"]
    assert [f for f, _ in _lib.RlFeatureSample._fields_] == fields and C.sizeof(_lib.RlFeatureSample) == 48
    assert list(R.FEATURE_SAMPLE_DTYPE.names) == fields and R.FEATURE_SAMPLE_DTYPE.itemsize == 48 and R.FEATURE_SAMPLE_DTYPE == FO.FEATURE_DTYPE
    for f in fields:
        assert getattr(_lib.RlFeatureSample, f).offset == R.FEATURE_SAMPLE_DTYPE.fields[f][1], f
    body = re.search(r"typedef struct RlFeatureSample \{(.*?)\} RlFeatureSample;\s*/\* 48 bytes \*/", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [n.strip() for stmt in body.split(";") if stmt.strip() for n in stmt.split(None, 1)[1].split(",")] == fields
    body = re.search(r"pub struct RlFeatureSample \{(.*?)\} // 48 bytes", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == fields
    # the enum and the default
    kinds = ["RL_FEATURE_VOID", "RL_FEATURE_EMITTER", "RL_FEATURE_DIFFUSE", "RL_FEATURE_LIMIT"]
    for value, kind in enumerate(kinds):
        assert re.search(r"%s = %d\b" % (kind, value), header) and re.search(r"pub const %s: u32 = %d;" % (kind, value), rust)
        assert getattr(_lib, kind) == value and getattr(R, kind[3:]) == value
    assert (FO.VOID, FO.EMITTER, FO.DIFFUSE, FO.LIMIT) == (0, 1, 2, 3)
    assert re.search(r"#define RL_FEATURE_MAX_SEGMENTS 64\b", header) and re.search(r"pub const RL_FEATURE_MAX_SEGMENTS: u32 = 64;", rust)
    assert _lib.RL_FEATURE_MAX_SEGMENTS == FO.MAX_SEGMENTS == 64
    assert callable(R.Scene.render_features)
    assert len(R.feature_launches()) == 6 and _lib.lib.rl_debug_feature_launches(None) == RL_E_INVALID


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    fn = _lib.lib.rl_scene_render_features
    scene, a, b, c = _Fake().ptr, _Fake().ptr, _Fake().ptr, _Fake().ptr
    rec = np.full(12 * 4 + 8, 0xAAAAAAAA, np.uint32)
    rp = C.c_void_p(rec.ctypes.data + (-rec.ctypes.data) % 16)
    odd = C.c_void_p(rp.value + 8)
    stats = _lib.RlFeatureStats(0xAA, 0xAA, (C.c_uint64 * 4)(0xAA, 0xAA, 0xAA, 0xAA))
    sp = C.byref(stats)
    LDS, TOP = R.FETCH_LDS, 2 ** 64 - 2
    # 1. scene, 2. fetch, 3. image size, 4. max_segments, 5. path range, 6. alignment, 7. distinct units: each with everything behind
    # it wrong as well, and alone
    cases = [((None, 7, 0, 0, 1, 0, TOP, 5, 70000, a, a, a, odd, sp), b"scene"), ((None, LDS, 16, 9, 1, 0, 0, 4, 0, a, b, c, rp, sp), b"scene"),
             ((scene, 7, 0, 0, 1, 0, TOP, 5, 70000, a, a, a, odd, sp), b"fetch"), ((scene, -1, 16, 9, 1, 0, 0, 4, 0, a, b, c, rp, sp), b"fetch"),
             ((scene, LDS, 0, 9, 1, 0, TOP, 5, 70000, a, a, a, odd, sp), b"zero image size"), ((scene, LDS, 16, 0, 1, 0, 0, 4, 0, a, b, c, rp, sp), b"zero image size"),
             ((scene, LDS, 65536, 32768, 1, 0, TOP, 5, 70000, a, a, a, odd, sp), b"RL_MAX_PIXELS"),
             ((scene, LDS, 16, 9, 1, 0, TOP, 5, 70000, a, a, a, odd, sp), b"max_segments"), ((scene, LDS, 16, 9, 1, 0, 0, 4, 65537, a, b, c, rp, sp), b"max_segments"),
             ((scene, LDS, 16, 9, 1, 0, TOP, 5, 65536, a, a, a, odd, sp), b"path indices"), ((scene, LDS, 16, 9, 1, 0, TOP, 1, 0, a, b, c, rp, sp), b"path indices"),
             ((scene, LDS, 16, 9, 1, 0, 2 ** 63, 2 ** 63, 0, a, b, c, rp, sp), b"path indices"),
             ((scene, LDS, 16, 9, 1, 0, 0, 4, 0, a, a, a, odd, sp), b"aligned"), ((scene, R.FETCH_GLOBAL, 16, 9, 1, 0, TOP - 4, 4, 65536, a, b, c, odd, None), b"aligned"),
             ((scene, LDS, 16, 9, 1, 0, 0, 4, 0, a, a, None, rp, sp), b"distinct"), ((scene, LDS, 16, 9, 1, 0, 0, 4, 0, a, None, a, rp, sp), b"distinct"),
             ((scene, LDS, 16, 9, 1, 0, 0, 0, 0, None, b, b, None, sp), b"distinct")]
    for args, word in cases:
        assert fn(*args) == RL_E_INVALID and word in _err(), (args, _err())
        assert stats.paths == 0xAA and stats.segments == 0xAA and list(stats.kinds) == [0xAA] * 4, args      # a refused call writes nothing
    assert (rec == 0xAAAAAAAA).all()
    # n_paths == 0: nothing but *stats, which becomes all zero; units, records and stats may be NULL
    for fetch in (LDS, R.FETCH_GLOBAL):
        stats = _lib.RlFeatureStats(0xAA, 0xAA, (C.c_uint64 * 4)(0xAA, 0xAA, 0xAA, 0xAA))
        assert fn(scene, fetch, 16, 9, 1, 0, TOP, 0, 65536, a, b, c, rp, C.byref(stats)) == 0
        assert stats.paths == 0 and stats.segments == 0 and list(stats.kinds) == [0] * 4
        assert fn(scene, fetch, 16, 9, 1, 0, 0, 0, 0, None, None, None, None, None) == 0
    assert (rec == 0xAAAAAAAA).all()


@pytest.fixture(scope="module")
def cpu_runs():
    """{(scene, max_segments): the contract on the CPU for the GPU tests' smallest inputs}; one set of camera samples per scene."""
    runs = {}
    for name, (objs, cam) in (("demo", O.demo_scene_desc()), ("random-1", RS.random_scene(1))):
        camera = DO.oracle_camera_samples(objs, cam, PATHS["w"], PATHS["h"], PATHS["seed"], PATHS["stream"], PATHS["first"], PATHS["n"])
        for (scene, ms) in TABLE:
            if scene == name:
                runs[(scene, ms)] = FO.cpu_features(objs, cam, PATHS["w"], PATHS["h"], PATHS["seed"], PATHS["stream"], PATHS["first"], PATHS["n"],
                                                    0 if ms == 64 else ms, camera=camera)
    return runs


def test_the_gpu_tests_inputs_reach_every_kind_where_the_table_says(cpu_runs):
    """Seed 4, stream 2, 320x180, 4097 paths from 2^33, on the CPU oracles alone: the counts of the four kinds on the built-in scene
    (closed: no VOID) and on random_scene(1) (the VOID case), and stats that add up over a cut at 1000."""
    for key, run in sorted(cpu_runs.items()):
        records, stats = run.prefix(PATHS["n"])
        print(key, stats, "longest chain", int(records["segments"].max()))
        assert tuple(stats["kinds"]) == TABLE[key], (key, stats)
        assert stats["paths"] == PATHS["n"] == sum(stats["kinds"]) and stats["segments"] == int(records["segments"].sum())
        assert FO.add_stats(run.span(0, 1000), run.span(1000, PATHS["n"])) == stats
        # the records hold the contract's own invariants
        surface = (records["kind"] == FO.EMITTER) | (records["kind"] == FO.DIFFUSE)
        assert ((records["object"] != FO.NONE) == surface).all() and not records["normal"][~surface].any() and not records["albedo"][~surface].any()
        assert np.allclose(np.linalg.norm(records["normal"][surface], axis=1), 1, atol=1e-4)
        assert (records["segments"][records["kind"] == FO.LIMIT] == (64 if key[1] == 64 else key[1])).all()
        assert ((records["depth"] == 0) == ((records["kind"] == FO.VOID) & (records["segments"] == 1))).all()
        assert not records["reserved"].any()
    demo = cpu_runs[("demo", 64)].records
    assert 3 < int(demo["segments"][demo["kind"] != FO.LIMIT].max()) < 64   # chains well past the limits 1, 2, 3 (19 segments here), and one path still in glass at 64
    assert np.isin(demo["kind"][:65], (FO.EMITTER, FO.DIFFUSE)).all()        # the first 1 / 63 / 64 / 65 paths are all DIFFUSE or EMITTER
    # a path's record up to the limit does not depend on the limit
    for ms in (1, 2, 3):
        short = cpu_runs[("demo", ms)].records
        same = short["kind"] != FO.LIMIT
        assert short[same].tobytes() == demo[same].tobytes() and (demo["segments"][~same] > ms).all()


def test_feature_kernels_hold_the_persistent_ray_kernels_bar(kernels):
    """Occupancy 4 under the path kernels' launch bounds: at most 128 VGPRs and no AGPRs; no scratch, no VGPR spills, no dynamic
    stack; no spilled SGPRs where the whole scene is staged and at most 32 elsewhere."""
    feature = {variant_of_name(n, "rl_feature_paths_kernel"): k for n, k in kernels.items() if "rl_feature_paths_kernel" in n}
    assert sorted(feature) == [(s, c) for s in "012" for c in "01"]
    for v, k in sorted(feature.items()):
        print("rl_feature_paths_kernel<%s, %s>: %d VGPRs, %d AGPRs, %d SGPRs spilled, %d bytes of scratch"
              % (v[0], v[1], k["vgpr_count"], k.get("agpr_count", 0), k["sgpr_spill_count"], k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (v, k)
        assert k["vgpr_count"] <= 128 and k.get("agpr_count", 0) == 0, (v, k)
        assert k["sgpr_spill_count"] <= (0 if v[0] == "2" else 32), (v, k["sgpr_spill_count"])
        assert k["max_flat_workgroup_size"] == 1024, (v, k)
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_features.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()


def test_the_command_line_parses_features_with_and_without_direct(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "2", "--photons-per-batch", "4096", "--seed", "3", "--quiet"]
    a = CLI.parse_args(base + ["--features", "guides"])
    assert a.features == "guides" and not a.direct and a.max_segments is None and a.concurrency == 2
    a = CLI.parse_args(base + ["--features", "out/g", "--direct", "--max-segments", "5"])
    assert a.features == "out/g" and a.direct and a.max_segments == 5
    assert CLI.parse_args(["--features", "g", "--max-segments", "3"]).max_segments == 3      # --max-segments applies to the guides too
    assert CLI.parse_args([]).features is None and CLI.parse_args(["--direct"]).features is None
    with pytest.raises(SystemExit) as e:
        CLI.parse_args(["--max-segments", "3"])
    told = capsys.readouterr().err
    assert e.value.code == 2 and "--max-segments" in told and "--features" in told and "--direct" in told, told
    with pytest.raises(SystemExit):
        CLI.parse_args(["--features"])
    capsys.readouterr()
