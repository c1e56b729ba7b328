"""The kernels on the scene shapes of tests/_scenes.py's SHAPE_SCENES -- descriptions whose order, flags and coincident objects no
generator of the other tests makes (tests/test_scene_shapes.py holds each to the branch of rl_scan_wave it is there for) -- and on
rays from far outside a scene (tests/_cases.py: far_rays), whose coarse distances tie distinct spheres.  Bit for bit against the
CPU oracle: the trace kernel in all eight launch kinds, rl_scene_intersect and rl_scene_occluded over every ray family and t_max
case, the step loop to its end and step by step; each call on the kernel variant the scene is meant to reach."""
import ctypes as C
import zlib

import numpy as np
import pytest

import _boundary as B
import _oracle as O
import _step_oracle as S
from _boundary import _ocam
from _cases import _filter, blocked, far_rays, oracle_hits, ray_sets, t_max_cases
from _compare import assert_film, assert_same, assert_same_bytes
from _device_arrays import _Device, _begin_device, _poison_hits
from _scenes import SHAPE_SCENES, _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE, LIVE = R.RL_OBJECT_NONE, R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
# What an LDS-fetch call stages (R.query_launches: 2 the whole scene, 1 its tables): the three rooms whole -- with the flags
# test_scene_shapes.py asserts, that selects six<false>, the ordered loop on tables in LDS and the general loop on z normals --
# shuffled-3000 its tables, shuffled-6000 its tables with a third level (that its table has one is test_scene_shapes.py's to hold:
# the third level's code is in the variants that do not stage the whole scene, and runs wherever the table has supers).
STAGE = {"room-tilted": 2, "room-plus-disc": 2, "room-reordered": 2, "shuffled-40": 2, "shuffled-300": 2, "shuffled-3000": 1,
         "shuffled-6000": 1, "coincident-300": 2, "coincident-3000": 1}
FAR_SCENES = ["demo", "demo-2500", "random-6000", "random-20000"]   # two and three table levels, staged and not
_CASES = {}


class _Case:
    pass


def _case(name):
    """Scene `name` on the device and in the oracle; built once, no test writes into it."""
    if name not in _CASES:
        c = _Case()
        c.objs, c.cam = _scene(name)
        c.objs = np.ascontiguousarray(c.objs).view(R.OBJECT_DTYPE)
        c.scene, c.oscene = R.Scene(c.objs, c.cam), O.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam))
        c.cyl = int((c.objs["surface_kind"] == 4).sum() >= 40)
        _CASES[name] = c
    return _CASES[name]


def _ray_case(name):
    """... with ray_sets' families at 4,096 rays each and the oracle's hits for them."""
    c = _case(name)
    if not hasattr(c, "sets"):
        c.sets = ray_sets(c.scene, c.objs, c.cam, np.random.default_rng(zlib.crc32(name.encode())), 4096)
        assert set(c.sets) >= {"camera", "bounce", "uniform", "non_unit", "tangent", "degenerate", "far"}, sorted(c.sets)
        c.want = {kind: oracle_hits(c.oscene, o, d) for kind, (o, d) in c.sets.items()}
        assert len(c.sets["far"][0]) >= 4000 and (c.want["far"]["object"] != NONE).mean() > 0.3, name
    return c


def _stage_ran(launches, before, c, name, fetch):
    v = B._variant_of(launches, before)
    assert v == 2 * (STAGE[name] if fetch == R.FETCH_LDS else 0) + c.cyl, (name, fetch, v)


def _on_variant(launches, c, name, fetch, call, *args):
    """call(*args, fetch=fetch), held to the one kernel variant the scene is meant to run on."""
    before = launches()
    got = call(*args, fetch=fetch)
    _stage_ran(launches, before, c, name, fetch)
    return got


@pytest.mark.parametrize("name", SHAPE_SCENES)
@pytest.mark.parametrize("open_launch", [False, True], ids=["plain", "open"])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("fetch", FETCHES, ids=["lds", "global"])
def test_trace_kernel_bit_exact_in_every_launch_kind(fetch, fused, open_launch, name):
    """test_gpu_parity.py's matrix on the shape scenes: photons byte for byte, the fused film by the project's tolerance against the
    oracle's plot of its photons, (paths, segments) exactly, and the instantiation meant is the one that ran."""
    c = _case(name)
    n = 1 << 13 if name == "shuffled-6000" else 1 << 15
    seed, stream, first = 5, 2, 777
    if not hasattr(c, "photons"):
        c.photons = c.oscene.render(W, H, seed, stream, first, n, threads=16)
        assert (c.photons[0]["probability"] != 0).mean() >= 0.05, name   # an all-black film cannot pass
    want, segs = c.photons
    t = R.TraceUnit(0, W, H, n_photons=n)
    t.set_fetch(fetch)
    before = R.variant_launches()
    if not fused:
        if open_launch:
            t.render(c.scene, seed=seed, stream=stream, first_path_index=first)
        else:
            t.render_async(c.scene, seed=seed, stream=stream, first_path_index=first)
            t.sync()
        assert t.mapped_photons.tobytes() == want.tobytes()
    else:
        p = R.PlotUnit(0, W, H)
        if open_launch:
            t.render_fused_sync(c.scene, p, n, seed=seed, stream=stream, first_path_index=first)
        else:
            t.render_fused(c.scene, p, n, seed=seed, stream=stream, first_path_index=first)
            t.sync()
        assert_film(p.tristimulus_buffer, W, H, want, "%s fetch %d open %d" % (name, fetch, open_launch))
    assert t.stats()[:2] == (n, segs)
    ran = [a - b for a, b in zip(R.variant_launches(), before)]
    staged = 0 if fetch != R.FETCH_LDS else (8 if STAGE[name] == 2 else 16)
    meant = staged | (4 if fused else 0) | (2 if open_launch else 0) | c.cyl
    assert ran[meant] >= 1 and sum(ran) == ran[meant], (name, meant, ran)


@pytest.mark.parametrize("name", SHAPE_SCENES)
def test_queries_bit_exact_over_every_ray_family(name):
    c = _ray_case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    for kind, (o, d) in c.sets.items():
        want = c.want[kind]
        t_max = t_max_cases(want, rng)
        want_t = _filter(want, t_max)
        for fetch in FETCHES:
            got = _on_variant(R.query_launches, c, name, fetch, c.scene.intersect, o, d)
            assert_same(got, want, "%s %s fetch %d t_max inf" % (name, kind, fetch))
            got = _on_variant(R.query_launches, c, name, fetch, c.scene.intersect, o, d, t_max)
            assert_same(got, want_t, "%s %s fetch %d t_max cases" % (name, kind, fetch))


@pytest.mark.parametrize("name", SHAPE_SCENES)
def test_occlusion_bit_exact_over_every_ray_family(name):
    """The far family's t_max cases are where the any-hit scan's bound meets the far cull: exactly the distance must not block,
    its nextafter must."""
    c = _ray_case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 2)
    for kind, (o, d) in c.sets.items():
        want = c.want[kind]
        for t in (np.float32(np.inf), t_max_cases(want, rng)):
            answer = blocked(want, t)
            for fetch in FETCHES:
                got = _on_variant(R.occlusion_launches, c, name, fetch, c.scene.occluded, o, d, t)
                assert_same_bytes(got, answer, "%s %s fetch %d t_max %s" % (name, kind, fetch, "inf" if np.ndim(t) == 0 else "per ray"))
        if kind == "far":
            assert 0.05 < blocked(want, t).mean() < 0.95, name   # (the per-ray cases: both answers occur)


def _step_device(scene, sb, seed, stream, fetch, hb=None):
    R.check(R.lib.rl_scene_step_paths_device(scene.handle, fetch, seed, stream, 0, C.c_void_p(sb.buf.data_ptr()), len(sb.host),
                                             C.c_void_p(hb.buf.data_ptr()) if hb is not None else None))


@pytest.mark.parametrize("name", SHAPE_SCENES)
def test_step_loop_to_its_end_carries_the_oracles_photons(name):
    """4,096 camera paths begun and stepped until none is live: the value and the segment count of every path are the oracle's."""
    c = _case(name)
    n, seed, stream, first = 4096, 3 + len(name), 1, 1000
    want, segs = c.oscene.render(W, H, seed, stream, first, n, threads=16)
    rays = np.ascontiguousarray(c.scene.camera_rays(W, H, seed, stream, first, n)["ray"])
    for fetch in FETCHES:
        sb = _begin_device(c.scene, rays, first)
        steps = 0
        before = R.step_launches()
        while steps < R.RL_PATH_MAX_SEGMENTS and (sb.get()["end"] == LIVE).any():
            _step_device(c.scene, sb, seed, stream, fetch)
            steps += 1
        _stage_ran(R.step_launches, before, c, name, fetch)
        final = sb.get()
        assert (final["end"] != LIVE).all() and (final["end"] != R.RL_PATH_END_LIMIT).all(), (name, fetch)
        assert final["value"].tobytes() == want["probability"].tobytes(), (name, fetch)
        assert int(final["segments"].sum()) == segs and steps == int(final["segments"].max()), (name, fetch, steps)


FAMILIES = ["camera", "bounce", "uniform", "non_unit", "tangent", "degenerate", "far"]


@pytest.mark.parametrize("name", SHAPE_SCENES)
@pytest.mark.parametrize("kind", FAMILIES)
def test_every_step_matches_the_step_oracle(kind, name):
    """All of one ray family of ray_sets at 4,096 rays (the tangent family has 1,024 by its make, the degenerate one 48) as begun
    states: every field of every state and of every hit equals tests/_step_oracle.py's after each of three steps, in both fetch
    modes, on the variant meant.  One family a case: the oracle's side is a Python loop."""
    c = _ray_case(name)
    o, d = c.sets[kind]
    assert len(o) >= {"tangent": 1024, "degenerate": 48, "bounce": 1024, "far": 4000}.get(kind, 4096), (name, kind, len(o))   # (bounce: the camera rays that hit)
    seed, stream, first = 5 + len(name), 2, 1 << 33
    rays = np.zeros(len(o), R.SPECTRAL_RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["wavelength"] = np.random.default_rng(zlib.crc32((name + kind).encode())).uniform(380.0, 780.0, len(o)).astype(np.float32)
    so = S.StepOracle(c.objs, c.cam)
    want_st, want_hits = S.begin(rays, first), _poison_hits(len(rays))
    got = {f: (_begin_device(c.scene, rays, first), _Device(_poison_hits(len(rays)))) for f in FETCHES}
    for step in range(3):
        so.step(want_st, seed, stream, hits=want_hits)
        for fetch, (sb, hb) in got.items():
            before = R.step_launches()
            _step_device(c.scene, sb, seed, stream, fetch, hb=hb)
            _stage_ran(R.step_launches, before, c, name, fetch)
            assert_same(sb.get(), want_st, "%s %s step %d fetch %d: states" % (name, kind, step, fetch))
            assert_same(hb.get(), want_hits, "%s %s step %d fetch %d: hits" % (name, kind, step, fetch))
    assert (want_st["segments"] >= 1).all() and (kind == "degenerate" or (want_st["end"] != S.VOID).mean() > 0.2), (name, kind)   # (it hit things)


@pytest.mark.parametrize("name", FAR_SCENES)
def test_far_rays_on_the_large_scenes(name):
    """The far family through query and occlusion on scenes with two and three table levels: ties between spheres of different
    clusters, rings and rounds, and the far-bound cull at equality."""
    objs, cam = _scene(name)
    objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)
    scene, oscene = R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    o, d = far_rays(objs, 4096)
    want = oracle_hits(oscene, o, d)
    assert len(o) >= 4000 and (want["object"] != NONE).mean() > 0.3
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 3)
    t_max = t_max_cases(want, rng)
    want_t = _filter(want, t_max)
    staged = {"demo": 2, "demo-2500": 1, "random-6000": 1}

    def held(launches, call, *args):
        """call(*args, fetch=fetch) on the variant meant: none of these scenes has 40 prisms; a table with a third level is never
        staged with the whole scene, and whether random-20000's tables fit beside a kernel's scratch is the library's to say."""
        before = launches()
        got = call(*args, fetch=fetch)
        v = B._variant_of(launches, before)
        assert v % 2 == 0, (name, fetch, v)
        if fetch != R.FETCH_LDS:
            assert v // 2 == 0, (name, fetch, v)
        elif name in staged:
            assert v // 2 == staged[name], (name, fetch, v)
        else:
            assert v // 2 <= 1, (name, fetch, v)
        return got

    for fetch in FETCHES:
        assert_same(held(R.query_launches, scene.intersect, o, d), want, "%s far fetch %d t_max inf" % (name, fetch))
        assert_same(held(R.query_launches, scene.intersect, o, d, t_max), want_t, "%s far fetch %d t_max cases" % (name, fetch))
        for t in (np.float32(np.inf), t_max):
            assert_same_bytes(held(R.occlusion_launches, scene.occluded, o, d, t), blocked(want, t), "%s far fetch %d occluded" % (name, fetch))
