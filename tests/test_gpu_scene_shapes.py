"""The kernels on the scene shapes of tests/_scenes.py's SHAPE_SCENES -- descriptions whose order, flags and coincident objects no
generator of the other tests makes (tests/test_scene_shapes.py holds each to the branch of rl_scan_wave it is there for) -- and on
rays from far outside a scene (tests/_cases.py: far_rays), whose coarse distances tie distinct spheres.  Bit for bit against the
CPU oracle: the trace kernel in all eight launch kinds, rl_scene_intersect and rl_scene_occluded over every ray family and t_max
case, the step loop to its end and step by step; each call on the kernel variant the scene is meant to reach.

And on rays from far outside at anything but spheres, up to the largest finite origin (tests/_cases.py: far_families; what the
oracle makes of each family on each scene is held in tests/test_scene_shapes.py).  The families:
    far-prisms, far-others   unit rays from 10^3 .. 10^8 units away at the prisms / at planes, circles and paraboloids
    deep                     from 10^8 .. 10^11.9 at every kind: the f32 direction no longer holds its target, hits are rounding's
    limit                    from 10^11.9 .. 10^12.1: hit distances up to the 1e12 below which alone a hit counts (scene.rs:43),
                             also under t_max = 1e12 and its two f32 neighbours
    beyond                   from 10^12.1 to FLT_MAX, with bands where |o|^2 overflows (1.8e19) and where the prism shortcut's tagged
                             quotients are infinities with a plane number in their low bits (1e33 up), components equal to
                             FLT_MAX, origins displaced along one axis: the oracle reports a miss for every ray
    edge-*                   camera rays whose f32 |d|^2 - 1 is -2^-20, 2^-20 and the four f32 neighbours: both sides of the switch
                             between the culled and the exact scan, each group compared on its own
The scenes (FAR_ON): the built-in scene's 22 prisms alone, with its spheres, with its paraboloids (in the closed room the walls
take every far ray before a prism); the glass-stress scene's sphere and 66 prisms, which runs the CYL variants and their cylinder
bound; the whole built-in scene for walls and paraboloids; random-6000 for a cull table with a third level.  The trace kernel draws
its own rays, so its camera is moved back instead (test_trace_kernel_bit_exact_from_a_camera_moved_back)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import _boundary as B
import _oracle as O
import _step_oracle as S
from _boundary import _ocam
from _cases import _filter, blocked, far_families, far_rays, oracle_hits, ray_sets, t_max_cases
from _compare import assert_film, assert_same, assert_same_bytes
from _device_arrays import _Device, _begin_device, _poison_hits
from _scenes import SHAPE_SCENES, _scene, camera_moved_back

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


# ---- rays from far outside, at anything but spheres -------------------------------------------------------------------------------

# (every one of these but random-6000 is staged whole under LDS fetch; glass-spheres-prisms has 66 prisms and runs CYL)
STAGE.update({"demo-prisms": 2, "demo-spheres-prisms": 2, "demo-prisms-paraboloids": 2, "glass-spheres-prisms": 2, "demo-open": 2,
              "demo": 2, "random-6000": 1})
FAR_ON = ["demo-prisms", "demo-spheres-prisms", "demo-prisms-paraboloids", "glass-spheres-prisms", "demo", "random-6000"]   # smallest first
EDGES = ["edge-below-outside", "edge-below-on", "edge-below-inside", "edge-above-inside", "edge-above-on", "edge-above-outside"]


def _families(name):
    """The families far_families makes for scene `name`."""
    others = ["far-others"] if name in ("demo-prisms-paraboloids", "demo", "random-6000") else []
    return ["far-prisms"] + others + ["deep", "limit", "beyond"] + (EDGES if name == "demo" else [])


FAR_CASES = [(name, family) for name in FAR_ON for family in _families(name)]


def _far_case(name):
    """_case(name) with far_families' rays and the oracle's hits for them."""
    c = _case(name)
    if not hasattr(c, "far_sets"):
        c.far_sets = far_families(c.objs, c.cam, 4096, edge=name == "demo")
        assert list(c.far_sets) == _families(name), (name, list(c.far_sets))
        c.far_want = {family: oracle_hits(c.oscene, o, d) for family, (o, d) in c.far_sets.items()}
        assert (c.cyl == 1) == (name == "glass-spheres-prisms"), name
    return c


@pytest.mark.parametrize("name,family", FAR_CASES)
def test_queries_and_occlusion_bit_exact_from_far_outside(name, family):
    """rl_scene_intersect and rl_scene_occluded under t_max = inf and the per-ray cases, in both fetch modes, each call on the
    variant meant; the limit family also under t_max = 1e12 and its f32 neighbours.  From beyond 1e12 every answer is a miss:
    all-zero records, nothing blocked."""
    c = _far_case(name)
    (o, d), want = c.far_sets[family], c.far_want[family]
    if family == "beyond":
        assert (want["object"] == NONE).all() and not want["distance"].any() and not want["position"].any(), name
    rng = np.random.default_rng(zlib.crc32((name + family).encode()))
    bounds = [np.float32(np.inf), t_max_cases(want, rng)]
    if family == "limit":
        bounds += [np.nextafter(np.float32(1e12), np.float32(0)), np.float32(1e12), np.nextafter(np.float32(1e12), np.float32(np.inf))]
    for k, t in enumerate(bounds):
        want_t, answer = _filter(want, t), blocked(want, t)
        for fetch in FETCHES:
            what = "%s %s fetch %d t_max %s" % (name, family, fetch, ["inf", "per ray", "below 1e12", "1e12", "above 1e12"][k])
            got = _on_variant(R.query_launches, c, name, fetch, c.scene.intersect, o, d) if k == 0 else \
                _on_variant(R.query_launches, c, name, fetch, c.scene.intersect, o, d, t)
            assert_same(got, want_t, what)
            assert_same_bytes(_on_variant(R.occlusion_launches, c, name, fetch, c.scene.occluded, o, d, t), answer, what + ": occluded")


@pytest.mark.parametrize("name,family", FAR_CASES)
def test_every_step_from_far_outside_matches_the_step_oracle(name, family):
    """test_every_step_matches_the_step_oracle on the far families: rl_intersect_segment inside a path.  Every field of every state
    and hit after each of three steps, in both fetch modes, on the variant meant; a path from beyond 1e12 ends in the void at once."""
    c = _far_case(name)
    o, d = c.far_sets[family]
    seed, stream, first = 7 + len(name), 3, 1 << 34
    rays = np.zeros(len(o), R.SPECTRAL_RAY_DTYPE)
    rays["origin"], rays["direction"] = o, d
    rays["wavelength"] = np.random.default_rng(zlib.crc32((name + family).encode()) + 1).uniform(380.0, 780.0, len(o)).astype(np.float32)
    so = S.StepOracle(c.objs, c.cam)
    want_st, want_hits = S.begin(rays, first), _poison_hits(len(rays))
    got = {f: (_begin_device(c.scene, rays, first), _Device(_poison_hits(len(rays)))) for f in FETCHES}
    for step in range(3):
        so.step(want_st, seed, stream, hits=want_hits)
        if family == "beyond":
            assert (want_st["end"] == S.VOID).all() and (want_st["segments"] == 1).all(), name
        for fetch, (sb, hb) in got.items():
            before = R.step_launches()
            _step_device(c.scene, sb, seed, stream, fetch, hb=hb)
            _stage_ran(R.step_launches, before, c, name, fetch)
            assert_same(sb.get(), want_st, "%s %s step %d fetch %d: states" % (name, family, step, fetch))
            assert_same(hb.get(), want_hits, "%s %s step %d fetch %d: hits" % (name, family, step, fetch))
    assert (want_st["segments"] >= 1).all(), (name, family)


MOVED = [("demo", 10.0, False), ("demo-open", 1e4, True), ("demo-open", 1e7, True)]
_MOVED = {}


@pytest.mark.parametrize("name,back,telescope", MOVED, ids=["demo-10", "demo-open-1e4", "demo-open-1e7"])
@pytest.mark.parametrize("open_launch", [False, True], ids=["plain", "open"])
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("fetch", FETCHES, ids=["lds", "global"])
def test_trace_kernel_bit_exact_from_a_camera_moved_back(fetch, fused, open_launch, name, back, telescope):
    """test_trace_kernel_bit_exact_in_every_launch_kind at 2^13 paths with the camera translated back along its view axis.
    The built-in scene is a closed room: from 10^7, 10^6, ... down to 10^2 units further back the camera stands outside its walls
    and the oracle's film is black (no photon of 8,192 is non-zero), so by the 5 % rule that scene is rendered from the next
    lower power of ten, 10 units back, for both distances.  The far renders are of demo-open -- the same scene without its plane
    and paraboloids -- from 10^4 and 10^7 units back through a field of view narrowed to keep the scene in the frame (over a
    twentieth of the photons are non-zero at either): camera rays that start 10^4 and 10^7 units from everything they meet."""
    if (name, back) not in _MOVED:
        c = _Case()
        objs, cam = _scene(name)
        c.objs, c.cam = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), camera_moved_back(cam, back, telescope)
        c.scene, c.oscene = R.Scene(c.objs, c.cam), O.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam))
        c.cyl = 0
        _MOVED[(name, back)] = c
    c = _MOVED[(name, back)]
    n, seed, stream, first = 1 << 13, 5, 2, 777
    if not hasattr(c, "photons"):
        c.photons = c.oscene.render(W, H, seed, stream, first, n, threads=16)
        assert (c.photons[0]["probability"] != 0).mean() >= 0.05, (name, back)   # an all-black film cannot pass
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
        assert_film(p.tristimulus_buffer, W, H, want, "%s back %g fetch %d open %d" % (name, back, fetch, open_launch))
    assert t.stats()[:2] == (n, segs)
    ran = [a - b for a, b in zip(R.variant_launches(), before)]
    meant = (8 if fetch == R.FETCH_LDS else 0) | (4 if fused else 0) | (2 if open_launch else 0)
    assert ran[meant] >= 1 and sum(ran) == ran[meant], (name, back, meant, ran)


TOP = float(np.log10(np.finfo(np.float32).max))


@pytest.mark.parametrize("which", [R.SCENE_DEMO, R.SCENE_GLASS_STRESS], ids=["demo", "glass"])
@pytest.mark.parametrize("band", [(8.0, 12.0), (12.0, TOP), (34.0, TOP)], ids=["1e8-1e12", "1e12-FLT_MAX", "1e34-FLT_MAX"])
def test_prism_shortcut_on_the_device_from_far_origins_never_contradicts_the_tree(band, which):
    """rl_hex_prism_fast as the device builds it -- v_rcp_f32, the running extrema from v_max3_f32 / v_min3_f32 -- against the
    Compound tree, both on the GPU (rl_debug_prism_probe), on tests/host_mirror's pairs from 10^8 units away to FLT_MAX.  From
    about 1e33 the tagged quotients are infinities with a plane number in their low bits, NaN patterns to the three-operand
    instructions; the host build's fmaxf / fminf ignore them.  Held: the device's tree is the g++ build's; whatever the device's
    shortcut decides is that tree's answer bit for bit; and it decides, not less than a sixth of the pairs.  What the two builds
    decide is printed side by side: they need not decide the same pairs (the reciprocals differ by an ulp as it is)."""
    import _mirror as M
    objs, cam = R.builtin_scene_desc(which)
    scene = R.Scene(objs, cam)
    ms = M.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    trials, seed = 400_000, 20261020 + which
    prisms, rays, tree = M.prism_pairs(ms, trials, seed, band=band)
    host = M.prism_fast_check(ms, trials, seed, band=band)
    assert len(prisms) == host["pairs"] > 300_000 and R.prism_count(scene) > prisms.max()
    assert (tree[:, 0] != 0xffffffff).sum() == host["tree_hits"] > 0.02 * len(prisms)      # the same pairs, and hits to contradict
    hits = misses = undecided = 0
    for p in np.unique(prisms):
        sel = prisms == p
        out = R.prism_probe(scene, p, rays[sel])
        assert (out[:, 3:5][out[:, 3] != 0xffffffff] == tree[sel][tree[sel][:, 0] != 0xffffffff]).all()   # same tree on both sides
        assert ((out[:, 3] == 0xffffffff) == (tree[sel][:, 0] == 0xffffffff)).all()
        hit, miss = out[:, 0] == 1, out[:, 0] == 0
        assert (out[hit, 1] == out[hit, 3]).all() and (out[hit, 2] == out[hit, 4]).all()   # a decided hit: the tree's t and half-space
        assert (out[miss, 3] == 0xffffffff).all()                                          # a decided miss: the tree misses
        hits, misses, undecided = hits + int(hit.sum()), misses + int(miss.sum()), undecided + int((out[:, 0] == 2).sum())
    print("band 10^%g .. 10^%g scene %d: device decides %d hits, %d misses, leaves %d; host %r" % (band + (which, hits, misses, undecided, host)))
    assert hits + misses + undecided == len(prisms) and hits + misses > len(prisms) / 6
