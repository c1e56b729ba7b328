"""Every kernel family on the scenes of tests/_scenes.py's EXTREME_SCENES -- descriptions at the two thresholds of the staging rule,
with 39 / 40 / 41 and up to 1,000 prisms, with 0 to 200 planes and circles and 65 paraboloids, 50-way exact ties, and scenes of
one object (tests/test_scene_extremes.py holds each to its shape and to the property it is named for, on the host).  Bit for bit
against the CPU oracles, the films by the film tests' bars:

    trace        un-fused / fused x plain / open, 4,096 paths: photons, fused films (assert_film), segment counts
    query        rl_scene_intersect and rl_scene_occluded on ray_sets' seven families filled up to 4,033 rays, t_max = inf and
    occlusion      per ray (t_max_cases)
    path, film   rl_scene_render_rays, rl_plot_unit_render_samples on 2,113 paths against _path_oracle
    step         rl_scene_step_paths to the end against _step_oracle, every state and hit after every step
    list step    rl_scene_step_path_list from the identity list against _path_list_oracle, three steps
    light        rl_scene_light_paths against _light_oracle on the scene with _with_lights' emitters appended; on a scene without
                 an emitter every state gets RL_LIGHT_SKIPPED
    light film   rl_plot_unit_light_paths: the samples, the `sampled` bytes and the film of _light_film_oracle's photons
    direct       rl_plot_unit_render_direct against _direct_oracle.cpu_direct, films 16 x 9 and 64 x 36, max_segments 3
    features     rl_scene_render_features against _feature_oracle.cpu_features, the same films

in both fetch modes.  After every call the family's launch counter must name exactly the variant that tests/_mirror.py's statement
of the staging rule predicts from the host mirror's layout figures (an open launch of the trace kernel carries 2,064 bytes more
scratch, so at the thresholds it stages less than a plain one); the last test holds every family to all of its variants and the
variants that stage nothing to having run under RL_FETCH_LDS, by the scene's size.  prisms-stack-200, small-200 and edge-whole run
the trace, query and light families once more on poisoned LDS.  Nothing here provokes a fault."""
import time
import zlib

import numpy as np
import pytest

import _boundary as B
import _direct_oracle as DO
import _feature_oracle as FO
import _lds_poison as LP
import _light_film_oracle as LF
import _light_oracle as LO
import _mirror as M
import _oracle as O
import _path_list_oracle as L
import _path_oracle as P
import _query_rays as QR
import _step_oracle as S
from _boundary import _ocam
from _cases import _filter, _photons_of, _results, _wavelengths, blocked, oracle_hits, ray_sets, t_max_cases
from _compare import assert_film, assert_same, assert_same_bytes
from _device_arrays import _Device, _poison_hits, _prefilled
from _scenes import EXTREME_SCENES, _scene, _with_lights

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE, LIVE = R.RL_OBJECT_NONE, R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
FILMS = ((16, 9), (64, 36))
N = 4033          # 63 full waves and one lane
NP = 2113         # paths where the reference is a Python loop
TRACE_N = 1 << 12
MAX_SEGMENTS = 3
POISONED = ["prisms-stack-200", "small-200", "edge-whole"]
FAMILIES = ("query", "occlusion", "path", "film", "step", "path_list", "light", "light_film", "direct", "feature")
_ran = {family: set() for family in ("trace",) + FAMILIES}
_unstaged_by_size = {family: set() for family in ("trace",) + FAMILIES}     # scenes that ran a family with nothing staged under RL_FETCH_LDS
_wall = {"start": None}
_CASES = {}


class _Case:
    pass


def _case(name):
    """Scene `name` on the device, in the oracle and in the host mirror, with the mirror's layout figures; built once."""
    _wall["start"] = _wall["start"] or time.time()
    if name not in _CASES:
        c = _Case()
        c.name = name
        objs, cam = _scene(name)
        c.objs, c.cam = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), cam
        c.scene, c.oscene = R.Scene(c.objs, c.cam), O.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(cam))
        c.lay = M.layout(M.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(cam)))
        _CASES[name] = c
    return _CASES[name]


def _lit_case(name):
    """... and the same description with _with_lights' six emitters appended, as a case of its own."""
    if ("lit", name) not in _CASES:
        base = _case(name)
        c = _Case()
        c.name = name + " with lights"
        c.objs, c.cam = np.ascontiguousarray(_with_lights(base.objs, np.random.default_rng(zlib.crc32(name.encode())))).view(R.OBJECT_DTYPE), base.cam
        c.scene = R.Scene(c.objs, c.cam)
        c.lay = M.layout(M.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam)))
        _CASES[("lit", name)] = c
    return _CASES[("lit", name)]


def _meant(c, fetch, open_launch=False):
    """(stage, cylinders) the library must pick for case c: the rule as tests/_mirror.py states it, on the mirror's figures."""
    return M.predicted_stage(c.lay, fetch == R.FETCH_LDS, open_launch)[0], c.lay["prism_cylinders"]


def _held(family, launches, c, fetch, call, *args, **kwargs):
    """call(*args, fetch=fetch, **kwargs), held to the one variant predicted for the scene; records that it ran."""
    before = launches()
    got = call(*args, fetch=fetch, **kwargs)
    _ran_as(family, launches, before, c, fetch)
    return got


def _ran_as(family, launches, before, c, fetch):
    v = B._variant_of(launches, before)
    stage, cyl = _meant(c, fetch)
    assert v == 2 * stage + cyl, "%s on %s fetch %d: variant %d ran, predicted stage %d cylinders %d (%r)" % (family, c.name, fetch, v, stage, cyl, c.lay)
    _ran[family].add(v)
    if fetch == R.FETCH_LDS and stage == M.STAGE_NONE:
        _unstaged_by_size[family].add(c.name)


# ---- the trace kernel ---------------------------------------------------------------------------------------------------------

def _trace(c, want, segs, fetch, fused, open_launch, what, before_launch=None):
    seed, stream, first = 5, 2, 777
    t = R.TraceUnit(0, W, H, n_photons=TRACE_N)
    t.set_fetch(fetch)
    p = R.PlotUnit(0, W, H) if fused else None
    if p is not None:
        p.sync()
    before = R.variant_launches()
    if before_launch:
        before_launch()
    if not fused:
        if open_launch:
            t.render(c.scene, seed=seed, stream=stream, first_path_index=first)
        else:
            t.render_async(c.scene, seed=seed, stream=stream, first_path_index=first)
            t.sync()
        got = t.mapped_photons
        if got.tobytes() != want.tobytes():
            rows = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1))
            raise AssertionError("%s: %d photons differ, first path %d: got %r want %r" % (what, len(rows), rows[0], got[rows[0]], want[rows[0]]))
    else:
        if open_launch:
            t.render_fused_sync(c.scene, p, TRACE_N, seed=seed, stream=stream, first_path_index=first)
        else:
            t.render_fused(c.scene, p, TRACE_N, seed=seed, stream=stream, first_path_index=first)
            t.sync()
        assert_film(p.tristimulus_buffer, W, H, want, what)
    assert t.stats()[:2] == (TRACE_N, segs), (what, t.stats()[:2], segs)
    v = B._variant_of(R.variant_launches, before)
    stage, cyl = _meant(c, fetch, open_launch)
    low = (4 if fused else 0) | (2 if open_launch else 0) | cyl
    meant = 16 + low if stage == M.STAGE_TABLES else (8 if stage == M.STAGE_ALL else 0) | low
    assert v == meant, "%s: trace variant %d ran, predicted %d (stage %d; %r)" % (what, v, meant, stage, c.lay)
    _ran["trace"].add(v)
    if fetch == R.FETCH_LDS and stage == M.STAGE_NONE:
        _unstaged_by_size["trace"].add(c.name)


def _trace_reference(c):
    if not hasattr(c, "photons"):
        c.photons = c.oscene.render(W, H, 5, 2, 777, TRACE_N, threads=16)
        assert bool((c.photons[0]["probability"] != 0).any()) == bool((c.objs["material_kind"] == 0).any()), c.name   # black without a light only
    return c.photons


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_trace_kernel_bit_exact_in_every_launch_kind(name):
    c = _case(name)
    want, segs = _trace_reference(c)
    for fetch in FETCHES:
        for fused in (False, True):
            for open_launch in (False, True):
                _trace(c, want, segs, fetch, fused, open_launch, "%s fetch %d %s %s" % (name, fetch, "fused" if fused else "unfused", "open" if open_launch else "plain"))


# ---- rays: query and occlusion ------------------------------------------------------------------------------------------------

def _ray_case(name):
    """_case(name) with ray_sets' families at 560 rays each, filled up to N with camera rays, a per-ray t_max and the oracle's answers."""
    c = _case(name)
    if not hasattr(c, "o"):
        rng = np.random.default_rng(zlib.crc32(("extremes " + name).encode()))
        sets = ray_sets(c.scene, c.objs, c.cam, rng, 560)
        has_spheres = bool(((c.objs["surface_kind"] == 0) & (c.objs["f"][:, 0] > 0)).any())
        assert set(sets) == {"camera", "bounce", "uniform", "non_unit", "degenerate"} | ({"tangent", "far"} if has_spheres else set()), (name, sorted(sets))
        os_, ds_ = [s[0] for s in sets.values()], [s[1] for s in sets.values()]
        have = sum(len(x) for x in os_)
        assert have < N
        po, pd = QR.camera_rays(c.cam, 1920, 1080, rng, N - have)
        c.o = np.ascontiguousarray(np.concatenate(os_ + [po]), dtype=np.float32)
        c.d = np.ascontiguousarray(np.concatenate(ds_ + [pd]), dtype=np.float32)
        assert len(c.o) == len(c.d) == N
        c.hits_inf = oracle_hits(c.oscene, c.o, c.d)
        hit = c.hits_inf["object"] != NONE
        assert hit.any() and not hit.all(), name
        c.t = t_max_cases(c.hits_inf, rng)
        c.hits_t = _filter(c.hits_inf, c.t)
        c.blocked_inf, c.blocked_t = blocked(c.hits_inf, np.float32(np.inf)), blocked(c.hits_inf, c.t)
        assert c.blocked_t.any() and not c.blocked_t.all(), name
    return c


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_queries_and_occlusion_bit_exact_over_every_ray_family(name):
    c = _ray_case(name)
    inf = np.full(N, np.inf, np.float32)
    for fetch in FETCHES:
        for t, hits, shadow, tag in ((inf, c.hits_inf, c.blocked_inf, "t_max inf"), (c.t, c.hits_t, c.blocked_t, "t_max cases")):
            what = "%s fetch %d %s" % (name, fetch, tag)
            assert_same(_held("query", R.query_launches, c, fetch, c.scene.intersect, c.o, c.d, t), hits, what)
            assert_same_bytes(_held("occlusion", R.occlusion_launches, c, fetch, c.scene.occluded, c.o, c.d, t), shadow, what + ": occluded")


# ---- paths: render_rays, render_samples, step_paths to the end ------------------------------------------------------------------

def _path_case(name):
    """NP of the case's rays with wavelengths (an eighth odd) as paths first .. of (seed, stream): the path oracle's results and the
    step oracle's states and hits turn by turn until nothing is live."""
    c = _ray_case(name)
    if not hasattr(c, "rays"):
        rng = np.random.default_rng(zlib.crc32(("extreme paths " + name).encode()))
        sel = np.sort(np.random.default_rng(N).permutation(N)[:NP])
        rays = np.zeros(NP, R.SPECTRAL_RAY_DTYPE)
        rays["origin"], rays["direction"], rays["wavelength"] = c.o[sel], c.d[sel], _wavelengths(rng, NP)
        c.seed, c.stream, c.first = 5, 2, int(rng.integers(0, 1 << 40))
        c.want_paths = P.PathOracle(c.objs, c.cam).render_rays(rays["origin"], rays["direction"], rays["wavelength"], c.seed, c.stream, c.first).view(R.PATH_RESULT_DTYPE)
        assert (c.want_paths["end"] != R.RL_PATH_END_LIMIT).all(), name
        so = S.StepOracle(c.objs, c.cam)
        c.begun = S.begin(rays, c.first).view(R.PATH_STATE_DTYPE)
        want, want_hits = c.begun.copy(), _poison_hits(NP)
        c.steps = []
        while (want["end"] == LIVE).any():
            assert len(c.steps) < R.RL_PATH_MAX_SEGMENTS
            so.step(want, c.seed, c.stream, hits=want_hits)
            c.steps.append((want.copy(), want_hits.copy()))
        assert_same(_results(c.steps[-1][0]), c.want_paths, "%s: the step oracle's final states against the path oracle" % name)
        c.rays = rays
    return c


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_paths_films_and_steps_to_the_end_match_the_oracles(name):
    c = _path_case(name)
    rng = np.random.default_rng(zlib.crc32(("extreme film " + name).encode()))
    samples = np.zeros(NP, R.CAMERA_SAMPLE_DTYPE)
    samples["ray"] = c.rays
    samples["x"] = rng.uniform(-1.005, 1.005, NP).astype(np.float32)
    samples["y"] = (rng.uniform(-1.005, 1.005, NP) * H / W).astype(np.float32)
    photons = _photons_of(samples, c.want_paths)
    photons = photons[np.isfinite(photons["wavelength"])]
    begun = c.scene.begin_paths(c.rays, c.first)
    assert_same(begun, c.begun, name + ": begin_paths")
    for fetch in FETCHES:
        what = "%s fetch %d" % (name, fetch)
        got = _held("path", R.path_launches, c, fetch, c.scene.render_spectral_rays, c.rays, c.seed, c.stream, c.first)
        assert_same(got, c.want_paths, what + ": render_rays")
        p = R.PlotUnit(0, W, H)
        p.sync()
        res = _held("film", R.film_launches, c, fetch, p.render_samples, c.scene, samples, c.seed, c.stream, c.first)
        assert_same(res, c.want_paths, what + ": render_samples")
        assert_film(p.tristimulus_buffer, W, H, photons, what + ": render_samples")
        st, hits = begun.copy(), _poison_hits(NP)
        for k, (want, want_hits) in enumerate(c.steps):
            _held("step", R.step_launches, c, fetch, c.scene.step_paths, st, c.seed, c.stream, hits=hits)
            assert_same(st, want, "%s step %d: states" % (what, k))
            assert_same(hits, want_hits, "%s step %d: hits" % (what, k))
        assert (st["end"] != LIVE).all(), what


# ---- the listed step --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_listed_steps_match_the_list_oracle(name):
    """Three listed steps from the identity list: the states, the hits and the survivors' list after each are _path_list_oracle's."""
    c = _path_case(name)
    so = S.StepOracle(c.objs, c.cam)
    ost, ohits, olive, turns = c.begun.copy().view(S.begin(c.rays[:1], 0).dtype), _poison_hits(NP), None, []
    for _ in range(MAX_SEGMENTS):
        olive = L.step_list(so, ost, c.seed, c.stream, list=olive, hits=ohits)
        turns.append((ost.copy().view(R.PATH_STATE_DTYPE), ohits.copy(), olive.copy()))
    assert len(turns[0][2]) > 0 or (turns[0][0]["end"] != LIVE).all(), name
    for fetch in FETCHES:
        st, hits, live = c.begun.copy(), _poison_hits(NP), None
        for k, (want, want_hits, want_live) in enumerate(turns):
            what = "%s fetch %d listed step %d" % (name, fetch, k)
            if live is not None and len(live) == 0:
                assert len(want_live) == 0, what      # (an empty list makes no launch)
                continue
            live = _held("path_list", R.path_list_launches, c, fetch, c.scene.step_path_list, st, c.seed, c.stream, list=live, hits=hits)
            assert live.tolist() == want_live.tolist(), what
            assert_same(st, want, what + ": states")
            assert_same(hits, want_hits, what + ": hits")


# ---- direct light: light_paths, the light film, render_direct; and the feature render ---------------------------------------------

def _vertex_case(c):
    """Case c (its scene, whatever lights it has) with NP camera paths of the CPU oracles after two segments -- after one on the
    scenes of one object, where no path has a second vertex: camera samples, states, hits, and the light oracle's samples for them."""
    if not hasattr(c, "vertex"):
        objs, cam = c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam)
        seed, stream, first = 7, 1, 1 << 34
        camera = DO.oracle_camera_samples(objs, cam, W, H, seed, stream, first, NP).view(R.CAMERA_SAMPLE_DTYPE)
        assert_same(c.scene.camera_rays(W, H, seed, stream, first, NP), camera, c.name + ": camera_rays against the oracles")
        so = S.StepOracle(objs, cam)
        st, hits = S.begin(np.ascontiguousarray(camera["ray"]), first), _poison_hits(NP)
        for _ in range(1 if c.name.startswith("min-") else 2):
            so.step(st, seed, stream, hits=hits)
        st = st.view(R.PATH_STATE_DTYPE)
        want = LO.light_paths(LO.Occluder(objs, cam), st, hits, seed, stream, samples=_prefilled(NP).view(LO.SAMPLE_DTYPE)).view(R.LIGHT_SAMPLE_DTYPE)
        c.vertex = (seed, stream, first, camera, st, hits, want)
    return c.vertex


def _light_calls(c, name, before_launch=None):
    """rl_scene_light_paths and rl_plot_unit_light_paths on case c's vertex states in both fetch modes: every byte of the samples,
    the `sampled` bytes and the films of the rule's photons."""
    seed, stream, first, camera, st, hits, want = _vertex_case(c)
    emitters = c.scene.emitters()
    assert emitters.tolist() == LO.emitters(c.objs.view(O.OBJECT_DTYPE)).tolist(), name
    if len(emitters) == 0:
        assert (want["status"] == R.RL_LIGHT_SKIPPED).all(), name
    photons, after = LF.film_photons(st, want, emitters, camera, np.zeros(NP, np.uint8))
    for fetch in FETCHES:
        what = "%s fetch %d" % (c.name, fetch)
        if before_launch:
            before_launch()
        got = _held("light", R.light_launches, c, fetch, c.scene.light_paths, st, hits, seed, stream, samples=_prefilled(NP))
        assert_same(got, want, what + ": light_paths")
        for w, h in FILMS:
            plot, sampled = R.PlotUnit(0, w, h), np.zeros(NP, np.uint8)
            plot.sync()
            if before_launch:
                before_launch()
            got = _held("light_film", R.light_film_launches, c, fetch, plot.light_paths, c.scene, st, hits, camera, seed, stream, sampled=sampled,
                        samples=_prefilled(NP))
            assert_same(got, want, "%s %dx%d: the light film's samples" % (what, w, h))
            assert sampled.tobytes() == after.tobytes(), what
            assert_film(plot.tristimulus_buffer, w, h, photons, "%s %dx%d: light film" % (what, w, h))
    return want


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_light_samples_and_light_films_match_the_oracles(name):
    lit = _lit_case(name)
    want = _light_calls(lit, name)
    share = np.bincount(want["status"], minlength=4) / float(NP)
    print("%s: light sample statuses (skipped, backfacing, occluded, visible) %s" % (lit.name, share))
    diffuse = bool(np.isin(lit.objs["material_kind"], (1, 2)).any())      # (only a diffuse vertex is sampled; among 670 spheres every
    assert (share[R.RL_LIGHT_SKIPPED] < 1) == diffuse, (name, share)      # sample may be occluded or behind its surface, none visible)
    bare = _case(name)
    if not (bare.objs["material_kind"] == 0).any():      # no emitter at all: nothing to sample, every state is skipped
        assert len(bare.scene.emitters()) == 0
        skipped = _light_calls(bare, name)
        assert (skipped["status"] == R.RL_LIGHT_SKIPPED).all() and not skipped["value"].any(), name


def _poisoned_results(n):
    res = np.zeros(n, R.PATH_RESULT_DTYPE)
    res["end"], res["segments"], res["value"] = 12345, 0xAAAAAAAA, np.nan
    return res


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_direct_render_matches_the_cpu_composition(name):
    c = _lit_case(name)
    seed, stream, first = 4, 2, 1 << 33
    loop = DO.cpu_direct(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam), W, H, seed, stream, first, NP, MAX_SEGMENTS)
    want, photons, want_stats = loop.prefix(NP)
    assert (want_stats["light_samples"] > 0) == bool(np.isin(c.objs["material_kind"], (1, 2)).any()) and len(photons) > 0, (name, want_stats)
    for fetch in FETCHES:
        for w, h in FILMS:
            what = "%s fetch %d %dx%d" % (c.name, fetch, w, h)
            plot, rb = R.PlotUnit(0, w, h), _Device(_poisoned_results(NP))
            plot.sync()
            stats = _held("direct", R.direct_launches, c, fetch, plot.render_direct, c.scene, seed, stream, first, NP, max_segments=MAX_SEGMENTS, results=rb.buf)
            assert_same(rb.get(), want.view(R.PATH_RESULT_DTYPE), what + ": results")
            assert stats == want_stats, (what, stats, want_stats)
            assert_film(plot.tristimulus_buffer, w, h, photons, what + ": render_direct")


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_feature_render_matches_the_cpu_composition(name):
    c = _lit_case(name)
    seed, stream, first = 4, 2, 1 << 33
    want, want_stats = FO.cpu_features(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam), W, H, seed, stream, first, NP, MAX_SEGMENTS).prefix(NP)
    for fetch in FETCHES:
        for w, h in FILMS:
            what = "%s fetch %d %dx%d" % (c.name, fetch, w, h)
            plots = [R.PlotUnit(k, w, h) for k in range(3)]
            rb = _Device(np.frombuffer(bytes([0xA5]) * (48 * NP), dtype=R.FEATURE_SAMPLE_DTYPE).copy())
            stats = _held("feature", R.feature_launches, c, fetch, c.scene.render_features, w, h, seed, stream, first, NP, max_segments=MAX_SEGMENTS,
                          records=rb.buf, **dict(zip(FO.FILMS, plots)))
            assert_same(rb.get(), want.view(R.FEATURE_SAMPLE_DTYPE), what + ": records")
            assert stats == want_stats, (what, stats, want_stats)
            for film, plot in zip(FO.FILMS, plots):
                FO.assert_film(plot.tristimulus_buffer, w, h, want, film, what)


# ---- poisoned LDS: the last LDS step and the rings that wrap most ---------------------------------------------------------------

@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
@pytest.mark.parametrize("name", POISONED)
def test_trace_query_and_light_on_poisoned_lds(name, pattern):
    """Every CU's LDS filled with the pattern immediately before each launch (tests/test_gpu_dirty_state.py has the control that the
    pattern is what the next kernel finds): the trace kernel's four launch kinds, the query and the light call, the light film."""
    c = _ray_case(name)
    want, segs = _trace_reference(c)
    poison = lambda: LP.poison_lds(pattern)
    for fused in (False, True):
        for open_launch in (False, True):
            _trace(c, want, segs, R.FETCH_LDS, fused, open_launch, "%s pattern 0x%08X %s %s" % (name, pattern, "fused" if fused else "unfused",
                                                                                               "open" if open_launch else "plain"), before_launch=poison)
    before = R.query_launches()
    poison()
    got = c.scene.intersect(c.o, c.d, c.t, fetch=R.FETCH_LDS)
    _ran_as("query", R.query_launches, before, c, R.FETCH_LDS)
    assert_same(got, c.hits_t, "%s pattern 0x%08X: query" % (name, pattern))
    _light_calls(_lit_case(name), name, before_launch=poison)


# ---- what ran -----------------------------------------------------------------------------------------------------------------------

def test_every_family_ran_every_variant_and_nothing_staged_was_reached_by_size():
    """Per family, the variants that ran on these scenes: all 24 of the trace kernel, all six of every other family; and in every
    family a scene too large for its tables ran the variant that stages nothing under RL_FETCH_LDS."""
    if _wall["start"]:
        print("tests/test_gpu_scene_extremes.py: %.0f s from the first case to here" % (time.time() - _wall["start"]))
    for family in ("trace",) + FAMILIES:
        print("%s: variants %s; nothing staged under LDS fetch on %s" % (family, sorted(_ran[family]), sorted(_unstaged_by_size[family])))
    assert _ran["trace"] == set(range(24)), sorted(set(range(24)) - _ran["trace"])
    for family in FAMILIES:
        assert _ran[family] == set(range(6)), (family, sorted(_ran[family]))
    for family in ("trace",) + FAMILIES:
        assert {"prisms-1000", "edge-tables+1"} <= {n.replace(" with lights", "") for n in _unstaged_by_size[family]}, (family, _unstaged_by_size[family])
