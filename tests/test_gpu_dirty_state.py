"""Every ray kernel on memory it did not write itself.

1. Dirty LDS.  Every kernel family runs the shared segment scan (rl_scan_wave, RlWaveScratch), which reads ring slots, merge keys,
the emitter queue and the camera stash that this launch has not necessarily written: a round of fewer than 64 pairs reads 64 ring
slots.  In a fresh process the LDS is zero or holds a benign earlier kernel's data, so a read of an unwritten slot passes by luck.
Here every CU's LDS is filled with a pattern (tests/_lds_poison.py) IMMEDIATELY before each launch under test -- all ones, the
quiet NaN, a plausible index -- and the results must still equal the family's own reference, bit for bit (the atomically summed
film within exactly the tolerances of tests/test_gpu_film.py, tests/_compare.py: assert_film): all 24 instantiations of the trace kernel and every variant of the
query, occlusion, path, film and step kernels in both fetch modes, on few rays (partial rounds everywhere), with a tail wave
(4,033 rays) and with lanes that have no work inside full waves (t_max 0 / negative / NaN, non-finite wavelengths, states that are
not live).  A control test first proves that the pattern IS what the next kernel finds; without it the rest would prove nothing.

2. Guarded, prefilled outputs.  Every _device form writes into a buffer of 0xAA between two 64-byte guards (tests/_guarded.py):
the guards must be intact and every byte of the n records must equal the host form's, padding and reserved fields included.

Order independence.  Queries, occlusion tests and stepped states are run a second time in a fixed random permutation and must
give the permuted bytes of the first run.  rl_scene_render_rays cannot be checked that way: ray i IS path first + i, so a permuted
batch draws other random numbers; its permuted run is compared with the path oracle's answer for the permuted batch instead, and
the permuted-bytes property of the path machinery is checked on the step kernel, whose states carry their path index."""
import time
import zlib

import numpy as np
import pytest

import _boundary as B
import _guarded as G
import _lds_poison as LP
import _occlusion_cases as OC
import _oracle as O
import _path_oracle as P
import _query_rays as QR
import _random_scene as RS
import _step_oracle as S
from _boundary import _ocam
from _cases import _filter, _photons_of, _results, _wavelengths, blocked, oracle_hits, ray_sets, synthetic_photons, t_max_cases
from _compare import assert_consistent, assert_film, assert_same, assert_same_bytes
from _device_arrays import _poison_hits, _upload
from _scenes import _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE, LIVE = R.RL_OBJECT_NONE, R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
PATTERNS = LP.PATTERNS
SCENES = ["demo", "many-prisms", "demo-2500", "tables-prisms", "random-6000"]   # whole scene / tables / third level, with and without CYL
N = 4033          # 63 full waves and one lane: a tail wave exists
NP = 2113         # rays of the path, film and step cases (33 waves and one lane): their references are Python loops
W, H = 320, 180
BATCHES = [1, 63, 64, 65, 4033]
PERM = np.random.default_rng(4033).permutation(N)
PPERM = np.random.default_rng(2113).permutation(NP)
_ran = {"trace": set(), "query": set(), "occlusion": set(), "path": set(), "film": set(), "step": set()}
_wall = {"start": None}


def _pid(p):
    return "0x%08X" % p


def _check_variant(v, cyl, fetch, what):
    assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)


# ---- 0. the control ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
def test_control_the_poison_is_what_the_next_kernel_finds(pattern):
    """poison, then peek (a kernel of the same grid and LDS size that writes no LDS and counts the words equal to the pattern).
    Asserted: lds_poison returned 0 and at least one workgroup found the pattern.  Printed: the measured persistence
    (profiles/lds_poison_control.txt).  If this fails, every other test of the module is vacuous."""
    _wall["start"] = _wall["start"] or time.time()
    LP.poison_lds(pattern)                     # (asserts that lds_poison returned 0)
    seen = LP.peek_lds(pattern)
    other = LP.peek_lds(pattern ^ 0x5A5A5A5A)  # a pattern nobody wrote: what "not found" looks like
    LP.poison_lds(pattern)
    staged = np.zeros(N, R.RAY_DTYPE)          # what a host form does between the poison and its kernel: a copy in, a copy out
    buf = QR.DeviceBuffer(staged.nbytes)
    buf.upload(staged)
    buf.download(staged)
    copied = LP.peek_lds(pattern)
    print("lds poison control: pattern %s, %d CUs: found in %d of %d workgroups, in %.4f %% of their words (per workgroup: min %.4f %%, "
          "max %.4f %%); a pattern that was not written: found in %d workgroups; with a host-to-device and a device-to-host copy "
          "between poison and peek: found in %d workgroups, in %.4f %% of their words"
          % (_pid(pattern), LP.cu_count(), seen["groups_found"], seen["groups"], 100.0 * seen["word_share"], 100.0 * seen["min_share"],
             100.0 * seen["max_share"], other["groups_found"], copied["groups_found"], 100.0 * copied["word_share"]))
    assert seen["groups_found"] >= 1, seen


# ---- the cases: rays and reference answers, computed once per scene ---------------------------------------------------------

class _Case:
    pass


_CASES = {}


def _case(name):
    """Scene `name` with N rays -- camera, bounce, uniform, non-unit, tangent, degenerate and short rays, filled up with camera
    rays -- a per-ray t_max (t_max_cases: inf, around the hit, 0, -1, NaN; the short rays keep theirs) and the oracle's answers."""
    if name in _CASES:
        return _CASES[name]
    c = _Case()
    c.name = name
    c.objs, c.cam = _scene(name)
    c.scene, c.oscene = R.Scene(c.objs, c.cam), O.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(c.cam))
    c.cyl = int((c.objs["surface_kind"] == 4).sum() >= 40)
    rng = np.random.default_rng(zlib.crc32(("dirty state " + name).encode()))
    sets = ray_sets(c.scene, c.objs, c.cam, rng, 640)
    cam_o, cam_d = sets["camera"]
    so, sd, st = OC.short_rays(cam_d, oracle_hits(c.oscene, cam_o, cam_d), rng)
    so, sd, st = so[:512], sd[:512], st[:512]
    os_, ds_ = [s[0] for s in sets.values()] + [so], [s[1] for s in sets.values()] + [sd]
    have = sum(len(x) for x in os_)
    short_rows = np.arange(have - len(so), have)
    assert have < N
    po, pd = QR.camera_rays(c.cam, 1920, 1080, rng, N - have)
    c.o = np.ascontiguousarray(np.concatenate(os_ + [po]), dtype=np.float32)
    c.d = np.ascontiguousarray(np.concatenate(ds_ + [pd]), dtype=np.float32)
    assert len(c.o) == len(c.d) == N
    c.hits_inf = oracle_hits(c.oscene, c.o, c.d)
    assert (c.hits_inf["object"] != NONE).mean() > 0.2, name
    c.t = t_max_cases(c.hits_inf, rng)
    bounded = c.t[short_rows] > 0                       # (the short rays keep t_max_cases' 0, -1 and NaN rows)
    c.t[short_rows[bounded]] = st[bounded]
    idle = ~(c.t > 0)                                   # t_max 0, negative or NaN: lanes without work inside full waves
    assert idle[:N - 1].reshape(-1, 64).any(axis=1).all() and np.isnan(c.t).any() and (c.t == 0).any()
    c.hits_t = _filter(c.hits_inf, c.t)
    c.blocked_inf, c.blocked_t = blocked(c.hits_inf, np.float32(np.inf)), blocked(c.hits_inf, c.t)
    assert 0.02 < c.blocked_t.mean() < 0.95, (name, c.blocked_t.mean())
    _CASES[name] = c
    return c


def _path_case(name):
    """NP of the case's rays with wavelengths (an eighth odd: outside the visible range, NaN, infinite) as paths first .. of
    (seed, stream), and the path oracle's results for them and for the same rays in the order PPERM."""
    c = _case(name)
    if hasattr(c, "rays"):
        return c
    rng = np.random.default_rng(zlib.crc32(("dirty paths " + name).encode()))
    sel = np.sort(PERM[:NP])
    rays = np.zeros(NP, R.SPECTRAL_RAY_DTYPE)
    rays["origin"], rays["direction"], rays["wavelength"] = c.o[sel], c.d[sel], _wavelengths(rng, NP)
    rays["reserved"] = 0xdeadbeef                        # ignored
    c.seed, c.stream, c.first = 5, 2, int(rng.integers(0, 1 << 40))
    invalid = ~np.isfinite(rays["wavelength"])
    assert invalid[:NP - 1].reshape(-1, 64).any(axis=1).mean() > 0.5    # lanes without a path inside full waves
    c.po = P.PathOracle(c.objs, c.cam)
    c.want_paths = c.po.render_rays(rays["origin"], rays["direction"], rays["wavelength"], c.seed, c.stream, c.first).view(R.PATH_RESULT_DTYPE)
    assert (c.want_paths["end"][invalid] == R.RL_PATH_END_INVALID).all() and (c.want_paths["end"] != R.RL_PATH_END_LIMIT).all()
    assert (c.want_paths["value"] != 0).sum() >= 20, name
    pr = rays[PPERM]
    c.want_paths_perm = c.po.render_rays(pr["origin"], pr["direction"], pr["wavelength"], c.seed, c.stream, c.first).view(R.PATH_RESULT_DTYPE)
    c.rays = rays
    # the camera half: N paths of the scene's own camera, the oracle's render of them and its segments path by path
    c.cam_seed, c.cam_stream, c.cam_first = 3 + len(name), 1, 1000
    c.cam_want, c.cam_segs = c.oscene.render(W, H, c.cam_seed, c.cam_stream, c.cam_first, N, threads=16)
    return c


def _step_case(name):
    """The step oracle on the path case's rays, turn by turn until nothing is live: [(states, hits) after step k]."""
    c = _path_case(name)
    if hasattr(c, "steps"):
        return c
    so = S.StepOracle(c.objs, c.cam)
    c.begun = S.begin(c.rays, c.first).view(R.PATH_STATE_DTYPE)
    want, want_hits = c.begun.copy(), _poison_hits(NP)
    c.steps = []
    while (want["end"] == LIVE).any():
        assert len(c.steps) < R.RL_PATH_MAX_SEGMENTS
        so.step(want, c.seed, c.stream, hits=want_hits)
        c.steps.append((want.copy(), want_hits.copy()))
    assert_same(_results(c.steps[-1][0]), c.want_paths, "%s: the step oracle's final states against the path oracle" % name)
    return c


# ---- 1. the trace kernel: 24 instantiations ---------------------------------------------------------------------------------

_TRACE = {}
TRACE_SCENES = {"demo": FETCHES, "glass": FETCHES, "seeds": (R.FETCH_LDS,), "prisms": (R.FETCH_LDS,), "random-6000": FETCHES}
TRACE_N = 1 << 12


def _trace_case(name):
    if name not in _TRACE:
        if name == "demo":
            objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
        elif name == "glass":
            objs, cam = R.builtin_scene_desc(R.SCENE_GLASS_STRESS)
        elif name == "seeds":
            objs, cam = R.builtin_scene_desc(R.SCENE_DEMO, 1500)
        elif name == "prisms":
            objs, cam = RS.random_scene(77, n_spheres=3000, n_prisms=48, n_planes=2, n_circles=3, n_parabs=1)
        else:
            objs, cam = RS.random_scene(41, n_spheres=6000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1)
        oscene = O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
        want, segs = oscene.render(W, H, 4, 2, 77, TRACE_N, threads=16)
        assert (want["probability"] != 0).sum() >= 20
        _TRACE[name] = (R.Scene(objs, cam), want, segs)
    return _TRACE[name]


@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", list(TRACE_SCENES))
def test_trace_kernel_every_instantiation_on_poisoned_lds(name, pattern):
    """rl_trace_kernel<stage, fused, open, cyl> on 4,096 paths: un-fused, the photons byte for byte; fused, the film by the film
    tests' tolerance; the segment count exactly; and rl_debug_variant_launches names the instantiation that ran."""
    scene, want, segs = _trace_case(name)
    seed, stream, first = 4, 2, 77
    cyl = int(name in ("glass", "prisms"))
    for fetch in TRACE_SCENES[name]:
        for fused in (False, True):
            for open_launch in (False, True):
                what = "%s pattern %s fetch %d %s %s" % (name, _pid(pattern), fetch, "fused" if fused else "unfused", "open" if open_launch else "plain")
                t = R.TraceUnit(0, W, H, n_photons=TRACE_N)
                t.set_fetch(fetch)
                p = R.PlotUnit(0, W, H) if fused else None
                if p is not None:
                    p.sync()
                before = R.variant_launches()
                LP.poison_lds(pattern)
                if not fused:
                    if open_launch:
                        t.render(scene, seed=seed, stream=stream, first_path_index=first)
                    else:
                        t.render_async(scene, seed=seed, stream=stream, first_path_index=first)
                        t.sync()
                    got = t.mapped_photons
                    if got.tobytes() != want.tobytes():
                        rows = np.flatnonzero(got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4))
                        raise AssertionError("%s: photons differ, first path %d: got %r want %r" % (what, rows[0] // 4, got[rows[0] // 4], want[rows[0] // 4]))
                else:
                    if open_launch:
                        t.render_fused_sync(scene, p, TRACE_N, seed=seed, stream=stream, first_path_index=first)
                    else:
                        t.render_fused(scene, p, TRACE_N, seed=seed, stream=stream, first_path_index=first)
                        t.sync()
                    assert_film(p.tristimulus_buffer, W, H, want, what)
                assert t.stats()[:2] == (TRACE_N, segs), (what, t.stats()[:2], segs)
                v = B._variant_of(R.variant_launches, before)
                low = (4 if fused else 0) | (2 if open_launch else 0) | cyl
                if name == "random-6000":                # a third level: never the whole scene; the tables where they fit
                    assert v in (low, 16 | low) and (fetch == R.FETCH_LDS or v == low), (what, v)
                else:
                    stage = 0 if fetch == R.FETCH_GLOBAL else (16 if name in ("seeds", "prisms") else 8)
                    assert v == stage | low, (what, v)
                _ran["trace"].add(v)


# ---- 2. query and occlusion -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", SCENES)
def test_query_on_poisoned_lds_and_in_another_order(name, pattern):
    c = _case(name)
    for fetch in FETCHES:
        for t, want, tag in ((np.full(N, np.inf, np.float32), c.hits_inf, "t_max inf"), (c.t, c.hits_t, "t_max cases")):
            what = "%s pattern %s fetch %d %s" % (name, _pid(pattern), fetch, tag)
            before = R.query_launches()
            LP.poison_lds(pattern)
            got = c.scene.intersect(c.o, c.d, t, fetch=fetch)
            v = B._variant_of(R.query_launches, before)
            _check_variant(v, c.cyl, fetch, what)
            _ran["query"].add(v)
            assert_same(got, want, what)
            LP.poison_lds(pattern)
            again = c.scene.intersect(c.o[PERM], c.d[PERM], t[PERM], fetch=fetch)
            assert_same(again, got[PERM], what + ", permuted")


@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", SCENES)
def test_occlusion_on_poisoned_lds_and_in_another_order(name, pattern):
    c = _case(name)
    for fetch in FETCHES:
        for t, want, tag in ((np.full(N, np.inf, np.float32), c.blocked_inf, "t_max inf"), (c.t, c.blocked_t, "t_max cases")):
            what = "%s pattern %s fetch %d %s" % (name, _pid(pattern), fetch, tag)
            before = R.occlusion_launches()
            LP.poison_lds(pattern)
            got = c.scene.occluded(c.o, c.d, t, fetch=fetch)
            v = B._variant_of(R.occlusion_launches, before)
            _check_variant(v, c.cyl, fetch, what)
            _ran["occlusion"].add(v)
            assert_same_bytes(got, want, what)
            LP.poison_lds(pattern)
            again = c.scene.occluded(c.o[PERM], c.d[PERM], t[PERM], fetch=fetch)
            assert_same_bytes(again, got[PERM], what + ", permuted")


# ---- 3. paths: camera_rays and render_rays ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", SCENES)
def test_paths_on_poisoned_lds(name, pattern):
    """rl_scene_camera_rays against the oracle's render (x, y, wavelength), its rays fed back to rl_scene_render_rays against
    the oracle's photon values and segments -- with every ninth wavelength made non-finite first -- and the case's arbitrary
    rays against the path oracle in every field, in two orders."""
    c = _path_case(name)
    LP.poison_lds(pattern)
    samples = c.scene.camera_rays(W, H, c.cam_seed, c.cam_stream, c.cam_first, N)
    assert samples["x"].tobytes() == c.cam_want["x"].tobytes() and samples["y"].tobytes() == c.cam_want["y"].tobytes(), (name, pattern)
    assert samples["ray"]["wavelength"].tobytes() == c.cam_want["wavelength"].tobytes()
    assert (samples["ray"]["reserved"] == 0).all() and (samples["reserved0"] == 0).all() and (samples["reserved1"] == 0).all()
    cam_rays = np.ascontiguousarray(samples["ray"])
    holes = cam_rays.copy()
    bad = np.arange(N) % 9 == 4
    holes["wavelength"][bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(bad.sum())) % 3]
    for fetch in FETCHES:
        what = "%s pattern %s fetch %d" % (name, _pid(pattern), fetch)
        before = R.path_launches()
        LP.poison_lds(pattern)
        res = c.scene.render_spectral_rays(cam_rays, c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch)
        v = B._variant_of(R.path_launches, before)
        _check_variant(v, c.cyl, fetch, what)
        _ran["path"].add(v)
        assert res["value"].tobytes() == c.cam_want["probability"].tobytes(), what
        assert int(res["segments"].sum(dtype=np.uint64)) == c.cam_segs, what
        assert_consistent(res)
        LP.poison_lds(pattern)
        holed = c.scene.render_spectral_rays(holes, c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch)
        want = res.copy()
        want[bad] = np.array([(0.0, 0, NONE, R.RL_PATH_END_INVALID)], dtype=R.PATH_RESULT_DTYPE)   # include/robigo_luculenta.h
        assert_same(holed, want, what + ", camera rays with non-finite wavelengths")
        LP.poison_lds(pattern)
        got = c.scene.render_spectral_rays(c.rays, c.seed, c.stream, c.first, fetch=fetch)
        assert_same(got, c.want_paths, what + ", arbitrary rays")
        LP.poison_lds(pattern)
        got = c.scene.render_spectral_rays(c.rays[PPERM], c.seed, c.stream, c.first, fetch=fetch)
        assert_same(got, c.want_paths_perm, what + ", arbitrary rays in another order (each ray another path index)")


# ---- 4. film: plot_photons and render_samples -------------------------------------------------------------------------------

def _samples_of(c):
    """The path case's rays as camera samples: screen positions all over the screen and just beyond it, one in sixteen not finite
    (traced, not splatted)."""
    rng = np.random.default_rng(zlib.crc32(("dirty film " + c.name).encode()))
    s = np.zeros(NP, R.CAMERA_SAMPLE_DTYPE)
    s["ray"] = c.rays
    s["x"] = rng.uniform(-1.005, 1.005, NP).astype(np.float32)
    s["y"] = (rng.uniform(-1.005, 1.005, NP) * H / W).astype(np.float32)
    odd = np.arange(NP) % 16 == 7
    s["x"][odd] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(odd.sum())) % 3]
    s["reserved0"], s["reserved1"] = 0xdeadbeef, 7      # ignored
    return s, ~odd


def _film_photons(samples, results):
    """The photons these samples and results put on a film: (x, y, value, wavelength) of the paths that were traced."""
    photons = _photons_of(samples, results)
    return photons[np.isfinite(photons["wavelength"])]   # (RL_PATH_END_INVALID: value 0, never splatted)


@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", SCENES)
def test_film_on_poisoned_lds(name, pattern):
    """rl_plot_unit_render_samples: the results are the path oracle's, the film is the oracle's plot of the photons those results
    make (both of tests/test_gpu_film.py's comparisons); with and without a results array."""
    c = _path_case(name)
    samples, splatted = _samples_of(c)
    photons = _film_photons(samples[splatted], c.want_paths[splatted])
    assert (photons["probability"] != 0).sum() >= 10
    for fetch in FETCHES:
        for results in (True, False):
            what = "%s pattern %s fetch %d results=%s" % (name, _pid(pattern), fetch, results)
            p = R.PlotUnit(0, W, H)
            p.sync()
            before = R.film_launches()
            LP.poison_lds(pattern)
            res = p.render_samples(c.scene, samples, c.seed, c.stream, c.first, fetch=fetch, results=results)
            v = B._variant_of(R.film_launches, before)
            assert v % 2 == c.cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
            _ran["film"].add(v)
            if results:
                assert_same(res, c.want_paths, what)
            assert_film(p.tristimulus_buffer, W, H, photons, what)


@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
def test_plot_photons_on_poisoned_lds(pattern):
    photons = synthetic_photons(W, H, 11, N)
    for form in ("host", "device"):
        p = R.PlotUnit(0, W, H)
        p.sync()
        db = _upload(photons)
        LP.poison_lds(pattern)
        if form == "host":
            p.plot_photons(photons)
        else:
            p.plot_photons_device(db)
        assert_film(p.tristimulus_buffer, W, H, photons, "plot_photons %s form, pattern %s" % (form, _pid(pattern)))


# ---- 5. step: begin and step until nothing is live --------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", PATTERNS, ids=_pid)
@pytest.mark.parametrize("name", SCENES)
def test_step_on_poisoned_lds_and_in_another_order(name, pattern):
    """begin_paths, then step_paths until nothing is live, LDS poisoned before every call: every field of every state and hit
    after every step is the step oracle's.  Then the same with the states shuffled before every step: a state's bytes do not
    depend on its place in the batch or on its wave companions (the path index travels with the record)."""
    c = _step_case(name)
    LP.poison_lds(pattern)
    begun = c.scene.begin_paths(c.rays, c.first)
    assert_same(begun, c.begun, "%s pattern %s: begin_paths" % (name, _pid(pattern)))
    assert (begun["end"] != LIVE).any()                  # states that are never live, from the first step on
    for fetch in FETCHES:
        what = "%s pattern %s fetch %d" % (name, _pid(pattern), fetch)
        st, hits = begun.copy(), _poison_hits(NP)
        for k, (want, want_hits) in enumerate(c.steps):
            before = R.step_launches()
            LP.poison_lds(pattern)
            c.scene.step_paths(st, c.seed, c.stream, fetch=fetch, hits=hits)
            v = B._variant_of(R.step_launches, before)
            _check_variant(v, c.cyl, fetch, what)
            _ran["step"].add(v)
            assert_same(st, want, "%s step %d: states" % (what, k))
            assert_same(hits, want_hits, "%s step %d: hits" % (what, k))
        assert (st["end"] != LIVE).all()
        rng = np.random.default_rng(len(name) + fetch)
        st = begun.copy()
        for k, (want, _) in enumerate(c.steps):
            st = np.ascontiguousarray(st[rng.permutation(NP)])
            LP.poison_lds(pattern)
            c.scene.step_paths(st, c.seed, c.stream, fetch=fetch)
            back = np.empty_like(st)
            back[(st["path_index"] - np.uint64(c.first)).astype(np.int64)] = st
            assert_same(back, want, "%s step %d: states, shuffled before every step" % (what, k))


# ---- 6. guarded, prefilled outputs of every _device form --------------------------------------------------------------------

_guarded = G.device_guarded


@pytest.mark.parametrize("n", BATCHES)
def test_guarded_intersect_device(n):
    c = _case("demo")
    rays = np.zeros(n, R.RAY_DTYPE)
    rays["origin"], rays["direction"], rays["t_max"], rays["reserved"] = c.o[:n], c.d[:n], c.t[:n], 0xdeadbeef
    for fetch in FETCHES:
        what = "rl_scene_intersect_device n=%d fetch %d" % (n, fetch)
        host = c.scene.intersect(c.o[:n], c.d[:n], c.t[:n], fetch=fetch)
        assert_same(host, c.hits_t[:n], what + ": host form against the oracle")   # (zero on a miss, reserved 0: the header's words)
        out = _guarded(n * 48)
        c.scene.intersect_device(_upload(rays), out, fetch=fetch)
        G.assert_written_as(out.payload(what, R.HIT_DTYPE), host, what)


@pytest.mark.parametrize("n", BATCHES)
def test_guarded_path_device_forms(n):
    """rl_scene_camera_rays_device (48-byte samples: reserved0, reserved1 written 0, and ray.reserved pinned to the host form's
    0) and rl_scene_render_rays_device (16-byte results), on the camera's rays with non-finite wavelengths mixed in."""
    c = _path_case("demo")
    host_samples = c.scene.camera_rays(W, H, c.cam_seed, c.cam_stream, c.cam_first, n)
    assert host_samples["x"].tobytes() == c.cam_want["x"][:n].tobytes() and host_samples["ray"]["wavelength"].tobytes() == c.cam_want["wavelength"][:n].tobytes()
    assert (host_samples["ray"]["reserved"] == 0).all() and (host_samples["reserved0"] == 0).all() and (host_samples["reserved1"] == 0).all()
    out = _guarded(n * 48)
    what = "rl_scene_camera_rays_device n=%d" % n
    c.scene.camera_rays_device(W, H, c.cam_seed, c.cam_stream, c.cam_first, out)
    G.assert_written_as(out.payload(what, R.CAMERA_SAMPLE_DTYPE), host_samples, what)
    rays = np.ascontiguousarray(host_samples["ray"])
    bad = np.arange(n) % 9 == 4
    rays["wavelength"][bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(bad.sum())) % 3]
    for fetch in FETCHES:
        what = "rl_scene_render_rays_device n=%d fetch %d" % (n, fetch)
        host = c.scene.render_spectral_rays(rays, c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch)
        assert host["value"][~bad].tobytes() == c.cam_want["probability"][:n][~bad].tobytes(), what
        assert (host["end"][bad] == R.RL_PATH_END_INVALID).all() and (host["value"][bad] == 0).all()
        out = _guarded(n * 16)
        c.scene.render_rays_device(_upload(rays), out, c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch)
        G.assert_written_as(out.payload(what, R.PATH_RESULT_DTYPE), host, what)


@pytest.mark.parametrize("n", BATCHES)
def test_guarded_begin_and_step_device(n):
    """rl_scene_begin_paths_device writes every byte of n 64-byte states (reserved 0); rl_scene_step_paths_device steps the live
    ones in place and leaves every byte of the others -- here a 0xC3 background with a non-live `end` -- and of their hits as it
    was, beside intact guards, for two steps."""
    c = _path_case("demo")
    rays = np.ascontiguousarray(c.scene.camera_rays(W, H, c.cam_seed, c.cam_stream, c.cam_first, n)["ray"])
    bad = np.arange(n) % 9 == 4
    rays["wavelength"][bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(bad.sum())) % 3]
    begun = c.scene.begin_paths(rays, c.cam_first)
    assert_same(begun, S.begin(rays, c.cam_first).view(R.PATH_STATE_DTYPE), "begin_paths, host form against its restatement")
    what = "rl_scene_begin_paths_device n=%d" % n
    out = _guarded(n * 64)
    assert out.data_ptr() % 16 == 0
    c.scene.begin_paths_device(_upload(rays), out, c.cam_first)
    G.assert_written_as(out.payload(what, R.PATH_STATE_DTYPE), begun, what)
    ends = np.array([LIVE, LIVE, R.RL_PATH_END_VOID, LIVE, R.RL_PATH_END_EMITTER, LIVE, R.RL_PATH_END_ROULETTE, R.RL_PATH_END_LIMIT, LIVE,
                     R.RL_PATH_END_INVALID, 7, 0xfffffffe], np.uint32)[(np.arange(n) + (n > 1)) % 12]
    start = begun.copy()
    dead = (ends != LIVE) | (start["end"] != LIVE)
    raw = start.view(np.uint8).reshape(n, 64)
    raw[ends != LIVE] = 0xC3
    start["end"][ends != LIVE] = ends[ends != LIVE]
    for fetch in FETCHES:
        what = "rl_scene_step_paths_device n=%d fetch %d" % (n, fetch)
        host, host_hits = start.copy(), np.frombuffer(bytes([G.FILL]) * (48 * n), dtype=R.HIT_DTYPE).copy()
        sb, hb = _guarded(initial=start), _guarded(n * 48)
        for step in range(2):
            was = host.copy()
            c.scene.step_paths(host, c.cam_seed, c.cam_stream, fetch=fetch, hits=host_hits)
            c.scene.step_paths_device(sb, c.cam_seed, c.cam_stream, fetch=fetch, hits=hb)
            got, got_hits = sb.payload(what, R.PATH_STATE_DTYPE), hb.payload(what + ": hits", R.HIT_DTYPE)
            G.assert_written_as(got, host, "%s step %d" % (what, step))
            G.assert_written_as(got_hits, host_hits, "%s step %d: hits" % (what, step))
            idle = was["end"] != LIVE
            assert got[idle].tobytes() == was[idle].tobytes(), what           # not live: every byte as it was
            assert (got["reserved"][~idle] == 0).all() and (got_hits["reserved"][~idle] == 0).all()
        assert got[dead].tobytes() == start[dead].tobytes()
        assert (got_hits[dead].view(np.uint8) == G.FILL).all()
        if n >= 63:
            assert dead.any() and (~dead).any() and (got["segments"][~dead] >= 1).all()


class _GuardedFilm:
    """A plot unit whose tristimulus buffer is caller-owned device memory between two guards (rl_plot_unit_create: external_xyz)."""

    def __init__(self, w, h, image):
        self.mem = _guarded(initial=np.ascontiguousarray(image, dtype=np.float32).reshape(h * w, 3))
        self.unit = R.PlotUnit(0, w, h, external_xyz=self.mem.data_ptr())

    def image(self, what):
        self.unit.sync()
        got = self.mem.payload(what, np.float32).reshape(-1, 3)
        self.unit.close()                                # (before the memory it does not own goes away)
        return got


def _background(w, h):
    """Non-zero, NaN-free, of both signs and many magnitudes."""
    rng = np.random.default_rng(w * h)
    return (rng.normal(0, 1, (h * w, 3)) * np.exp(rng.uniform(-20, 20, (h * w, 1)))).astype(np.float32) + np.float32(1e-30)


@pytest.mark.parametrize("n", BATCHES)
def test_guarded_film_device_forms(n):
    """rl_plot_unit_plot_photons_device and rl_plot_unit_render_samples_device: the results array guarded as above; the film --
    caller-owned memory between guards -- is the oracle's plot and nothing outside width x height x 3 floats is written, although
    photons lie on and beyond every border; and a unit that gets no valid photon or sample keeps its buffer, uploaded as a
    non-zero pattern, bit for bit."""
    c = _path_case("demo")
    photons = synthetic_photons(W, H, 13, max(n, 8))[:n]
    what = "rl_plot_unit_plot_photons_device n=%d" % n
    film = _GuardedFilm(W, H, np.zeros((H * W, 3), np.float32))
    film.unit.plot_photons_device(_upload(photons))
    assert_film(film.image(what), W, H, photons, what)
    samples = c.scene.camera_rays(W, H, c.cam_seed, c.cam_stream, c.cam_first, n)
    edge = np.arange(n) % 5 == 2                         # on and just beyond the borders
    samples["x"][edge] = np.array([-1.0, 1.0, -1.004, 1.004], np.float32)[np.arange(int(edge.sum())) % 4]
    samples["y"][edge] = (np.array([1.0, -1.0, 1.004, -1.004, 0.3], np.float32)[np.arange(int(edge.sum())) % 5] * np.float32(H) / np.float32(W)).astype(np.float32)
    bad = np.arange(n) % 9 == 4
    samples["ray"]["wavelength"][bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(int(bad.sum())) % 3]
    background = _background(W, H)
    for fetch in FETCHES:
        what = "rl_plot_unit_render_samples_device n=%d fetch %d" % (n, fetch)
        host_unit = R.PlotUnit(1, W, H)
        host = host_unit.render_samples(c.scene, samples, c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch)
        assert host["value"][~bad].tobytes() == c.cam_want["probability"][:n][~bad].tobytes(), what
        assert (host["end"][bad] == R.RL_PATH_END_INVALID).all()
        film, out = _GuardedFilm(W, H, np.zeros((H * W, 3), np.float32)), _guarded(n * 16)
        film.unit.render_samples_device(c.scene, _upload(samples), c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch, results=out)
        G.assert_written_as(out.payload(what, R.PATH_RESULT_DTYPE), host, what)
        assert_film(film.image(what), W, H, _film_photons(samples, host), what)
        # nothing valid: wavelengths that are not finite (no path), and photons without a finite position or with probability 0
        nothing = samples.copy()
        nothing["ray"]["wavelength"] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(n) % 3]
        film, out = _GuardedFilm(W, H, background), _guarded(n * 16)
        film.unit.render_samples_device(c.scene, _upload(nothing), c.cam_seed, c.cam_stream, c.cam_first, fetch=fetch, results=out)
        res = out.payload(what + ", nothing valid", R.PATH_RESULT_DTYPE)
        assert (res["end"] == R.RL_PATH_END_INVALID).all() and (res["value"] == 0).all() and (res["segments"] == 0).all() and (res["object"] == NONE).all()
        assert film.image(what).tobytes() == background.tobytes(), what + ": a unit without a valid sample was written"
    dud = synthetic_photons(W, H, 14, max(n, 8))[:n]
    dud["x"][0::2] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(dud["x"][0::2])) % 3]
    dud["probability"][1::2] = 0.0
    film = _GuardedFilm(W, H, background)
    film.unit.plot_photons_device(_upload(dud))
    assert film.image("plot_photons_device, nothing valid").tobytes() == background.tobytes()


# ---- 7. what ran ------------------------------------------------------------------------------------------------------------

def test_every_variant_ran_on_poisoned_lds():
    """All 24 instantiations of the trace kernel and every variant of the five other families ran with the LDS poisoned in this
    module's run (the tests above record what rl_debug_*_launches reported after each poisoned launch)."""
    if _wall["start"]:
        print("tests/test_gpu_dirty_state.py: %.0f s from the control test to here" % (time.time() - _wall["start"]))
    assert _ran["trace"] == set(range(24)), sorted(set(range(24)) - _ran["trace"])
    for family in ("query", "occlusion", "path", "film", "step"):
        assert _ran[family] == set(range(6)), (family, sorted(_ran[family]))
