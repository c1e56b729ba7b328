"""Every ray kernel at the full width of its RNG coordinates (tests/_rng_width.py): seeds with a high word, streams with bit 31
set, path ranges that carry from the low into the high counter word inside one launch, caller-held states whose 64 lanes share
no high word and whose words are float NaN, -0 and infinity patterns, and `segments` at the edges of 32 bits.  The chain is numpy
Philox -> CPU oracle (tests/test_rng_width.py) -> the device, here: the trace kernel's photons byte for byte in every launch
kind; the camera, path, step, list-step, film and light calls against the oracles their own modules hold them to; one plain fused
launch of more than 2^32 paths by its exact counters.  A GPU fault ends the run: nothing here provokes one."""
import numpy as np
import pytest

import _guarded as G
import _light_film_oracle as FO
import _light_oracle as LO
import _oracle as O
import _path_list_oracle as L
import _path_oracle as P
import _rng_width as RW
import _step_oracle as S
from _boundary import _ocam, _variant_of
from _compare import assert_film, assert_same
from _device_arrays import _Device, _Words, _begin_device, _poison_hits, _prefilled
from _scenes import _lit_scene, _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

LIVE = R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
FETCH_IDS = ["lds", "global"]
W, H, N, NQ = RW.W, RW.H, RW.N_TRACE, RW.N_QUERY
FILL32 = 0xAAAAAAAA
DEVICE_FORM_CASES = ("carry-mid-wave", "top")
# (case, fetch, device form): the host forms on every case, the _device forms on two
QUERY_PARAMS = [pytest.param(c, f, False, id="%s-%s-host" % (c.id, FETCH_IDS[f])) for c in RW.CASES for f in FETCHES] + \
               [pytest.param(RW.BY_ID[i], f, True, id="%s-%s-device" % (i, FETCH_IDS[f])) for i in DEVICE_FORM_CASES for f in FETCHES]

_cache = {}


def _once(key, make):
    """What `make` returns, computed once per key and shared, never written to by a test."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _scenes(name, lit=False):
    """(objects, camera, the device's scene, the oracle's scene) of scene `name`."""
    def make():
        objs, cam = _lit_scene(name) if lit else _scene(name)
        objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)
        return objs, cam, R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))
    return _once(("scene", name, lit), make)


def _oracle_photons(name, case, n=N):
    """(photons, segments) of the CPU oracle for the case's n paths on scene `name`."""
    return _once(("photons", name, case.id, n), lambda: _scenes(name)[3].render(W, H, case.seed, case.stream, case.first, n, threads=16))


# ---- a. the trace kernel ---------------------------------------------------------------------------------------------------------

TRACE_SCENES = [("demo", R.FETCH_LDS, 8), ("demo", R.FETCH_GLOBAL, 0), ("tables-prisms", R.FETCH_LDS, 16 | 1)]
LAUNCH_KINDS = ["render", "render_async", "render_fused_sync", "render_fused"]


def _assert_photons(got, want, what):
    """Byte for byte; the message says whether the photons that differ ended on an emitter: those are written by the kernel's
    process_emitted from first + idx, the others from the draws rl_begin_path made for the path."""
    if got.tobytes() == want.tobytes():
        return
    differs = got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero(differs.any(axis=1))
    lit = want["probability"][bad] != 0
    fields = [f for k, f in enumerate(want.dtype.names) if differs[:, k].any()]
    raise AssertionError("%s: %d of %d photons differ (fields %s), first %d: got %r want %r; %d of them ended on an emitter (the record "
                         "process_emitted re-derives from first + idx), %d did not (the draws of rl_begin_path)"
                         % (what, len(bad), len(want), fields, bad[0], got[bad[0]], want[bad[0]], int(lit.sum()), int((~lit).sum())))


@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
@pytest.mark.parametrize("kind", LAUNCH_KINDS)
@pytest.mark.parametrize("name, fetch, base", TRACE_SCENES, ids=["demo-lds", "demo-global", "tables-prisms"])
def test_trace_kernel_in_every_launch_kind(name, fetch, base, kind, case):
    _, _, scene, _ = _scenes(name)
    want, segs = _oracle_photons(name, case)
    assert (want["probability"] != 0).sum() > (20 if name == "demo" else 0)   # both of the kernel's ways to write a record are exercised
    fused, open_launch = "fused" in kind, kind in ("render", "render_fused_sync")
    t = R.TraceUnit(0, W, H, n_photons=N)
    if fetch != R.FETCH_LDS:
        t.set_fetch(fetch)
    kw = dict(seed=case.seed, stream=case.stream, first_path_index=case.first)
    what = "%s %s %s" % (name, kind, case.id)
    before = R.variant_launches()
    if not fused:
        if open_launch:
            t.render(scene, **kw)                          # blocking: appended to an open launch
        else:
            t.render_async(scene, **kw)                    # one plain launch
            t.sync()
        _assert_photons(t.mapped_photons, want, what)
    else:
        p = R.PlotUnit(0, W, H)
        if open_launch:
            t.render_fused_sync(scene, p, N, **kw)
        else:
            t.render_fused(scene, p, N, **kw)
            t.sync()
        assert_film(p.tristimulus_buffer, W, H, want, what)
    assert _variant_of(R.variant_launches, before) == (base | (4 if fused else 0) | (2 if open_launch else 0)), what
    assert t.stats()[:2] == (N, segs), what


# ---- b. the query-style calls on the demo scene --------------------------------------------------------------------------------

def _paths(case):
    """What the query tests of one case share: the device's camera samples (held to numpy by the camera test), the oracle's photons
    and segment total for these NQ paths, _path_oracle's results for the rays, and the oracle's listed loop from the identity
    list: (states, hits, survivors) after every step."""
    def make():
        objs, cam, scene, _ = _scenes("demo")
        camera = scene.camera_rays(W, H, case.seed, case.stream, case.first, NQ)
        rays = np.ascontiguousarray(camera["ray"])
        photons, segs = _oracle_photons("demo", case, NQ)
        results = P.PathOracle(objs, cam).render_rays(rays["origin"], rays["direction"], rays["wavelength"], case.seed, case.stream,
                                                      case.first).view(R.PATH_RESULT_DTYPE)
        so = S.StepOracle(objs, cam)
        st, hits, live, turns = S.begin(rays, case.first), _poison_hits(NQ), None, []
        while live is None or len(live):
            assert len(turns) < R.RL_PATH_MAX_SEGMENTS
            live = L.step_list(so, st, case.seed, case.stream, list=live, hits=hits)
            turns.append((st.copy().view(R.PATH_STATE_DTYPE), hits.copy(), live.copy()))
        return {"camera": camera, "rays": rays, "photons": photons, "segments": segs, "results": results, "turns": turns}
    return _once(("paths", case.id), make)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_camera_rays_are_the_numpy_draws_and_the_trace_kernels(case):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    camera = q["camera"]
    x, y, wavelength = RW.numpy_camera(case.seed, case.stream, case.first, NQ)
    for name, got, want in (("x", camera["x"], x), ("y", camera["y"], y), ("wavelength", camera["ray"]["wavelength"], wavelength)):
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert not len(bad), (case.id, name, len(bad), bad[:4])
    t = R.TraceUnit(0, W, H, n_photons=NQ)
    t.render(scene, seed=case.seed, stream=case.stream, first_path_index=case.first)
    ph = t.mapped_photons
    _assert_photons(ph, q["photons"], case.id)
    assert ph["x"].tobytes() == camera["x"].tobytes() and ph["y"].tobytes() == camera["y"].tobytes()
    assert ph["wavelength"].tobytes() == np.ascontiguousarray(camera["ray"]["wavelength"]).tobytes()
    if case.id in DEVICE_FORM_CASES:
        poison = np.frombuffer(bytes([G.FILL]) * (48 * NQ), dtype=R.CAMERA_SAMPLE_DTYPE).copy()
        cb = _Device(poison)
        scene.camera_rays_device(W, H, case.seed, case.stream, case.first, cb.buf)
        assert_same(cb.get()[:NQ], camera, case.id + ": device form")


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_render_rays_is_the_photons_probability_and_the_path_oracle(case, fetch, device):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    before = R.path_launches()
    if device:
        poison = np.zeros(NQ, R.PATH_RESULT_DTYPE)
        poison["end"] = 12345
        rb, ob = _Device(q["rays"]), _Device(poison)
        R.check(R.lib.rl_scene_render_rays_device(scene.handle, fetch, case.seed, case.stream, case.first, 0, rb.buf.data_ptr(), NQ, ob.buf.data_ptr()))
        got = ob.get()
    else:
        got = scene.render_spectral_rays(q["rays"], case.seed, case.stream, case.first, fetch=fetch)
    assert _variant_of(R.path_launches, before) == (4 if fetch == R.FETCH_LDS else 0)
    # the header's Identity: the value of camera ray i as path first + i is photon i's probability
    assert got["value"].tobytes() == q["photons"]["probability"].tobytes(), case.id
    assert int(got["segments"].sum(dtype=np.uint64)) == q["segments"]
    assert_same(got, q["results"], "%s fetch %d: against the path oracle" % (case.id, fetch))


def _begin(scene, q, case, device):
    if device:
        return _begin_device(scene, q["rays"], case.first)
    return scene.begin_paths(q["rays"], case.first)


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_begin_and_the_step_loop_are_the_step_oracle(case, fetch, device):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    sb = _begin(scene, q, case, device)
    begun = sb.get() if device else sb
    assert (begun["path_index"] == RW.paths_of(case.first, NQ)).all(), case.id      # first + i across the carry
    assert begun.tobytes() == S.begin(q["rays"], case.first).tobytes()
    hb = _Device(_poison_hits(NQ)) if device else _poison_hits(NQ)
    before = R.step_launches()
    for k, (wst, whits, _) in enumerate(q["turns"]):
        what = "%s fetch %d step %d" % (case.id, fetch, k)
        if device:
            scene.step_paths_device(sb.buf, case.seed, case.stream, fetch=fetch, hits=hb.buf)
            st, hits = sb.get(), hb.get()
        else:
            st, hits = scene.step_paths(sb, case.seed, case.stream, fetch=fetch, hits=hb), hb
        assert_same(st, wst, what + ": states")
        assert_same(hits, whits, what + ": hits")
    assert _variant_of(R.step_launches, before) == (4 if fetch == R.FETCH_LDS else 0)
    assert (st["end"] != LIVE).all() and (st["path_index"] == RW.paths_of(case.first, NQ)).all()


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_the_listed_loop_from_a_permuted_list_is_the_oracle(case, fetch, device):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    lst = np.random.default_rng(NQ).permutation(NQ).astype(np.uint32)
    sb = _begin(scene, q, case, device)
    hb = _Device(_poison_hits(NQ)) if device else _poison_hits(NQ)
    ping, pong = (_Words(lst), _Words(np.full(NQ, FILL32))) if device else (None, None)
    n_list = NQ
    before = R.path_list_launches()
    for k, (wst, whits, _) in enumerate(q["turns"]):
        what = "%s fetch %d step %d" % (case.id, fetch, k)
        assert n_list, what
        want_live = lst[:n_list][wst["end"][lst[:n_list]] == LIVE]      # stable: the survivors in the list's order
        if device:
            n_live = scene.step_path_list_device(sb.buf, case.seed, case.stream, ping.buf, n_list, pong.buf, fetch=fetch, hits=hb.buf)
            st, hits, live = sb.get(), hb.get(), pong.get()[:n_live].copy()
            ping, pong = pong, ping
        else:
            live = scene.step_path_list(sb, case.seed, case.stream, list=lst, n_list=n_list, fetch=fetch, hits=hb)
            st, hits = sb, hb
        assert_same(st, wst, what + ": states")
        assert_same(hits, whits, what + ": hits")
        assert live.tolist() == want_live.tolist(), what
        lst, n_list = live, len(live)
    assert n_list == 0
    assert _variant_of(R.path_list_launches, before) == (4 if fetch == R.FETCH_LDS else 0)


def _poisoned_results():
    res = np.zeros(NQ, R.PATH_RESULT_DTYPE)
    res["end"] = 12345
    return res


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_render_samples_gives_the_results_and_the_film_of_the_photons(case, fetch, device):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    p = R.PlotUnit(0, W, H)
    before = R.film_launches()
    if device:
        cb, rb = _Device(q["camera"]), _Device(_poisoned_results())
        p.render_samples_device(scene, cb.buf, case.seed, case.stream, case.first, fetch=fetch, results=rb.buf)
        got = rb.get()
    else:
        got = p.render_samples(scene, q["camera"], case.seed, case.stream, case.first, fetch=fetch)
    assert _variant_of(R.film_launches, before) == (4 if fetch == R.FETCH_LDS else 0)
    assert_same(got, q["results"], "%s fetch %d" % (case.id, fetch))
    assert_film(p.tristimulus_buffer, W, H, q["photons"], "%s fetch %d" % (case.id, fetch))


def _direct_photons(case):
    """The photons of rl_plot_unit_render_samples_direct's film as its contract states it, from the oracles alone: per step of the
    oracle's listed loop, _light_oracle's samples for the listed states and the rule of tests/_light_film_oracle.py."""
    def make():
        objs, cam, scene, _ = _scenes("demo")
        q = _paths(case)
        occ = LO.Occluder(objs, cam)
        emitters = LO.emitters(objs.view(O.OBJECT_DTYPE))
        sampled, lst, photons = np.zeros(NQ, np.uint8), None, []
        for wst, whits, live in q["turns"]:
            n_list = NQ if lst is None else len(lst)
            samples = LO.light_paths(occ, wst.view(S.STATE_DTYPE), whits, case.seed, case.stream, list=lst, n_list=n_list,
                                     samples=_prefilled(NQ).view(LO.SAMPLE_DTYPE))
            of_step, sampled = FO.film_photons(wst, samples, emitters, q["camera"], sampled, lst, n_list)
            photons.append(of_step)
            lst = live
        return np.concatenate(photons)
    return _once(("direct", case.id), make)


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_render_samples_direct_gives_the_results_and_the_film_of_the_oracles_loop(case, fetch, device):
    _, _, scene, _ = _scenes("demo")
    q = _paths(case)
    photons = _direct_photons(case)
    assert len(photons) > 20
    p = R.PlotUnit(0, W, H)
    before = R.light_film_launches()
    if device:
        cb, rb = _Device(q["camera"]), _Device(_poisoned_results())
        p.render_samples_direct_device(scene, cb.buf, case.seed, case.stream, case.first, fetch=fetch, results=rb.buf)
        got = rb.get()
    else:
        got = p.render_samples_direct(scene, q["camera"], case.seed, case.stream, case.first, fetch=fetch)
    ran = {i for i, (a, b) in enumerate(zip(R.light_film_launches(), before)) if a != b}
    assert ran == {4 if fetch == R.FETCH_LDS else 0}, ran
    assert_same(got, q["results"], "%s fetch %d" % (case.id, fetch))
    assert_film(p.tristimulus_buffer, W, H, photons, "%s fetch %d" % (case.id, fetch))


def _light_calls(scene, st, hits, camera, seed, stream, fetch, device, what, want, emitters, film=(W, H)):
    """rl_scene_light_paths* and rl_plot_unit_light_paths* for whole arrays: the samples of both are `want` byte for byte, the film
    is the rule's photons, the `sampled` bytes are the rule's; one launch each, of the variant returned."""
    n = len(st)
    w, h = film
    photons, after = FO.film_photons(st, want, emitters, camera, np.zeros(n, np.uint8))
    plot = R.PlotUnit(0, w, h)
    before, before_film = R.light_launches(), R.light_film_launches()
    if device:
        sb, hb, cb = _Device(st), _Device(hits), _Device(camera)
        mb, fb, yb = _Device(_prefilled(n)), _Device(_prefilled(n)), _Device(np.zeros(n, np.uint8))
        scene.light_paths_device(sb.buf, hb.buf, mb.buf, seed, stream, fetch=fetch)
        v = _variant_of(R.light_launches, before)
        plot.light_paths_device(scene, sb.buf, hb.buf, cb.buf, seed, stream, fetch=fetch, sampled=yb.buf, samples=fb.buf)
        got, got_film, got_bytes = mb.get(), fb.get(), yb.get()
        assert sb.get().tobytes() == st.tobytes() and hb.get().tobytes() == hits.tobytes()
    else:
        got = scene.light_paths(st, hits, seed, stream, fetch=fetch, samples=_prefilled(n))
        v = _variant_of(R.light_launches, before)
        got_bytes = np.zeros(n, np.uint8)
        got_film = plot.light_paths(scene, st, hits, camera, seed, stream, fetch=fetch, sampled=got_bytes, samples=_prefilled(n))
    assert _variant_of(R.light_film_launches, before_film) == v, what
    assert_same(got, want.view(R.LIGHT_SAMPLE_DTYPE), what + ": rl_scene_light_paths against the light oracle")
    assert_same(got_film, got, what + ": rl_plot_unit_light_paths' samples against rl_scene_light_paths'")
    assert got_bytes.tobytes() == after.tobytes(), what
    assert_film(plot.tristimulus_buffer, w, h, photons, what)
    return v


@pytest.mark.parametrize("case, fetch, device", QUERY_PARAMS)
def test_light_calls_at_the_first_vertex_are_the_light_oracle(case, fetch, device):
    objs, cam, scene, _ = _scenes("demo")
    q = _paths(case)
    st, hits, _ = q["turns"][0]
    want = _once(("light", case.id), lambda: LO.light_paths(LO.Occluder(objs, cam), st.view(S.STATE_DTYPE), hits, case.seed, case.stream,
                                                            samples=_prefilled(NQ).view(LO.SAMPLE_DTYPE)))
    assert (want["status"] == LO.VISIBLE).sum() > 20 and (want["status"] == LO.SKIPPED).sum() > 20
    v = _light_calls(scene, st, hits, q["camera"], case.seed, case.stream, fetch, device, "%s fetch %d" % (case.id, fetch), want,
                     LO.emitters(objs.view(O.OBJECT_DTYPE)))
    assert v == (4 if fetch == R.FETCH_LDS else 0)


def test_host_form_adds_the_chunks_offset_to_the_first_path_index_across_the_carry():
    """The host forms stage in chunks of 2^20 records and add `first_path_index + first` per chunk: rl_scene_render_rays on
    2^20 + 4097 rays whose range carries into the high word inside the second chunk, against the _device form's bytes."""
    case = RW.BY_ID["carry-mid-wave"]
    n = (1 << 20) + 4097
    first = (1 << 32) - (1 << 20) - 2081
    at = (1 << 32) - first
    assert 1 << 20 < at < n and at % 64 == 33
    _, _, scene, _ = _scenes("demo")
    rays = np.ascontiguousarray(scene.camera_rays(W, H, case.seed, case.stream, first, n)["ray"])
    host = scene.render_spectral_rays(rays, case.seed, case.stream, first)
    poison = np.zeros(n, R.PATH_RESULT_DTYPE)
    poison["end"] = 12345
    rb, ob = _Device(rays), _Device(poison)
    R.check(R.lib.rl_scene_render_rays_device(scene.handle, R.FETCH_LDS, case.seed, case.stream, first, 0, rb.buf.data_ptr(), n, ob.buf.data_ptr()))
    assert_same(host, ob.get(), "host form against the device form")
    assert (host["value"] != 0).mean() > 0.05
    # the tail of this range is the head of the case's own, which the tests above hold to the oracle
    off = case.first - first
    assert off + NQ <= n
    assert_same(host[off:off + NQ], _paths(case)["results"], "the rays from path 2^32 - 2081 on")


# ---- c. one plain fused launch of more than 2^32 paths ---------------------------------------------------------------------------

def test_one_plain_fused_launch_of_more_than_2_32_paths_traces_every_path_once():
    """Only with more than 2^32 paths in one plain launch is the high half of the kernel's queue offset ever non-zero.  Three
    launches from F = 2^33 + 12345: W1 = [F, F + 2^32 - 2^16), W2 = [F, F + 2^32 + 2^16), B = [F + 2^32 - 2^16, F + 2^32 + 2^16).
    W2's paths are W1's and B's, disjoint: the integer counters must add up exactly.  A path traced twice, skipped or drawn at
    another index shifts the segment total."""
    _, _, scene, _ = _scenes("demo")
    seed, stream, F = 0xA5A5A5A500000007, 1, (1 << 33) + 12345
    w, h = 1920, 1080
    t, p = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
    launches = {"W1": (F, (1 << 32) - (1 << 16)), "W2": (F, (1 << 32) + (1 << 16)), "B": (F + (1 << 32) - (1 << 16), 1 << 17)}
    got, last = {}, (0, 0, 0.0)
    for name, (first, n) in launches.items():
        t.render_fused(scene, p, n, seed=seed, stream=stream, first_path_index=first)
        t.sync()
        now = t.stats()
        got[name] = (now[0] - last[0], now[1] - last[1])
        print("%s: %d paths from %d: %d segments, kernel_ms %.3f" % (name, n, first, got[name][1], now[2] - last[2]))
        last = now
        assert got[name][0] == n, (name, got[name])
    assert got["W2"][0] - got["W1"][0] == 1 << 17 == got["B"][0]
    assert got["W2"][1] - got["W1"][1] == got["B"][1], got
    assert got["B"][1] > 1 << 17 and np.isfinite(p.tristimulus_buffer).all()


# ---- d, e. caller-held states: per-lane path indices, `segments` at the edges ----------------------------------------------------

# whole scene / tables only, without and with the prisms' second bound: with the global fetch of each, all six variants
STATE_SCENES = [("demo", 2, 0), ("many-prisms", 2, 1), ("demo-2500", 1, 0), ("tables-prisms", 1, 1)]
STATE_KINDS = ["path-index", "segments"]


def _vertex_states(name):
    """(camera samples, states, hits) of the NQ paths of carry-mid-wave on scene `name` after one step by the step oracle."""
    def make():
        case = RW.BY_ID["carry-mid-wave"]
        objs, cam, scene, _ = _scenes(name, lit=True)
        camera = scene.camera_rays(W, H, case.seed, case.stream, case.first, NQ)
        st, hits = S.begin(np.ascontiguousarray(camera["ray"]), case.first), np.zeros(NQ, S.HIT_DTYPE)
        hits["object"] = R.RL_OBJECT_NONE
        S.StepOracle(objs, cam).step(st, case.seed, case.stream, hits=hits)
        return camera, st, hits
    return _once(("vertex", name), make)


def _held_states(name, kind):
    """The vertex states with what a caller may have made of them: `path-index`, a mixture no begin makes, or `segments`, the edges
    of 32 bits.  With the oracles' answers for one more step of a hostile list, for a step of all, and for the light sample."""
    def make():
        case = RW.BY_ID["carry-mid-wave"]
        objs, cam, _, _ = _scenes(name, lit=True)
        camera, st, hits = _vertex_states(name)
        st, hits = st.copy(), hits.copy()
        if kind == "path-index":
            st["path_index"] = RW.mixed_path_indices(NQ)
            for wave in range(NQ // 64):
                assert len(set((st["path_index"][64 * wave:64 * wave + 64] >> np.uint64(32)).tolist())) > 32   # no wave shares a high word
        else:
            st["segments"] = RW.edge_segments(NQ)
        so = S.StepOracle(objs, cam)
        rng = np.random.default_rng(NQ + len(name))
        left_out = np.arange(NQ) % 3 == 1
        wild = np.concatenate([[NQ, NQ + 1, 0xffffffff, 0x80000000, 0xfffffffe, NQ + 63, NQ + 64], rng.integers(NQ, 1 << 32, 200)]).astype(np.uint32)
        lst = np.concatenate([np.flatnonzero(~left_out).astype(np.uint32), wild])
        lst = lst[rng.permutation(len(lst))]
        out = {"camera": camera, "states": st.view(R.PATH_STATE_DTYPE), "hits": hits, "list": lst, "left_out": left_out}
        for flags in (0, R.RL_STEP_NO_ROULETTE):
            all_st, all_hits = st.copy(), _poison_hits(NQ)
            so.step(all_st, case.seed, case.stream, flags, hits=all_hits)
            listed_st, listed_hits = st.copy(), _poison_hits(NQ)
            live = L.step_list(so, listed_st, case.seed, case.stream, list=lst, flags=flags, hits=listed_hits)
            # the oracle's two answers agree where the list names a state
            assert listed_st[~left_out].tobytes() == all_st[~left_out].tobytes() and listed_st[left_out].tobytes() == st[left_out].tobytes()
            out[flags] = (all_st.view(R.PATH_STATE_DTYPE), all_hits, listed_st.view(R.PATH_STATE_DTYPE), listed_hits, live)
        at_vertex = np.flatnonzero(st["segments"] >= 1)        # the light contract: a vertex is reached with a segment
        out["lit"] = at_vertex
        sub, sub_hits = np.ascontiguousarray(st[at_vertex]), np.ascontiguousarray(hits[at_vertex])
        out["samples"] = LO.light_paths(LO.Occluder(objs, cam), sub, sub_hits, case.seed, case.stream,
                                        samples=_prefilled(len(sub)).view(LO.SAMPLE_DTYPE))
        return out
    return _once(("held", name, kind), make)


@pytest.mark.parametrize("fetch", FETCHES, ids=FETCH_IDS)
@pytest.mark.parametrize("kind", STATE_KINDS)
@pytest.mark.parametrize("name, stage, cyl", STATE_SCENES, ids=[s[0] for s in STATE_SCENES])
def test_steps_of_caller_held_states_are_the_step_oracle(name, stage, cyl, kind, fetch):
    """rl_scene_step_paths_device and rl_scene_step_path_list_device (a shuffled list with entries out of range and a third of the
    states left out, into guarded, prefilled buffers): states and hits byte for byte -- path_index, object and reserved written
    back as the oracle has them, segments + 1 wrapped, the bounce drawn from block (2 + segments) mod 2^32 at each lane's own
    64-bit path index."""
    case = RW.BY_ID["carry-mid-wave"]
    _, _, scene, _ = _scenes(name, lit=True)
    held = _held_states(name, kind)
    start, lst, left_out = held["states"], held["list"], held["left_out"]
    meant = (2 * stage if fetch == R.FETCH_LDS else 0) + cyl
    live_before = start["end"] == LIVE
    assert 0.2 < live_before.mean() < 1.0 or name != "demo"
    for flags in (0, R.RL_STEP_NO_ROULETTE):
        what = "%s %s fetch %d flags %d" % (name, kind, fetch, flags)
        all_st, all_hits, listed_st, listed_hits, want_live = held[flags]
        if kind == "segments":
            stepped = live_before & (start["segments"] == 0xFFFFFFFF)
            assert (stepped.any() or name != "demo") and (all_st["segments"][stepped] == 0).all()
        sb, hb = _Device(start), _Device(_poison_hits(NQ))
        before = R.step_launches()
        scene.step_paths_device(sb.buf, case.seed, case.stream, fetch=fetch, flags=flags, hits=hb.buf)
        assert _variant_of(R.step_launches, before) == meant, what
        assert_same(sb.get(), all_st, what + ": rl_scene_step_paths_device, states")
        assert_same(hb.get(), all_hits, what + ": rl_scene_step_paths_device, hits")
        gs, gh = G.device_guarded(initial=start), G.device_guarded(initial=_poison_hits(NQ))
        gl, gv = G.device_guarded(initial=lst), G.device_guarded(len(lst) * 4)
        before = R.path_list_launches()
        n_live = scene.step_path_list_device(gs, case.seed, case.stream, gl, len(lst), gv, fetch=fetch, flags=flags, hits=gh)
        assert _variant_of(R.path_list_launches, before) == meant, what
        assert_same(gs.payload(what, R.PATH_STATE_DTYPE), listed_st, what + ": rl_scene_step_path_list_device, states")
        assert_same(gh.payload(what + ": hits", R.HIT_DTYPE), listed_hits, what + ": rl_scene_step_path_list_device, hits")
        assert gl.payload(what + ": list", np.uint32).tobytes() == lst.tobytes()
        got_live = gv.payload(what + ": live_list", np.uint32)
        assert n_live == len(want_live) and got_live[:n_live].tolist() == want_live.tolist(), what
        assert (got_live[n_live:] == FILL32).all(), what


@pytest.mark.parametrize("fetch", FETCHES, ids=FETCH_IDS)
@pytest.mark.parametrize("kind", STATE_KINDS)
@pytest.mark.parametrize("name, stage, cyl", STATE_SCENES, ids=[s[0] for s in STATE_SCENES])
def test_light_samples_of_caller_held_states_are_the_light_oracle(name, stage, cyl, kind, fetch):
    """rl_scene_light_paths* and rl_plot_unit_light_paths* on the same states: the light's block is (2^31 + segments) mod 2^32 at
    each lane's own 64-bit path index."""
    case = RW.BY_ID["carry-mid-wave"]
    objs, _, scene, _ = _scenes(name, lit=True)
    held = _held_states(name, kind)
    rows = held["lit"]
    st, hits = np.ascontiguousarray(held["states"][rows]), np.ascontiguousarray(held["hits"][rows])
    camera = np.ascontiguousarray(held["camera"][rows])
    want = held["samples"]
    if name == "demo":
        assert (want["status"] != LO.SKIPPED).sum() > 100
    for device in (True, False):
        v = _light_calls(scene, st, hits, camera, case.seed, case.stream, fetch, device,
                         "%s %s fetch %d %s" % (name, kind, fetch, "device" if device else "host"), want, LO.emitters(objs.view(O.OBJECT_DTYPE)))
        assert v == (2 * stage if fetch == R.FETCH_LDS else 0) + cyl
