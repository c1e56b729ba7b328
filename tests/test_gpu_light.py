"""Scene.light_paths* on the device (rl_scene_light_paths*): every byte of the samples against the numpy restatement
(tests/_light_oracle.py) on the scenes that reach all six kernel variants; list sizes around the chunk of 64 and beyond the slice
rule's threshold; a hostile list into guarded, prefilled buffers; determinism under splits, permutations and the fetch mode;
agreement with rl_scene_occluded on the rebuilt shadow rays; the estimator's mean against the path's own emitter hits; every
variant on poisoned LDS.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C

import numpy as np
import pytest

import _guarded as G
import _lds_poison as LP
import _light_oracle as LO
import _oracle as O
import _query_rays as QR
from _cases import _rays, _stepped, bounce_directions, vertex_states
from _compare import assert_means_agree, assert_same
from _device_arrays import _Device, _Words, _prefilled, _slice_crossing_size
from _scenes import _lit_scene, _scene, closed_scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
SCENES = ["demo", "many-prisms", "demo-2500", "tables-prisms", "random-6000"]   # whole scene / tables / third level, with and without CYL
FILL32 = 0xAAAAAAAA
SAMPLE = R.LIGHT_SAMPLE_DTYPE


def _light_device(scene, st, hits, seed, stream, lst=None, n_list=None, fetch=R.FETCH_LDS, samples=None):
    sb, hb = _Device(st), _Device(hits)
    mb = _Device(_prefilled(len(st)) if samples is None else samples)
    scene.light_paths_device(sb.buf, hb.buf, mb.buf, seed, stream, None if lst is None else _Words(lst).buf, len(st) if n_list is None and lst is None else
                             (len(lst) if n_list is None else n_list), fetch=fetch)
    assert sb.get().tobytes() == st.tobytes() and hb.get().tobytes() == hits.tobytes()
    return mb.get().copy()


# ---- 1. bit-exact against the oracle -----------------------------------------------------------------------------------------

def test_every_byte_is_the_oracle_on_all_six_variants():
    before = R.light_launches()
    for name in SCENES:
        objs, cam = _lit_scene(name)
        scene = R.Scene(objs, cam)
        assert scene.emitters().tolist() == R.description_emitters(objs).tolist() == LO.emitters(objs.view(O.OBJECT_DTYPE)).tolist()
        occ = LO.Occluder(objs, cam)
        n, seed, stream, first = 4097, 7, 1, 1 << 34      # seed 7: the first seed tried gives every class its 5 % in the demo scene
        for steps in (1, 2, 3):
            st, hits = _stepped(scene, n, seed, stream, first, steps)
            want = LO.light_paths(occ, st, hits, seed, stream, samples=_prefilled(n).view(LO.SAMPLE_DTYPE)).view(SAMPLE)
            if name == "demo" and steps == 2:
                share = np.bincount(want["status"], minlength=4) / float(n)
                assert (share >= 0.05).all(), share      # on the oracle's output alone: no class is vacuous
            for fetch in FETCHES:
                got = _light_device(scene, st, hits, seed, stream, fetch=fetch)
                assert_same(got, want, "%s steps %d fetch %d" % (name, steps, fetch))
        host = scene.light_paths(st, hits, seed, stream)
        assert_same(host, want, "%s: host form" % name)
    ran = [a - b for a, b in zip(R.light_launches(), before)]
    assert all(r > 0 for r in ran), ran


# ---- 2. sizes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4033, "slice"])
def test_identity_list_equals_the_listed_form_in_every_byte(n):
    n = _slice_crossing_size() if n == "slice" else n
    scene = R.Scene(*_scene("demo"))
    seed, stream, first = 9, 0, 5
    sb = _Device(scene.begin_paths(_rays(scene, n, seed, stream, first, holes=False), first))
    hb = _Device(np.zeros(n, R.HIT_DTYPE))
    for _ in range(2):
        scene.step_paths_device(sb.buf, seed, stream, hits=hb.buf)
    a, b = _Device(_prefilled(n)), _Device(_prefilled(n))
    lst = _Words(np.arange(n))
    scene.light_paths_device(sb.buf, hb.buf, a.buf, seed, stream)
    scene.light_paths_device(sb.buf, hb.buf, b.buf, seed, stream, list=lst.buf, n_list=n)
    got = a.get()
    assert got.tobytes() == b.get().tobytes()
    assert (got["status"] <= 3).all() and (n < 64 or (got["status"] == R.RL_LIGHT_VISIBLE).any())
    # a shorter identity list samples a prefix; the rest is untouched
    k = max(1, n // 2)
    c = _Device(_prefilled(n))
    scene.light_paths_device(sb.buf, hb.buf, c.buf, seed, stream, n_list=k)
    part = c.get()
    assert part[:k].tobytes() == got[:k].tobytes() and (part[k:].view(np.uint8) == G.FILL).all()


# ---- 3. a hostile list into guarded buffers ----------------------------------------------------------------------------------

def test_hostile_list_into_guarded_prefilled_buffers():
    objs, cam = _scene("demo")
    scene = R.Scene(objs, cam)
    n, seed, stream, first = 2113, 21, 3, 1 << 35
    rng = np.random.default_rng(n)
    st, hits = _stepped(scene, n, seed, stream, first, 2)
    left_out = np.arange(n) % 3 == 1
    listed = np.flatnonzero(~left_out)
    wild = np.concatenate([[n, n + 1, 0xffffffff, 0x80000000, 0xfffffffe, n + 63, n + 64], rng.integers(n, 1 << 32, 200)]).astype(np.uint32)
    lst = np.concatenate([listed.astype(np.uint32), wild])
    lst = lst[rng.permutation(len(lst))]
    want = LO.light_paths(LO.Occluder(objs, cam), st, hits, seed, stream, list=lst, n_list=len(lst), samples=_prefilled(n).view(LO.SAMPLE_DTYPE))
    guard = lambda **kw: G.Guarded(QR.DeviceBuffer, **kw)
    for fetch in FETCHES:
        what = "fetch %d" % fetch
        sb, hb, lb, mb = guard(initial=st), guard(initial=hits), guard(initial=lst), guard(nbytes=32 * n)
        scene.light_paths_device(sb, hb, mb, seed, stream, list=lb, n_list=len(lst), fetch=fetch)
        got = mb.payload(what + ": samples", SAMPLE)
        assert sb.payload(what + ": states").tobytes() == st.tobytes(), what + ": the states were written"
        assert hb.payload(what + ": hits").tobytes() == hits.tobytes(), what + ": the hits were written"
        assert lb.payload(what + ": list").tobytes() == lst.tobytes(), what + ": the list was written"
        G.assert_written_as(got, want, what)
        assert (got[left_out].view(np.uint8) == G.FILL).all() and not (got[listed].view(np.uint32) == FILL32).all(axis=None)
        host = scene.light_paths(st, hits, seed, stream, list=lst, fetch=fetch, samples=_prefilled(n))
        assert host.tobytes() == want.tobytes(), what + ": host form"
    # the device form's own checks: pageable host memory and misaligned buffers are refused, nothing written
    fn, h = R.lib.rl_scene_light_paths_device, scene.handle
    sb, hb, mb, lb = _Device(st), _Device(hits), _Device(_prefilled(n)), _Words(lst)
    sp, hp, mp, lp = (C.c_void_p(d.buf.data_ptr()) for d in (sb, hb, mb, lb))
    host_ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    host_samples = _prefilled(n)
    for args in ((host_ptr(st), n, lp, 8, hp, mp), (sp, n, host_ptr(lst), 8, hp, mp), (sp, n, lp, 8, host_ptr(hits), mp), (sp, n, lp, 8, hp, host_ptr(host_samples))):
        assert fn(h, 0, seed, stream, *args) == -1 and b"device memory" in R.lib.rl_last_error(), args
    for args in ((C.c_void_p(sp.value + 8), n - 1, lp, 8, hp, mp), (sp, n, lp, 8, hp, C.c_void_p(mp.value + 8)), (sp, n, C.c_void_p(lp.value + 2), 8, hp, mp)):
        assert fn(h, 0, seed, stream, *args) == -1 and b"aligned" in R.lib.rl_last_error(), args
    assert (mb.get().view(np.uint8) == G.FILL).all() and (host_samples.view(np.uint8) == G.FILL).all()


# ---- 4. determinism, 5. agreement with the occlusion query -------------------------------------------------------------------

def test_splits_permutations_and_fetch_modes_give_the_same_records_and_the_occlusion_query_agrees():
    for name in ("demo", "many-prisms"):
        scene = R.Scene(*_lit_scene(name))
        n, seed, stream, first = 4097, 13, 2, 99
        st, hits = _stepped(scene, n, seed, stream, first, 2)
        whole = _light_device(scene, st, hits, seed, stream)
        assert (whole.view(np.uint32).reshape(n, 8) != FILL32).any(axis=1).all()
        assert _light_device(scene, st, hits, seed, stream, fetch=R.FETCH_GLOBAL).tobytes() == whole.tobytes()
        cuts = [0, 1000, 1001, n]
        parts = [_light_device(scene, st[a:b], hits[a:b], seed, stream) for a, b in zip(cuts, cuts[1:])]
        assert np.concatenate(parts).tobytes() == whole.tobytes()
        perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
        assert _light_device(scene, st, hits, seed, stream, lst=perm).tobytes() == whole.tobytes()
        moved = _light_device(scene, st[perm], hits[perm], seed, stream)        # the states themselves reordered
        assert moved.tobytes() == whole[perm].tobytes()
        # the cast shadow rays, rebuilt from the sample and the hit, through rl_scene_occluded_device
        cast = np.flatnonzero(whole["status"] >= R.RL_LIGHT_OCCLUDED)
        assert len(cast) > (n // 20 if name == "demo" else 0)      # (the demo scene's shares: test 1; a random scene's camera may face few lights)
        rays = np.zeros(len(cast), R.RAY_DTYPE)
        d = whole["direction"][cast]
        rays["origin"] = hits["position"][cast] + d * np.float32(0.00001)
        rays["direction"] = d
        rays["t_max"] = (whole["distance"][cast] - np.float32(0.00001)) * np.float32(0.9990234375)
        rb, ob = _Device(rays), _Device(np.full(len(cast), 0xAA, np.uint8))
        scene.occluded_device(rb.buf, ob.buf)
        blocked = ob.get()
        assert (blocked == (whole["status"][cast] == R.RL_LIGHT_OCCLUDED)).all(), name
        assert name != "demo" or 0 < blocked.sum() < len(cast)
        lit = whole["status"] == R.RL_LIGHT_VISIBLE
        assert (whole["value"][lit] == st["intensity"][lit] * whole["weight"][lit]).all() and not whole["value"][~lit].any()


# ---- 6. it is the right estimator --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("occluder", [True, False])
def test_the_mean_of_the_samples_is_the_mean_of_the_paths_own_emitter_hits(occluder):
    """2^16 states at one vertex of a small closed scene: the mean of `value` from this call against the mean of `value` over the
    same states stepped once more with RL_STEP_NO_ROULETTE, counting only ends on the two lights; at most 5 combined standard
    errors apart, each from the samples (tests/test_light_abi.py runs the same on the CPU oracle)."""
    objs, cam = closed_scene(occluder)
    scene = R.Scene(objs, cam)
    n, seed, stream = 1 << 16, 17, 3
    st, ht = vertex_states(n)
    light = scene.light_paths(st, ht, seed, stream)
    seen = set(np.unique(light["status"]).tolist())
    assert seen >= ({R.RL_LIGHT_BACKFACING, R.RL_LIGHT_VISIBLE} | ({R.RL_LIGHT_OCCLUDED} if occluder else set())), seen
    # the path's own next segment leaves the vertex in the direction its diffuse bounce draws: the step before this vertex made it
    nxt = st.copy()
    nxt["direction"] = bounce_directions(st, seed, stream)
    nxt["origin"] = (ht["position"] + nxt["direction"] * np.float32(1e-5)).astype(np.float32)
    scene.step_paths(nxt, seed, stream, flags=R.RL_STEP_NO_ROULETTE)
    lights = scene.emitters()
    assert lights.tolist() == [1, 2]
    on_light = (nxt["end"] == R.RL_PATH_END_EMITTER) & np.isin(nxt["object"], lights)
    assert_means_agree(light["value"], np.where(on_light, nxt["value"], 0), "occluder %s" % occluder)


# ---- 7. every variant on poisoned LDS ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
def test_every_variant_on_poisoned_lds(pattern):
    """The LDS of every CU filled with the pattern immediately before each call; the samples against a call on clean LDS under the
    other fetch mode's variant where there is one (test 1 holds those against the oracle), and rl_debug_light_launches names one
    variant per call: all six by the end."""
    ran = set()
    for name in SCENES:
        objs, cam = _lit_scene(name)
        scene = R.Scene(objs, cam)
        cyl = int((objs["surface_kind"] == 4).sum() >= 40)
        n, seed, stream, first = 2113, 5, 2, 12345
        st, hits = _stepped(scene, n, seed, stream, first, 2)
        sb, hb = _Device(st), _Device(hits)
        ref = _Device(_prefilled(n))
        scene.light_paths_device(sb.buf, hb.buf, ref.buf, seed, stream, fetch=R.FETCH_GLOBAL)
        want = ref.get().copy()
        for fetch in FETCHES:
            what = "%s pattern 0x%08X fetch %d" % (name, pattern, fetch)
            mb = _Device(_prefilled(n))
            before = R.light_launches()
            LP.poison_lds(pattern)
            scene.light_paths_device(sb.buf, hb.buf, mb.buf, seed, stream, fetch=fetch)
            launched = [a - b for a, b in zip(R.light_launches(), before)]
            assert sum(launched) == 1, (what, launched)
            v = launched.index(1)
            assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
            ran.add(v)
            assert_same(mb.get(), want, what)
    assert ran == set(range(6)), sorted(ran)
