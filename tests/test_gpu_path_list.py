"""Scene.step_path_list* on the device (rl_scene_step_path_list*), bit for bit and through the C ABI: the listed loop from the
identity list to the last live path gives rl_scene_render_rays' results, and after every step the states, the hits and the
survivors' list are those of the numpy restatement (tests/_path_list_oracle.py); one listed step of the identity list equals
rl_scene_step_paths_device byte for byte; a hostile list (shuffled, with entries out of range, with ended states, a third of the
states left out) into guarded, prefilled buffers; live_list == list; RL_STEP_NO_ROULETTE; every kernel variant on poisoned LDS;
list sizes around the chunk of 64 and beyond the slice rule's threshold.  A GPU fault ends the run: nothing here provokes one."""
import ctypes as C

import numpy as np
import pytest

import _guarded as G
import _lds_poison as LP
import _path_list_oracle as L
import _step_oracle as S
from _cases import _rays, _results
from _compare import assert_same
from _device_arrays import _Device, _Words, _begin_device, _poison_hits, _slice_crossing_size
from _scenes import _scene

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

NONE, LIVE = R.RL_OBJECT_NONE, R.RL_PATH_LIVE
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
W, H = 320, 180
BUDGET = R.RL_PATH_MAX_SEGMENTS
FILL32 = 0xAAAAAAAA


def _step(scene, sb, seed, stream, lst, n_list, live, fetch=R.FETCH_LDS, flags=0, hb=None):
    """One listed step in the device form; lst and live are _Words (or None).  Returns n_live."""
    return scene.step_path_list_device(sb.buf, seed, stream, None if lst is None else lst.buf, n_list, None if live is None else live.buf,
                                       fetch=fetch, flags=flags, hits=None if hb is None else hb.buf)


# ---- (a) the loop ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo", "glass", "random-seed-1", "random-seed-2", "many-prisms"])
def test_listed_loop_is_render_rays_and_every_step_is_the_oracle(name):
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    n, seed, stream, first = 1500, 3 + len(name), 1, 1000
    rays = _rays(scene, n, seed, stream, first)
    want = scene.render_spectral_rays(rays, seed, stream, first)
    assert (want["end"] != R.RL_PATH_END_LIMIT).all() and (want["value"] != 0).any()
    # the oracle's loop, once: (states, hits, survivors) after every step
    so = S.StepOracle(objs, cam)
    ost, ohits, olive, turns = S.begin(rays, first), _poison_hits(n), None, []
    while olive is None or len(olive):
        assert len(turns) < BUDGET
        olive = L.step_list(so, ost, seed, stream, list=olive, hits=ohits)
        turns.append((ost.copy(), ohits.copy(), olive.copy()))
    assert len(turns) == int(want["segments"].max())
    for fetch in FETCHES:
        sb, hb = _begin_device(scene, rays, first), _Device(_poison_hits(n))
        ping, pong = _Words(np.full(n, FILL32)), _Words(np.full(n, FILL32))
        lst, n_list, steps = None, n, 0
        while n_list and steps < BUDGET:
            out = pong if lst is ping else ping
            n_live = _step(scene, sb, seed, stream, lst, n_list, out, fetch, hb=hb)
            what = "%s fetch %d step %d" % (name, fetch, steps)
            wst, whits, wlive = turns[steps]
            assert n_live == len(wlive), (what, n_live, len(wlive))
            got_live = out.get()
            assert got_live[:n_live].tolist() == wlive.tolist(), what
            assert (got_live[n_live:n_list] == (FILL32 if steps < 2 else got_live[n_live:n_list])).all()
            assert (np.diff(got_live[:n_live].astype(np.int64)) > 0).all(), what   # the first list was the identity: strictly ascending
            assert_same(sb.get(), wst.view(R.PATH_STATE_DTYPE), what + ": states")
            assert_same(hb.get(), whits, what + ": hits")
            lst, n_list = out, n_live
            steps += 1
        assert n_list == 0 and steps < BUDGET, (name, fetch, steps)   # the cap was not reached
        assert steps == len(turns)
        final = sb.get()
        assert (final["end"] != LIVE).all()
        assert_same(_results(final), want, "%s fetch %d: final states against render_rays" % (name, fetch))
    # the host form, looped the same way
    st, live, steps = scene.begin_paths(rays, first), None, 0
    while (live is None or len(live)) and steps < BUDGET:
        live = scene.step_path_list(st, seed, stream, list=live)
        assert live.tolist() == turns[steps][2].tolist()
        steps += 1
    assert steps == len(turns)
    assert_same(st, turns[-1][0].view(R.PATH_STATE_DTYPE), "%s: host form" % name)


# ---- (b) one step against rl_scene_step_paths_device, (g) sizes -------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4033, "slice"])
def test_identity_list_equals_step_paths_device_in_every_byte(n):
    big = n == "slice"
    n = _slice_crossing_size() if big else n
    scene = R.Scene(*_scene("demo"))
    seed, stream, first = 9, 0, 5
    rays = _rays(scene, n, seed, stream, first)
    begun = _begin_device(scene, rays, first).get().copy()
    del rays
    for fetch in ((R.FETCH_LDS,) if big else FETCHES):
        for with_hits in ((False,) if big else (True, False)):
            what = "n=%d fetch %d hits=%s" % (n, fetch, with_hits)
            a, b = _Device(begun), _Device(begun)
            ha, hb = (_Device(_poison_hits(n)), _Device(_poison_hits(n))) if with_hits else (None, None)
            live = _Words(np.full(n, FILL32))
            for step in range(1 if big else 3):   # (the identity list every time: ended states are listed and not written)
                scene.step_paths_device(a.buf, seed, stream, fetch=fetch, hits=None if ha is None else ha.buf)
                n_live = _step(scene, b, seed, stream, None, n, live, fetch, hb=hb)
                want = a.get()
                assert b.get().tobytes() == want.tobytes(), what
                if with_hits:
                    assert hb.get().tobytes() == ha.get().tobytes(), what
                survivors = np.flatnonzero(want["end"] == LIVE)
                got = live.get()
                assert n_live == len(survivors), (what, n_live, len(survivors))
                assert (got[:n_live] == survivors).all(), what
                assert (got[n_live:] == FILL32).all() or step > 0, what
            # without a survivors' list, and with the count alone
            c = _Device(begun)
            assert _step(scene, c, seed, stream, None, n, None, fetch) == int((scene_first_step_live(a, begun, scene, seed, stream, fetch)))
    if not big:
        # a shorter identity list steps a prefix; the rest is untouched
        k = max(1, n // 2)
        c, live = _Device(begun), _Words(np.full(n, FILL32))
        n_live = _step(scene, c, seed, stream, None, k, live)
        ref = begun.copy()
        scene.step_paths(ref[:k], seed, stream)
        assert c.get().tobytes() == ref.tobytes()
        assert live.get()[:n_live].tolist() == np.flatnonzero(ref["end"][:k] == LIVE).tolist() and (live.get()[n_live:] == FILL32).all()


def scene_first_step_live(a, begun, scene, seed, stream, fetch):
    """The number of states of `begun` that are live after one step (by rl_scene_step_paths_device on a copy)."""
    d = _Device(begun)
    scene.step_paths_device(d.buf, seed, stream, fetch=fetch)
    return (d.get()["end"] == LIVE).sum()


# ---- (c) a hostile list ------------------------------------------------------------------------------------------------------

_guarded = G.device_guarded


@pytest.mark.parametrize("name", ["demo", "glass"])
def test_hostile_list_into_guarded_prefilled_buffers(name):
    objs, cam = _scene(name)
    scene = R.Scene(objs, cam)
    n, seed, stream, first = 2113, 21, 3, 1 << 35
    rng = np.random.default_rng(n + len(name))
    start = scene.begin_paths(_rays(scene, n, seed, stream, first), first)
    scene.step_paths(start, seed, stream)
    scene.step_paths(start, seed, stream)          # two segments in: some states have ended
    ended = start["end"] != LIVE
    assert 0.05 < ended.mean() < 0.95
    left_out = np.arange(n) % 3 == 1               # a third of the states is not listed
    listed = np.flatnonzero(~left_out)
    assert ended[listed].any() and (~ended)[listed].any() and (~ended)[left_out].any()
    wild = np.concatenate([[n, n + 1, 0xffffffff, 0x80000000, 0xfffffffe, n + 63, n + 64], rng.integers(n, 1 << 32, 200)]).astype(np.uint32)
    lst = np.concatenate([listed.astype(np.uint32), wild])
    lst = lst[rng.permutation(len(lst))]
    so = S.StepOracle(objs, cam)
    for fetch in FETCHES:
        for flags in (0, R.RL_STEP_NO_ROULETTE):
            what = "%s fetch %d flags %d" % (name, fetch, flags)
            want, want_hits = start.copy(), np.frombuffer(bytes([G.FILL]) * (48 * n), dtype=R.HIT_DTYPE).copy()
            want_live = L.step_list(so, want, seed, stream, list=lst, flags=flags, hits=want_hits)
            sb, hb = _guarded(initial=start), _guarded(n * 48)
            lb, vb = _guarded(initial=lst), _guarded(len(lst) * 4)
            n_live = scene.step_path_list_device(sb, seed, stream, lb, len(lst), vb, fetch=fetch, flags=flags, hits=hb)
            got, got_hits = sb.payload(what, R.PATH_STATE_DTYPE), hb.payload(what + ": hits", R.HIT_DTYPE)
            got_live, got_list = vb.payload(what + ": live_list", np.uint32), lb.payload(what + ": list", np.uint32)
            assert got_list.tobytes() == lst.tobytes(), what + ": the list was written"
            G.assert_written_as(got, want, what)
            G.assert_written_as(got_hits, want_hits, what + ": hits")
            untouched = left_out | ended
            assert got[untouched].tobytes() == start[untouched].tobytes(), what
            assert (got_hits[untouched].view(np.uint8) == G.FILL).all(), what
            assert (got["segments"][~untouched] == 3).all()
            assert n_live == len(want_live) and got_live[:n_live].tolist() == want_live.tolist(), what
            assert (got_live[n_live:] == FILL32).all(), what + ": written behind n_live"
            assert 0 < n_live < len(listed)
            # the host form on the same list
            host, host_hits = start.copy(), np.frombuffer(bytes([G.FILL]) * (48 * n), dtype=R.HIT_DTYPE).copy()
            host_live = scene.step_path_list(host, seed, stream, list=lst, fetch=fetch, flags=flags, hits=host_hits)
            assert host.tobytes() == want.tobytes() and host_hits.tobytes() == want_hits.tobytes() and host_live.tolist() == want_live.tolist()


# ---- (d) live_list == list ---------------------------------------------------------------------------------------------------

def test_live_list_may_be_the_list():
    scene = R.Scene(*_scene("demo"))
    n, seed, stream, first = 64 * 40 + 17, 8, 0, 77
    begun = scene.begin_paths(_rays(scene, n, seed, stream, first), first)
    lst = np.random.default_rng(5).permutation(n).astype(np.uint32)
    for fetch in FETCHES:
        a, b = _Device(begun), _Device(begun)
        la, va = _Words(lst), _Words(np.full(n, FILL32))
        lb = _Words(lst)
        na = _step(scene, a, seed, stream, la, n, va, fetch)
        nb = _step(scene, b, seed, stream, lb, n, lb, fetch)
        assert na == nb and 0 < na < n
        assert b.get().tobytes() == a.get().tobytes()
        assert la.get().tobytes() == lst.tobytes()
        assert lb.get()[:nb].tolist() == va.get()[:na].tolist()
        assert lb.get()[nb:].tolist() == lst[nb:].tolist()      # nothing written behind the count
        assert (va.get()[na:] == FILL32).all()
        final = a.get()
        assert va.get()[:na].tolist() == [i for i in lst.tolist() if final["end"][i] == LIVE]   # stable: the list's order


# ---- (e) RL_STEP_NO_ROULETTE -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["demo", "glass"])
def test_no_roulette_keeps_every_bounced_state_listed(name):
    scene = R.Scene(*_scene(name))
    n, seed, stream, first = 4033, 31, 4, 1 << 33
    st = scene.begin_paths(_rays(scene, n, seed, stream, first), first)
    lst, kept_by_flag = None, 0
    for step in range(4):
        hits = _poison_hits(n)
        before = st.copy()
        plain = scene.step_path_list(st.copy(), seed, stream, list=lst)
        live = scene.step_path_list(st, seed, stream, list=lst, flags=R.RL_STEP_NO_ROULETTE, hits=hits)
        listed = np.arange(n) if lst is None else lst.astype(np.int64)
        stepped = listed[before["end"][listed] == LIVE]
        bounced = stepped[(hits["object"][stepped] != NONE) & (st["end"][stepped] != R.RL_PATH_END_EMITTER)]
        assert live.tolist() == bounced.tolist(), (name, step)   # neither the void nor an emitter: still listed
        assert not (st["end"] == R.RL_PATH_END_ROULETTE).any()
        kept_by_flag += len(live) - len(plain)
        assert set(plain.tolist()) <= set(live.tolist())
        lst = live
        assert len(live)
    assert kept_by_flag > 0


# ---- (f) every variant on poisoned LDS ---------------------------------------------------------------------------------------

POISON_SCENES = ["demo", "many-prisms", "demo-2500", "tables-prisms", "random-6000"]   # whole scene / tables / third level, with and without CYL


@pytest.mark.parametrize("pattern", LP.PATTERNS, ids=lambda p: "0x%08X" % p)
def test_every_variant_on_poisoned_lds(pattern):
    """The LDS of every CU filled with the pattern immediately before each listed step; states, hits and survivors against
    rl_scene_step_paths (whose own poisoned runs tests/test_gpu_dirty_state.py holds against the oracle) for four steps, and
    rl_debug_path_list_launches names one variant per call: all six by the end."""
    ran, fed_back = set(), 0
    for name in POISON_SCENES:
        objs, cam = _scene(name)
        scene = R.Scene(objs, cam)
        cyl = int((objs["surface_kind"] == 4).sum() >= 40)
        n, seed, stream, first = 2113, 5, 2, 12345
        begun = scene.begin_paths(_rays(scene, n, seed, stream, first), first)
        for fetch in FETCHES:
            ref, ref_hits = begun.copy(), _poison_hits(n)
            sb, hb = _Device(begun), _Device(_poison_hits(n))
            ping, pong = _Words(np.full(n, FILL32)), _Words(np.full(n, FILL32))
            lst, n_list = None, n
            for step in range(4):
                what = "%s pattern 0x%08X fetch %d step %d" % (name, pattern, fetch, step)
                scene.step_paths(ref, seed, stream, fetch=fetch, hits=ref_hits)
                out = pong if lst is ping else ping
                before = R.path_list_launches()
                LP.poison_lds(pattern)
                n_live = _step(scene, sb, seed, stream, lst, n_list, out, fetch, hb=hb)
                launched = [a - b for a, b in zip(R.path_list_launches(), before)]
                assert sum(launched) == 1, (what, launched)
                v = launched.index(1)
                assert v % 2 == cyl and (fetch == R.FETCH_LDS or v // 2 == 0), (what, v)
                ran.add(v)
                assert_same(sb.get(), ref, what + ": states")
                assert_same(hb.get(), ref_hits, what + ": hits")
                survivors = np.flatnonzero(ref["end"] == LIVE)
                assert n_live == len(survivors) and (out.get()[:n_live] == survivors).all(), what
                lst, n_list = out, n_live
                fed_back += int(step > 0)
                if not n_live:                      # (a scene most of whose camera rays leave at once: nothing left to list)
                    break
    assert fed_back >= 6                            # survivors' lists went back in as lists, not only the identity list
    assert ran == set(range(6)), sorted(ran)


# ---- the device form's own checks --------------------------------------------------------------------------------------------

def test_device_form_refuses_host_memory_and_misaligned_buffers():
    scene = R.Scene(*_scene("demo"))
    begun = scene.begin_paths(_rays(scene, 64, 1, 0, 0), 0)
    sb, lb = _Device(begun), _Words(np.arange(64))
    host_list = np.arange(64, dtype=np.uint32)
    n_live = C.c_uint32(7)
    fn, h = R.lib.rl_scene_step_path_list_device, scene.handle
    sp, lp = C.c_void_p(sb.buf.data_ptr()), C.c_void_p(lb.buf.data_ptr())
    assert fn(h, 0, 1, 0, 0, sp, 64, host_list.ctypes.data_as(C.c_void_p), 64, None, None, C.byref(n_live)) == -1 and b"device memory" in R.lib.rl_last_error()
    assert fn(h, 0, 1, 0, 0, sp, 64, lp, 64, None, host_list.ctypes.data_as(C.c_void_p), C.byref(n_live)) == -1 and b"device memory" in R.lib.rl_last_error()
    assert fn(h, 0, 1, 0, 0, begun.ctypes.data_as(C.c_void_p), 64, lp, 64, None, None, None) == -1
    assert fn(h, 0, 1, 0, 0, C.c_void_p(sb.buf.data_ptr() + 8), 63, lp, 63, None, None, None) == -1 and b"aligned" in R.lib.rl_last_error()
    assert fn(h, 0, 1, 0, 0, sp, 64, C.c_void_p(lb.buf.data_ptr() + 2), 32, None, None, None) == -1 and b"aligned" in R.lib.rl_last_error()
    assert sb.get().tobytes() == begun.tobytes() and (lb.get() == np.arange(64)).all() and (host_list == np.arange(64)).all()
    # a list longer than the states, all of it out of range but one entry
    lst = _Words(np.array([64, 65, 5, 0xffffffff, 1 << 31], np.uint32))
    live = _Words(np.full(5, FILL32))
    assert fn(h, 0, 1, 0, 0, sp, 64, C.c_void_p(lst.buf.data_ptr()), 5, None, C.c_void_p(live.buf.data_ptr()), C.byref(n_live)) == 0
    after = sb.get()
    changed = [i for i in range(64) if after[i].tobytes() != begun[i].tobytes()]
    assert changed == [5] and after["segments"][5] == 1
    assert n_live.value == int(after["end"][5] == LIVE) and (live.get()[n_live.value:] == FILL32).all()
