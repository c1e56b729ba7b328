"""Wavelength importance sampling on the device (rl_wavelength_table_*, rl_trace_unit_set_wavelengths, rl_app_run_sampled): the
table read back against the numpy rule; the photons of every launch kind byte for byte against tests/wavelength_host, the g++ compile
of the same per-path header; fused films against the oracle's plot of those photons by the film tests' bars; which instantiation
ran; open launches keyed by the table; dirty LDS; set and reset; the film's expectation and the recorded gain; the App and the
command line.  A GPU fault ends the run: nothing here provokes one."""
import functools
import json
import os

import numpy as np
import pytest

import _boundary as B
import _lds_poison as LP
import _mirror as M
import _oracle as O
import _rng_width as RW
import _scenes as SC
import _wavelength_oracle as WO
from _boundary import _ocam
from _compare import assert_film

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip
from robigo_luculenta_amd import __main__ as CLI

RL_E_STATE = -5
W, H = 64, 36
N_PLAIN, N_OPEN = 4096, 4160       # a plain launch; a blocking render of a multiple of 64 paths: an open one
SEED, STREAM, FIRST = 5, 2, 777
FETCHES = (R.FETCH_LDS, R.FETCH_GLOBAL)
SCENES = ["demo", "edge-tables", "prisms-300", "glass"]     # staged whole; tables; nothing staged; the second prism bound
MORE_SCENES = ["edge-whole+1", "tables-prisms"]             # tables in plain and open launches alike, without and with the second bound; the CIE table only
TABLES = ("cie-0.1", "one-hot-1e-3", "null")
CARRY = RW.BY_ID["carry-mid-wave"]
_ran = set()


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name):
    c = _Case()
    c.name = name
    objs, cam = SC._scene(name)
    c.objs, c.cam = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), cam
    c.scene = R.Scene(c.objs, c.cam)
    c.host = WO.HostScene(c.objs, cam)
    c.lay = M.layout(M.Scene(c.objs.view(O.OBJECT_DTYPE), _ocam(cam)))
    return c


@functools.lru_cache(maxsize=None)
def _table(name):
    """(the table on the device, its 513 floats by the numpy rule); what the device holds is the rule's, bit for bit."""
    g, n, u = WO.case_table(name)
    table = R.WavelengthTable(g, u, n_nodes=n)
    status, q, w = WO.table(g, n, u)
    assert status == WO.OK
    got_q, got_w = table.download()
    assert got_q.tobytes() == q.tobytes() and got_w.tobytes() == w.tobytes(), name
    return table, WO.packed(q, w)


@functools.lru_cache(maxsize=None)
def _reference(scene, table, seed=SEED, stream=STREAM, first=FIRST):
    """(photons of N_OPEN paths, segments of the first N_PLAIN, segments of all) by the host compile; computed once."""
    c = _case(scene)
    tab = _table(table)[1] if table else None
    head, head_segs, _ = c.host.render(W, H, tab, seed, stream, first, N_PLAIN)
    tail, tail_segs, _ = c.host.render(W, H, tab, seed, stream, first + N_PLAIN, N_OPEN - N_PLAIN)
    photons = np.concatenate([head, tail])
    photons.setflags(write=False)
    return photons, head_segs, head_segs + tail_segs


def _meant(c, fetch, fused, open_launch):
    stage = M.predicted_stage(c.lay, fetch == R.FETCH_LDS, open_launch)[0]
    low = (4 if fused else 0) | (2 if open_launch else 0) | c.lay["prism_cylinders"]
    return 16 + low if stage == M.STAGE_TABLES else (8 if stage == M.STAGE_ALL else 0) | low


def _held(c, fetch, fused, open_launch, call, what):
    """call(), held to the one WL instantiation predicted for the scene; the counters of the plain instantiations must not move."""
    plain, before = R.variant_launches(), R.wavelength_variant_launches()
    call()
    v = B._variant_of(R.wavelength_variant_launches, before)
    assert v == _meant(c, fetch, fused, open_launch), "%s: WL variant %d ran, predicted %d (%r)" % (what, v, _meant(c, fetch, fused, open_launch), c.lay)
    assert R.variant_launches() == plain, what
    _ran.add(v)


def _same_photons(got, want, what):
    if got.tobytes() != want.tobytes():
        rows = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1))
        raise AssertionError("%s: %d photons differ, first path %d: got %r want %r" % (what, len(rows), rows[0], got[rows[0]], want[rows[0]]))


def _unfused(c, table, fetch, ref, seed=SEED, stream=STREAM, first=FIRST, before_launch=None, what=""):
    want, segs_plain, segs_open = ref
    for n, open_launch, segs in ((N_PLAIN, False, segs_plain), (N_OPEN, True, segs_open)):
        t = R.TraceUnit(0, W, H, n_photons=n)
        t.set_fetch(fetch)
        t.set_wavelengths(_table(table)[0])

        def call():
            if before_launch:
                before_launch()
            if open_launch:
                t.render(c.scene, seed=seed, stream=stream, first_path_index=first)
            else:
                t.render_async(c.scene, seed=seed, stream=stream, first_path_index=first)
                t.sync()

        label = "%s %s fetch %d un-fused %s %s" % (c.name, table, fetch, "open" if open_launch else "plain", what)
        _held(c, fetch, False, open_launch, call, label)
        _same_photons(t.mapped_photons, want[:n], label)
        assert t.stats()[:2] == (n, segs), (label, t.stats()[:2], segs)


def _fused(c, table, fetch, ref):
    want, segs_plain, segs_open = ref
    for kind, n, open_launch, segs in (("fused", N_PLAIN, False, segs_plain), ("fused_sync", N_OPEN, True, segs_open), ("fused_begin", N_OPEN, True, segs_open)):
        t = R.TraceUnit(0, W, H, n_photons=64)
        t.set_fetch(fetch)
        t.set_wavelengths(_table(table)[0])
        p = R.PlotUnit(0, W, H)
        p.sync()

        def call():
            if kind == "fused":
                t.render_fused(c.scene, p, n, seed=SEED, stream=STREAM, first_path_index=FIRST)
                t.sync()
            elif kind == "fused_sync":
                t.render_fused_sync(c.scene, p, n, seed=SEED, stream=STREAM, first_path_index=FIRST)
            else:
                t.render_fused_begin(c.scene, p, n, seed=SEED, stream=STREAM, first_path_index=FIRST)
                p.sync()

        label = "%s %s fetch %d %s" % (c.name, table, fetch, kind)
        _held(c, fetch, True, open_launch, call, label)
        assert_film(p.tristimulus_buffer, W, H, want[:n].view(O.PHOTON_DTYPE), label)
        assert t.stats()[:2] == (n, segs), (label, t.stats()[:2], segs)


# ---- parity ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES + MORE_SCENES)
def test_photons_are_the_host_compiles_in_every_launch_kind(name):
    c = _case(name)
    for table in (TABLES if name in SCENES else TABLES[:1]):
        ref = _reference(name, table)
        assert (ref[0]["probability"] != 0).any(), (name, table)
        for fetch in FETCHES:
            _unfused(c, table, fetch, ref)
            _fused(c, table, fetch, ref)


def test_the_weighted_photons_are_the_unweighted_paths_of_their_wavelengths():
    """What the references above are: with the NULL-importance table every weight is 1 and the bins are 400 / 256 nm wide, so a
    path differs from the uniform draw's by its wavelength's rounding alone; with the CIE table the photons that carry light do so
    with W[bin_of(wavelength)] times the unweighted value of the very same path."""
    c = _case("demo")
    packed = _table("cie-0.1")[1]
    q, w = packed[:WO.M + 1], packed[WO.M + 1:]
    photons, _, values = c.host.render(W, H, packed, SEED, STREAM, FIRST, N_PLAIN)
    assert photons["probability"].tobytes() == (values * w[WO.bin_of(q, photons["wavelength"])]).astype(np.float32).tobytes()
    uniform = c.host.render(W, H, None, SEED, STREAM, FIRST, N_PLAIN)[0]
    null = _reference("demo", "null")[0][:N_PLAIN]
    assert null["x"].tobytes() == uniform["x"].tobytes() and np.abs(null["wavelength"] - uniform["wavelength"]).max() < 1.0e-3


def test_a_path_range_that_carries_into_the_high_counter_word():
    c = _case("demo")
    ref = _reference("demo", "cie-0.1", CARRY.seed, CARRY.stream, CARRY.first)
    assert RW.carry_position(CARRY.first, N_OPEN) is not None
    _unfused(c, "cie-0.1", R.FETCH_LDS, ref, seed=CARRY.seed, stream=CARRY.stream, first=CARRY.first, what="carry")


@pytest.mark.parametrize("name, fetch", [("demo", R.FETCH_LDS), ("edge-whole+1", R.FETCH_LDS), ("demo", R.FETCH_GLOBAL)], ids=["whole", "tables", "none"])
def test_unfused_on_poisoned_lds(name, fetch):
    c = _case(name)
    ref = _reference(name, "cie-0.1")
    for pattern in LP.PATTERNS:
        _unfused(c, "cie-0.1", fetch, ref, before_launch=lambda: LP.poison_lds(pattern), what="poisoned %#x" % pattern)


# ---- the unit's state ----------------------------------------------------------------------------------------------------------------

def test_set_and_reset():
    """A render after set_wavelengths(None) is the render before any table was set, byte for byte, on the plain instantiation; a set
    call is refused while a render begun on the unit has not ended; a table gives back what it held."""
    c = _case("demo")
    t = R.TraceUnit(0, W, H, n_photons=N_PLAIN)

    def render():       # (a plain launch: every one of them picks its instantiation, an appended call does not)
        t.render_async(c.scene, seed=SEED, stream=STREAM, first_path_index=FIRST)
        t.sync()
        return t.mapped_photons

    plain0, wl0 = R.variant_launches(), R.wavelength_variant_launches()
    before = render()
    assert before.tobytes() == c.host.render(W, H, None, SEED, STREAM, FIRST, N_PLAIN)[0].tobytes()
    assert R.wavelength_variant_launches() == wl0 and sum(R.variant_launches()) == sum(plain0) + 1
    t.set_wavelengths(_table("cie-0.1")[0])
    _same_photons(render(), _reference("demo", "cie-0.1")[0][:N_PLAIN], "with the table")
    t.render_begin(c.scene, seed=SEED, stream=STREAM, first_path_index=FIRST)
    with pytest.raises(R.RlError) as e:
        t.set_wavelengths(None)
    assert e.value.code == RL_E_STATE and "begun" in str(e.value)
    t.render_end()
    t.set_wavelengths(None)
    plain1, wl1 = R.variant_launches(), R.wavelength_variant_launches()
    assert render().tobytes() == before.tobytes()
    assert R.wavelength_variant_launches() == wl1 and sum(R.variant_launches()) == sum(plain1) + 1
    live = R.live_resources()
    table = R.WavelengthTable("cie", 0.25)
    assert tuple(R.live_resources()) == (live[0] + 1,) + tuple(live[1:])      # one allocation in the ledger
    table.close()
    assert R.live_resources() == live
    assert R.wavelength_importance_cie1931().tobytes() == WO.cie_importance().tobytes()


def test_open_launches_are_keyed_by_the_table():
    """Two units with the same table share an open launch; a third with another table and a fourth with none get launches of their
    own; all four results are those of separate plain launches."""
    c = _case("demo")
    n = 1 << 16
    tables = [_table("cie-0.1")[0], _table("cie-0.1")[0], _table("one-hot-1e-3")[0], None]
    units = [R.TraceUnit(i, W, H, n_photons=n) for i in range(4)]
    firsts = [i * n + 11 for i in range(4)]
    separate = []
    for u, table, first in zip(units, tables, firsts):
        u.set_wavelengths(table)
        u.render_async(c.scene, seed=3, stream=1, first_path_index=first)
        u.sync()
        separate.append(u.mapped_photons)
    assert separate[0].tobytes() != separate[2].tobytes()
    before = R.batch_histogram()
    for u, first in zip(units, firsts):
        u.render_begin(c.scene, seed=3, stream=1, first_path_index=first)
    for u in units:
        u.render_end()
    for i, u in enumerate(units):
        _same_photons(u.mapped_photons, separate[i], "unit %d" % i)
    after = R.batch_histogram()
    carried = {k: after.get(k, 0) - before.get(k, 0) for k in after if after.get(k, 0) != before.get(k, 0)}
    assert carried == {2: 1, 1: 2}, carried


# ---- the estimator -------------------------------------------------------------------------------------------------------------------

def test_unbiased_and_the_gain_is_what_the_cpu_run_showed():
    """64 x 36, demo scene, seed 1, 16 batches of 2^16 paths of stream 0, each observed by an error unit, without a table and with the
    CIE table at a share of 0.1.  The film totals of X, Y and Z agree within 5 of their combined standard errors (from the spread of
    the batches); the Y relative_error falls, by the ratio tools/wavelength_gain.py found on the CPU (tests/golden/wavelength_gain.json)
    to four digits: the photons are the host compile's, the films differ by the order of the atomics."""
    cfg = WO.GAIN
    w, h, n, k = cfg["w"], cfg["h"], cfg["n"], WO.GAIN_TEST_BUDGET
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavelength_gain.json")) as f:
        golden = json.load(f)
    assert golden["config"] == {key: (list(v) if isinstance(v, tuple) else v) for key, v in cfg.items()}
    scene = _case("demo").scene
    totals, rel = {}, {}
    for sampled in (False, True):
        trace, plot, gather, error = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h), R.GatherUnit(w, h), R.ErrorUnit(w, h)
        trace.set_wavelengths(R.WavelengthTable("cie", cfg["share"]) if sampled else None)
        per_batch = []
        for batch in range(k):
            trace.render_fused(scene, plot, n, seed=cfg["seed"], stream=cfg["stream"], first_path_index=batch * n)
            per_batch.append(plot.tristimulus_buffer.astype(np.float64).sum(axis=0))
            error.observe(plot, n)
            gather.accumulate(plot)
        totals[sampled] = np.array(per_batch)
        rel[sampled] = error.estimate(se=False)[0]["relative_error"]
    for i, name in enumerate("XYZ"):
        a, b = totals[False][:, i], totals[True][:, i]
        se = np.sqrt(a.var(ddof=1) / k + b.var(ddof=1) / k)
        print("%s: uniform %.6g importance %.6g diff %.3g combined se %.3g; batch spread %.4g -> %.4g" % (name, a.mean(), b.mean(), a.mean() - b.mean(), se, a.std(ddof=1), b.std(ddof=1)))
        assert abs(a.mean() - b.mean()) <= 5 * se, (name, a.mean(), b.mean(), se)
    ratio, want = rel[True] / rel[False], golden["ratio_relative_error"][str(k)]["Y"]
    print("Y relative_error: uniform %.6g importance %.6g ratio %.5f (CPU: %.5f)" % (rel[False], rel[True], ratio, want))
    assert ratio < 1 and want < 1
    assert abs(ratio / want - 1.0) < 5e-4, (ratio, want)      # four digits, as tests/test_gpu_adaptive.py holds its ratios


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False], ids=["fused", "un-fused"])
def test_the_app_renders_estimates_and_writes_an_image(tmp_path, fused):
    out = str(tmp_path / "image.ppm")
    plain, before = R.variant_launches(), R.wavelength_variant_launches()
    rgb, st, err = R.app_run_to_error(64, 36, 8, target_error=0.0, min_observations=2, photons_per_batch=1 << 16, fused=fused, output_ppm=out,
                                      wavelength_importance="cie")
    assert st["batches"] == 8 and st["paths"] == 8 << 16 and err["estimates"] >= 1 and 0 < err["at_end"]["relative_error"] < 1
    assert rgb.max() > 0 and open(out, "rb").read().startswith(b"P6\n64 36\n255\n")
    assert R.variant_launches() == plain and sum(R.wavelength_variant_launches()) > sum(before)
    # the same run without the table: the same image up to the noise of 2^19 paths, and a larger estimate of it
    rgb0, st0, err0 = R.app_run_to_error(64, 36, 8, target_error=0.0, min_observations=2, photons_per_batch=1 << 16, fused=fused)
    assert st0["paths"] == st["paths"] and sum(R.variant_launches()) > sum(plain)
    if err0["at_end"]["observations"] == err["at_end"]["observations"]:
        assert err["at_end"]["relative_error"] < err0["at_end"]["relative_error"]
    rgb1, _ = R.app_run(64, 36, 2, photons_per_batch=1 << 14, wavelength_importance="cie", wavelength_uniform_share=0.5)
    assert rgb1.max() > 0


def test_the_command_line_flag(tmp_path, capsys):
    out, cube = str(tmp_path / "image.png"), str(tmp_path / "cube.npy")
    before = R.wavelength_variant_launches()
    CLI.main(["--wavelength-importance", "cie", "--target-error", "0.0", "--min-observations", "2", "--output", out, "--width", "64", "--height", "36",
              "--batches", "8", "--photons-per-batch", "65536", "--spectral", cube, "--quiet"])
    told = capsys.readouterr().out
    assert "relative_error" in told and "wrote %s" % out in told and "spectral film" in told, told
    assert open(out, "rb").read().startswith(b"\x89PNG") and np.load(cube).shape == (81, 36, 64)
    ran = [a - b for a, b in zip(R.wavelength_variant_launches(), before)]
    assert sum(ran[4:8] + ran[12:16] + ran[20:24]) > 0 and sum(ran[0:4] + ran[8:12] + ran[16:20]) > 0     # the App's fused launches, --spectral's un-fused ones


def test_every_new_instantiation_ran():
    """(last in the module) All 24 WL instantiations, each held to the host compile above."""
    assert _ran == set(range(24)), sorted(set(range(24)) - _ran)
