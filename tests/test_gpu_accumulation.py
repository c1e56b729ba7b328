"""The accumulated XYZ film -- what the product hands its caller -- against the float64 sum of its photons (tests/_accumulation.py):
at depth (9,437,184 paths on 16x9 and 64x36: 65,536 and 4,096 paths per pixel, through 1,024 and 16 gathers, fused and un-fused),
and from the App's buffer.raw under many workers, two ranks on one GPU and a resume.  A batch that is plotted twice, never
gathered or cleared under a running splat moves these sums; the tonemapped u8 image the older App tests read does not see it.
A NaN or infinite photon is out of scope here (the plot tests cover it): every reference photon is finite."""
import numpy as np
import pytest

import _accumulation as A
import _image_cases as IC
import _oracle as O
from _boundary import _ocam

pytestmark = pytest.mark.gpu
PIN = 77                       # the slice of the reference records that is pinned to the oracle


@pytest.fixture(scope="module")
def R():
    import robigo_luculenta_amd as R
    assert R.device_count() > 0
    return R


@pytest.fixture(scope="module")
def scenes(R):
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    return R.Scene(objs, cam), O.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))


@pytest.fixture(scope="module")
def reference(R, scenes):
    """Per depth shape, computed once and left unchanged: the device's un-fused records that carry light (downloaded slice by slice),
    their terms, and per gather count the exact film, its bound and what a loss must show."""
    cache = {}

    def get(shape, gathers=None):
        w, h = shape
        if shape not in cache:
            path, records, pinned = A.device_records(R, scenes[0], w, h, pin=PIN)
            _, idx, terms = A.lit_terms(w, h, records)
            assert np.isfinite(terms).all() and (terms >= 0).all()
            cache[shape] = {"path": path, "records": records, "pinned": pinned, "idx": idx, "terms": terms}
        ref = cache[shape]
        if gathers is not None and gathers not in ref:
            k, s, exact = A.film_terms(w, h, ref["records"], ref["path"] // (A.PATHS // gathers), gathers)
            bound = A.accumulation_bound(k, s)
            exact = exact.sum(axis=0)
            _, want_srgb, _ = O.tonemap(exact.astype(np.float32), w, h)
            ref[gathers] = {"exact": exact, "bound": bound, "want_srgb": want_srgb,
                            "single": float(A.caught_if_lost(ref["terms"], ref["idx"], bound).mean()),
                            "launches": A.caught_if_group_lost(ref["terms"], ref["idx"], bound, ref["path"] // A.DEPTH_SPLITS[gathers][1],
                                                               A.PATHS // A.DEPTH_SPLITS[gathers][1])}
        return ref if gathers is None else ref[gathers]
    return get


@pytest.mark.parametrize("shape", A.DEPTH_SHAPES, ids=IC.shape_id)
def test_reference_records_are_the_oracles(reference, scenes, shape):
    """One 65,536-path slice of the records the depth films are held to, bit for bit; and about 10.5 % of the paths carry light."""
    w, h = shape
    ref = reference(shape)
    want, _ = scenes[1].render(w, h, A.DEPTH_SEED, A.DEPTH_STREAM, PIN * A.SLICE, A.SLICE, threads=8)
    assert ref["pinned"].tobytes() == want.tobytes()
    in_slice = (ref["path"] >= PIN * A.SLICE) & (ref["path"] < (PIN + 1) * A.SLICE)
    assert ref["records"][in_slice].tobytes() == want[want["probability"] != 0].tobytes()
    assert 0.09 < len(ref["path"]) / A.PATHS < 0.12 and np.all(np.diff(ref["path"]) > 0)


# what a loss must show, from the reference photons alone: the least share of photons whose single loss is certain to be caught
SINGLE_SHARE = {((16, 9), 1024): 0.65, ((64, 36), 1024): 0.90}


@pytest.mark.parametrize("gathers", [1024, 16])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape", A.DEPTH_SHAPES, ids=IC.shape_id)
def test_film_at_depth_is_the_f64_sum_of_its_photons(R, scenes, reference, shape, fused, gathers):
    """9,437,184 paths of seed 11 in G gathers (1,024 of one 9,216-path launch, 16 of nine 65,536-path launches); the fused cases
    run free, nothing waits for the device until the last gather is queued, and with G = 1024 two plot units take turns as the
    App's do.  Every component of the accumulated film lies within accumulation_bound of the exact sum, and its tonemapped sRGB
    within 1e-3 of the oracle's tonemap of the exact film."""
    w, h = shape
    ref = reference(shape, gathers)
    # the check has teeth: every launch's loss is certain to be caught, and (G = 1024) that of most single photons
    assert ref["launches"].all(), (int(ref["launches"].sum()), len(ref["launches"]))
    print("%dx%d G=%d: single-photon share %.3f" % (w, h, gathers, ref["single"]))
    if (shape, gathers) in SINGLE_SHARE:
        assert ref["single"] >= SINGLE_SHARE[(shape, gathers)]
    buffers = []
    record = (lambda j, px: buffers.append(px)) if (gathers == 1024 and not fused) else None
    g = A.run_depth_case(R, scenes[0], w, h, fused, gathers, on_plot_buffer=record)
    acc, comp = g.tristimulus_buffer, g.compensation_buffer
    bad, worst = A.violations(acc, ref["exact"], ref["bound"])
    print("  max |got - exact| / bound = %.3f" % worst)
    assert not len(bad), (len(bad), worst, bad[:4].tolist())
    tm = R.TonemapUnit(w, h)
    tm.tonemap(g)
    d = np.abs(tm.srgb_float()[0].astype(np.float64) - ref["want_srgb"])
    print("  max |delta sRGB| = %.2e" % d.max())
    assert d.max() <= 1e-3
    if record is not None:
        # the Kahan level alone, over the plot buffers the gathers were given
        assert len(buffers) == gathers
        want_acc, want_comp = np.zeros_like(acc), np.zeros_like(comp)
        for px in buffers:
            O.accumulate(want_acc, want_comp, px)
        assert acc.tobytes() == want_acc.tobytes() and comp.tobytes() == want_comp.tobytes()
        p64 = np.sum([b.astype(np.float64) for b in buffers], axis=0)      # P_j >= 0: also sum |P_j|
        bound = A.kahan_bound(gathers, p64)
        assert not len(A.violations(acc, p64, bound)[0])
        bad, worst = A.violations(A.naive_sum(buffers), p64, bound)
        print("  a float32 running sum of the same P_j: %d components beyond the Kahan-level bound, worst %.1f x" % (len(bad), worst))
        assert len(bad) >= 1


# ---- the App's raw film ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_film(scenes):
    """The oracle's photons of paths [first, first + count) of `ranks` streams (stream = stream0 + rank): k, S and the exact sum of
    the whole list (the partition into gathers is the scheduler's), and the segment total; once per configuration."""
    cache = {}

    def get(w, h, seed, ranks, count, first=0, stream0=0):
        key = (w, h, seed, ranks, count, first, stream0)
        if key not in cache:
            rendered = [scenes[1].render(w, h, seed, stream0 + r, first, count, threads=8) for r in range(ranks)]
            ph = np.concatenate([p for p, _ in rendered])
            k, s, exact = A.film_terms(w, h, ph, np.zeros(len(ph), np.int64), 1)
            cache[key] = (exact[0], A.accumulation_bound(k[0], s[0], ranks), sum(segs for _, segs in rendered))
        return cache[key]
    return get


def _raw_film(path, w, h):
    raw = np.fromfile(path, np.float32)
    assert raw.size == 2 * w * h * 3
    return raw[:w * h * 3].reshape(w * h, 3)


def _assert_app_film(st, acc, want, ranks, paths):
    exact, bound, segs = want
    assert st["paths"] == ranks * paths and st["segments"] == segs
    bad, worst = A.violations(acc, exact, bound)
    print("max |got - exact| / bound = %.3f" % worst)
    assert not len(bad), (len(bad), worst, bad[:4].tolist())


@pytest.mark.parametrize("fused, blocking, threads", [(False, False, 0), (False, True, 0), (True, False, 0), (True, True, 0), (True, False, 1)],
                         ids=["unfused", "unfused-blocking", "fused", "fused-blocking", "fused-one-thread"])
def test_app_with_many_workers_accumulates_every_batch_exactly_once(R, oracle_film, tmp_path, fused, blocking, threads):
    """600 batches of 1,024 paths through 16 workers' worth of units: buffer.raw after the drain and the last gather is the sum of
    the oracle's photons of paths [0, 600 * 1024) within the any-partition bound, under which the loss or doubling of any one
    batch is certain to show (tests/test_accumulation.py)."""
    w, h, n, batches = 64, 36, 1 << 10, 600
    raw = str(tmp_path / "buffer.raw")
    _, st = R.app_run(w, h, batches, concurrency=16, threads=threads, photons_per_batch=n, seed=9, fused=fused, blocking_trace=blocking,
                      checkpoint=raw)
    assert st["batches"] == batches
    _assert_app_film(st, _raw_film(raw, w, h), oracle_film(w, h, 9, 1, batches * n), 1, batches * n)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_app_with_two_ranks_on_one_gpu_accumulates_the_sum_of_two_streams(R, oracle_film, tmp_path, fused):
    w, h, n, batches = 96, 54, 1 << 14, 10
    raw = str(tmp_path / "buffer.raw")
    _, st = R.app_run(w, h, batches, concurrency=3, photons_per_batch=n, seed=5, fused=fused, devices=[0, 0], checkpoint=raw)
    assert st["batches"] == batches
    _assert_app_film(st, _raw_film(raw, w, h), oracle_film(w, h, 5, 2, batches * n), 2, batches * n)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_resumed_run_accumulates_all_twelve_batches(R, oracle_film, tmp_path, fused):
    """6 batches, then 6 more resumed from the first run's checkpoint: the film is the sum of all 12, each once."""
    w, h, n, batches = 80, 45, 1 << 13, 6
    raw = str(tmp_path / "buffer.raw")
    kw = dict(concurrency=2, photons_per_batch=n, seed=9, fused=fused, checkpoint=raw)
    _, st1 = R.app_run(w, h, batches, **kw)
    first = _raw_film(raw, w, h).copy()
    _assert_app_film(st1, first, oracle_film(w, h, 9, 1, batches * n), 1, batches * n)
    _, st2 = R.app_run(w, h, batches, resume=True, **kw)
    assert st2["next_batch"] == 2 * batches
    both = {"paths": st1["paths"] + st2["paths"], "segments": st1["segments"] + st2["segments"]}
    _assert_app_film(both, _raw_film(raw, w, h), oracle_film(w, h, 9, 1, 2 * batches * n), 1, 2 * batches * n)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_app_batches_across_2_32_paths_under_a_wide_seed_and_the_last_two_streams(R, oracle_film, tmp_path, fused):
    """12 batches of 4,096 paths from batch 2^20 - 6 on: the path indices [2^32 - 24576, 2^32 + 24576), so batch * photons_per_batch
    carries into the high counter word half way; a seed with a high word; two ranks on one GPU on streams 0xFFFFFFFE and
    0xFFFFFFFF.  buffer.raw is the sum of the oracle's photons of exactly those ranges and streams."""
    w, h, n, batches, first_batch = 64, 36, 1 << 12, 12, (1 << 20) - 6
    seed, stream = 0xA5A5A5A500000009, 0xFFFFFFFE
    assert first_batch * n == (1 << 32) - 24576 and (first_batch + batches) * n == (1 << 32) + 24576
    raw = str(tmp_path / "buffer.raw")
    _, st = R.app_run(w, h, batches, concurrency=3, photons_per_batch=n, seed=seed, stream=stream, fused=fused, devices=[0, 0],
                      checkpoint=raw, first_batch=first_batch)
    assert st["batches"] == batches and st["next_batch"] == (1 << 20) + 6
    _assert_app_film(st, _raw_film(raw, w, h), oracle_film(w, h, seed, 2, batches * n, first_batch * n, stream), 2, batches * n)
