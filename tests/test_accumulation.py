"""CPU proofs of tests/_accumulation.py: the terms are IC.splat's, the any-partition bound dominates every partition, the oracle's own
plot + Kahan accumulation passes the bound and a sum without the compensation does not, and under the App's conditions a lost or
doubled batch is certain to be seen."""
import numpy as np
import pytest

import _accumulation as A
import _image_cases as IC
import _oracle as O


@pytest.fixture(scope="module")
def oscene():
    objs, cam = O.demo_scene_desc()
    return O.Scene(objs, cam)


@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (1, 2), (3, 5), (1, 17), (37, 101), (101, 37), (64, 36)], ids=IC.shape_id)
def test_film_terms_are_the_splats_k_s_and_exact_sum(oscene, shape):
    w, h = shape
    ph, _ = oscene.render(w, h, 3, 1, 1000, 1 << 14, threads=4)
    _, k, s, exact = IC.splat(w, h, ph)
    k1, s1, e1 = A.film_terms(w, h, ph, np.zeros(len(ph), np.int64))
    assert k1.shape == (1, w * h, 3) and k.max() >= 3
    assert np.array_equal(k1[0], k)
    # two float64 sums of the same terms, each within (k - 1) 2^-53 S of the true one
    tol = 2 * (k - 1).clip(0) * 2.0 ** -53 * s
    assert np.all(np.abs(s1[0] - s) <= tol) and np.all(np.abs(e1[0] - exact) <= tol)
    # split over intervals: the intervals' k, S and sums add up to the whole list's
    interval = np.arange(len(ph)) % 5
    k5, s5, e5 = A.film_terms(w, h, ph, interval)
    assert k5.shape == (5, w * h, 3) and np.array_equal(k5.sum(axis=0), k)
    assert np.all(np.abs(s5.sum(axis=0) - s) <= 2 * tol) and np.all(np.abs(e5.sum(axis=0) - exact) <= 2 * tol)
    for j in (0, 4):                                                         # and each interval is the splat of its own photons
        _, kj, sj, ej = IC.splat(w, h, ph[interval == j])
        assert np.array_equal(k5[j], kj) and np.all(np.abs(e5[j] - ej) <= tol) and np.all(np.abs(s5[j] - sj) <= tol)
    # the photons without light add nothing: the terms of the lit ones alone are the film's
    lit, idx, terms = A.lit_terms(w, h, ph)
    assert 0 < len(lit) < len(ph) and not ph["probability"][np.setdiff1d(np.arange(len(ph)), lit)].any()
    assert idx.shape == (len(lit), 4) and terms.shape == (len(lit), 4, 3) and terms.dtype == np.float32


def test_any_partition_bound_is_at_least_every_partitions(oscene):
    w, h = 16, 9
    ph, _ = oscene.render(w, h, 11, 0, 0, 1 << 16, threads=4)
    k, s, _ = A.film_terms(w, h, ph, np.zeros(len(ph), np.int64))
    for ranks in (1, 2):
        whole = A.accumulation_bound(k[0], s[0], ranks)
        assert np.array_equal(whole, A.accumulation_bound(k, s, ranks)) and (whole > 0).all()
        rng = np.random.default_rng(7)
        for g in (2, 16, 1024):
            for interval in (rng.integers(0, g, len(ph)), np.arange(len(ph)) * g // len(ph), np.sort(rng.integers(0, g, len(ph)))):
                kj, sj, _ = A.film_terms(w, h, ph, interval, g)
                part = A.accumulation_bound(kj, sj, ranks)
                assert np.all(part <= whole * (1 + 1e-12))
                assert (part < whole).any()                                  # and the partition is worth knowing
    # its parts: one photon alone on a pixel is held to Kahan's 2u (the 65,536 gathers cost under 1 % of it), two ranks add one u
    one = A.accumulation_bound(np.ones((1, 3), np.int64), np.ones((1, 3)))
    two = A.accumulation_bound(np.ones((1, 3), np.int64), np.ones((1, 3)), ranks=2)
    assert np.all(one >= 2 * A.U) and np.all(one <= 2.02 * A.U) and np.allclose(two - one, A.U, rtol=1e-5, atol=0)


def _oracle_intervals(oscene, w, h, intervals, n):
    ph, _ = oscene.render(w, h, 11, 0, 0, intervals * n, threads=8)
    buffers = [O.plot(w, h, ph[j * n:(j + 1) * n]) for j in range(intervals)]
    return ph, buffers


def test_the_oracles_own_plot_and_accumulate_stay_within_the_bound(oscene):
    """The reference alone passes: O.plot per interval, O.accumulate over the intervals, on a crowded small film."""
    w, h, intervals, n = 16, 9, 64, 4096
    ph, buffers = _oracle_intervals(oscene, w, h, intervals, n)
    acc, comp = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    for px in buffers:
        O.accumulate(acc, comp, px)
    k, s, exact = A.film_terms(w, h, ph, np.arange(len(ph)) // n, intervals)
    assert k.max() > 100 and (k.sum(axis=0) > 0).all()
    bad, worst = A.violations(acc, exact.sum(axis=0), A.accumulation_bound(k, s))
    assert not len(bad), (len(bad), worst)
    bad, worst = A.violations(acc, exact.sum(axis=0), A.accumulation_bound(k.sum(axis=0), s.sum(axis=0)))
    assert not len(bad), (len(bad), worst)
    # the Kahan level on its own: the accumulator against the float64 sum of the plot buffers it was given
    p64 = np.sum([b.astype(np.float64) for b in buffers], axis=0)
    assert not len(A.violations(acc, p64, A.kahan_bound(intervals, p64))[0])
    # a film that lacks one interval, or holds it twice, does not pass
    for wrong in (acc - buffers[5], acc + buffers[5]):
        assert len(A.violations(wrong.astype(np.float32), exact.sum(axis=0), A.accumulation_bound(k, s))[0])


def test_a_running_sum_without_compensation_breaks_the_kahan_level_bound_at_depth(oscene):
    """G = 1024 plot buffers of the spread the rendered ones have (each a rendered buffer times a factor of 0.5 .. 2): Kahan
    holds (2u + 3 G u^2) sum |P_j|, the plain float32 running sum does not."""
    w, h, intervals, n, G = 16, 9, 64, 4096, 1024
    _, rendered = _oracle_intervals(oscene, w, h, intervals, n)
    rng = np.random.default_rng(11)
    buffers = [(rendered[j % intervals] * rng.uniform(0.5, 2.0, (w * h, 1))).astype(np.float32) for j in range(G)]
    p64 = np.sum([b.astype(np.float64) for b in buffers], axis=0)            # P_j >= 0: this is sum |P_j| too
    bound = A.kahan_bound(G, p64)
    acc, comp = np.zeros((w * h, 3), np.float32), np.zeros((w * h, 3), np.float32)
    for px in buffers:
        O.accumulate(acc, comp, px)
    assert not len(A.violations(acc, p64, bound)[0])
    bad, worst = A.violations(A.naive_sum(buffers), p64, bound)
    assert len(bad) >= 1 and worst > 1.0
    print("naive float32 sum over %d gathers: %d of %d components beyond the Kahan-level bound, worst %.1f x" % (G, len(bad), p64.size, worst))


@pytest.fixture(scope="module")
def app_photons(oscene):
    """The oracle's photons of one RNG stream of the App configuration below, rendered once."""
    cache = {}

    def get(stream):
        if stream not in cache:
            cache[stream] = oscene.render(64, 36, 9, stream, 0, 600 * 1024, threads=8)[0]
        return cache[stream]
    return get


@pytest.mark.parametrize("ranks, single_share", [(1, 0.85), (2, 0.80)])
def test_under_the_apps_conditions_every_lost_batch_is_caught(app_photons, ranks, single_share):
    """64x36, 600 batches of 1,024 paths, seed 9, stream = rank, the partition into gathers unknown: every batch's loss (or
    doubling) is certain to break the any-partition bound, and so is the loss of most single photons (measured on the oracle's
    photons: 0.891 of them with one stream, 0.838 with two)."""
    w, h, n, batches = 64, 36, 1024, 600
    ph = np.concatenate([app_photons(r) for r in range(ranks)])
    batch = np.concatenate([np.arange(batches * n) // n + r * batches for r in range(ranks)])
    k, s, _ = A.film_terms(w, h, ph, np.zeros(len(ph), np.int64))
    bound = A.accumulation_bound(k[0], s[0], ranks)
    lit, idx, terms = A.lit_terms(w, h, ph)
    caught = A.caught_if_group_lost(terms, idx, bound, batch[lit], ranks * batches)
    assert caught.sum() == len(caught) == ranks * batches
    share = A.caught_if_lost(terms, idx, bound).mean()
    print("ranks %d: %d of %d batches, single-photon share %.3f" % (ranks, caught.sum(), len(caught), share))
    assert share >= single_share
