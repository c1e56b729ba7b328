"""CPU proofs of tests/_image_cases.py: the shapes reach the kernel paths they name, the numpy splat is the oracle's,
the exposure fixtures can see a dropped, doubled or re-associated pixel, and the edge-path fixture holds what it claims."""
import numpy as np
import pytest

import _image_cases as IC
import _oracle as O


def test_shapes_reach_every_exposure_and_gather_path():
    ex = [IC.exposure_path(w * h) for w, h in IC.SHAPES]
    assert {e["tail"] for e in ex if e["tiles"] == 1} == set(range(16))
    assert {e["tail"] for e in ex if e["tiles"] > 1} >= {0, 1, 15}
    n16 = {(e["tiles"] > 1, min(e["n16"], 3), e["n16"] % 2) for e in ex}
    for multi in (False, True):
        # n16 = 0, 1, 2, odd >= 3, even >= 4, with one tile (no prefetch) and with several
        assert {(multi, 0, 0), (multi, 1, 1), (multi, 2, 0), (multi, 3, 1), (multi, 3, 0)} <= n16, (multi, n16)
    g = [IC.gather_path(w * h) for w, h in IC.SHAPES]
    assert {x["tail"] for x in g} == {0, 1, 2, 3}
    assert any(x["n4"] == 0 for x in g)                                      # the tail alone
    assert {(w * h) % 4 for w, h in IC.SHAPES if w > 1 and h > 1} == {0, 1, 2, 3}
    assert {(1, 4097), (4097, 1), (37, 101), (3, 5), (1919, 1079), (1279, 719), (1920, 1080), (3840, 2160)} <= set(IC.SHAPES)
    for n in range(1, 81):
        assert (n, 1) in IC.SHAPES and (1, n) in IC.SHAPES
    cov = IC.coverage()
    assert cov[(1, 1)] == ("1 (no prefetch) tile(s); last: no 16-pixel reads, tail loop of 1", "no float4 body, scalar tail of 3")
    assert cov[(2049, 1)][0] == "2 tile(s); last: no 16-pixel reads, tail loop of 1"


def test_tristimulus_restatement_is_the_oracles_at_the_range_ends():
    wl = np.concatenate([np.float32([380.0, 780.0, 379.99997, 780.00006, 375.0, 785.0, 379.0, 781.0, 400.0, 555.5]),
                         np.random.default_rng(0).uniform(370, 790, 2000).astype(np.float32)])
    got = IC.tristimulus(wl)
    want = np.zeros_like(got)
    for i, w in enumerate(wl):
        O.lib().oracle_tristimulus(float(w), O.ptr(want[i]))
    assert IC.same_bits(got, want), IC.first_difference(got, want)
    assert got[1].any()                                                      # 780 nm: index 80, remainder 0


@pytest.fixture(scope="module")
def oscene():
    objs, cam = O.demo_scene_desc()
    return O.Scene(objs, cam)


@pytest.mark.parametrize("shape", [(1, 1), (2, 1), (1, 2), (3, 5), (1, 17), (37, 101), (101, 37), (333, 127), (64, 36)],
                         ids=IC.shape_id)
def test_numpy_splat_is_the_oracle_plot_bit_for_bit(oscene, shape):
    w, h = shape
    ph, _ = oscene.render(w, h, 3, 1, 1000, 1 << 14, threads=4)
    img, k, s, exact = IC.splat(w, h, ph)
    want = O.plot(w, h, ph)
    assert IC.same_bits(img, want), IC.first_difference(img, want)
    assert img.any() and k.max() >= 3
    # k_p and S_p: zero terms are left out; S_p bounds the sum
    assert np.all(np.abs(img.astype(np.float64)) <= s * (1 + 1e-5) + 1e-30)
    assert np.all((k == 0) == (s == 0))


def test_splat_at_the_border_follows_the_oracle_and_rendered_photons_stay_inside():
    """Images one pixel wide or tall, photons at x = +-1 and y = +-1 / aspect, and (synthetic) photons just beyond them,
    whose clamped weights cx, cy go negative: the restatement follows the oracle everywhere.  A rendered photon never
    lies beyond: |fl(fl(d / aspect) * aspect)| <= 1 for every draw |d| <= 1, so its weights stay in [0, 1]."""
    rng = np.random.default_rng(5)
    f = np.float32
    for w, h in [(1, 1), (1, 7), (7, 1), (3, 5), (37, 101), (101, 37)]:
        n = 4096
        ph = np.zeros(n, O.PHOTON_DTYPE)
        aspect = f(w) / f(h)
        ends = f([-1.0, 1.0, -0.99999994, 0.99999994, -1.0000001, 1.0000001])
        ph["x"] = rng.choice(np.append(ends, f(0.0)), n)
        ph["y"] = rng.choice(ends, n) / aspect
        ph["x"][::3] = rng.uniform(-1, 1, len(ph[::3])).astype(np.float32)
        ph["wavelength"] = rng.choice(f([380.0, 780.0, 555.0, 400.5]), n)
        ph["probability"] = rng.uniform(0, 2, n).astype(np.float32)
        img, k, s, exact = IC.splat(w, h, ph)
        want = O.plot(w, h, ph)
        assert IC.same_bits(img, want), (w, h, IC.first_difference(img, want))
        _, terms = IC.splat_terms(w, h, ph)
        assert (terms < 0).any() == (h > 1 or w > 1)                         # beyond the border: negative weights
        for d in (f(1.0), f(-1.0)):
            assert abs(f(d / aspect) * aspect) <= 1.0


def test_splat_bound_is_exact_for_two_terms_and_catches_a_missing_dim_pixel():
    img = np.float32([[1.0, 0, 0], [3.0, 0, 0]])
    k = np.array([[2, 0, 0], [5, 0, 0]])
    s = np.array([[1.0, 0, 0], [3.0, 0, 0]])
    exact = img.astype(np.float64)
    assert not len(IC.splat_violations(img, img, k, s, exact)[0])
    off = img.copy()
    off[0, 0] = np.nextafter(off[0, 0], np.float32(2))                       # k = 2: one ulp is too much
    assert len(IC.splat_violations(off, img, k, s, exact)[0]) == 1
    off = img.copy()
    off[1, 0] = np.nextafter(off[1, 0], np.float32(4))                       # k = 5: one ulp is within 4 * 2^-24 * 3
    assert not len(IC.splat_violations(off, img, k, s, exact)[0])
    off[1, 0] = np.float32(3.0) + np.float32(3 * 2.0 ** -21)                  # ... three ulps are not
    assert len(IC.splat_violations(off, img, k, s, exact)[0]) == 1
    off[1, 0] = 0.0                                                          # a missing dim pixel fails whatever the image's maximum
    assert len(IC.splat_violations(off, img, k, s, exact)[0]) == 1


def test_oracle_splat_is_within_the_bound_of_the_exact_sum(oscene):
    """The bound holds for the oracle's own order (so for any order), on rendered photons at a crowded small image."""
    ph, _ = oscene.render(17, 9, 2, 0, 0, 1 << 15, threads=4)
    img, k, s, exact = IC.splat(17, 9, ph)
    assert k.max() > 100
    assert not len(IC.splat_violations(img, img, k, s, exact)[0])
    assert not len(IC.splat_violations(O.plot(17, 9, ph[::-1].copy()), img, k, s, exact)[0])  # the reverse order


def test_same_bits():
    a = np.float32([1.0, np.nan, 0.0, -0.0])
    b = a.copy()
    b[1] = -np.float32(np.nan)                                               # NaNs of another sign: equal
    assert IC.same_bits(a, b)
    c = a.copy()
    c[3] = 0.0                                                               # -0 against +0: a difference
    assert not IC.same_bits(a, c)
    d = a.copy()
    d[0] = np.nan                                                            # NaN against a number: a difference
    assert not IC.same_bits(a, d)
    assert IC.same_bits(np.uint8([1, 2]), np.uint8([1, 2])) and not IC.same_bits(np.uint8([1, 2]), np.uint8([1, 3]))


# (class, kernel error) pairs that a class cannot see at some sizes, with the reason.  Every other pair must be seen at every
# size of 2048 pixels or more; a listed pair must indeed go unseen at one size at least (else it is not listed).
INSENSITIVE = {
    ("lone_tail", "pairwise"): "one nonzero term: every summation order gives the same sum",
    ("constant", "dropped"): "where the variance rounds negative max_intensity is NaN either way; elsewhere one value "
                             "more or less can round away in sum / n",
    ("constant", "doubled"): "where the variance rounds negative max_intensity is NaN either way",
    ("constant", "pairwise"): "where the variance rounds negative max_intensity is NaN in every order",
    ("yy_overflow", "dropped"): "sum(Y * Y) = inf with or without the last pixel: max_intensity stays inf",
    ("yy_overflow", "doubled"): "sum(Y * Y) = inf with or without the last pixel: max_intensity stays inf",
    ("yy_overflow", "pairwise"): "sum(Y * Y) = inf in every order: max_intensity stays inf",
    ("sum_overflow", "dropped"): "sum(Y) = inf already: the variance is inf - inf = NaN either way",
    ("sum_overflow", "doubled"): "sum(Y) = inf already: the variance is inf - inf = NaN either way",
    ("sum_overflow", "pairwise"): "sum(Y) = inf in every order: NaN either way",
    ("nonfinite_y", "dropped"): "a non-finite Y makes every variant NaN or inf",
    ("nonfinite_y", "doubled"): "a non-finite Y makes every variant NaN or inf",
    ("nonfinite_y", "pairwise"): "a non-finite Y makes every variant NaN or inf",
}
# Single sizes where the tree and the chain happen to round to the same max_intensity (they must indeed do so).
COINCIDENT = {("loguniform", "pairwise", (2081, 1)), ("denormal", "pairwise", (2048, 1)), ("denormal", "pairwise", (2064, 1))}
SENSITIVITY_SHAPES = [s for s in IC.SHAPES if s[0] * s[1] >= IC.EXPOSURE_TILE]


@pytest.mark.parametrize("cls", sorted(IC.XYZ_CLASSES))
def test_exposure_fixtures_see_a_dropped_doubled_or_reassociated_pixel(cls):
    """At every shape of 2048 pixels or more the oracle's max_intensity differs from the value a kernel would produce
    that dropped the last pixel, added it twice, or summed pairwise -- except where INSENSITIVE says by name why not."""
    unseen = {name: [] for name in ("dropped", "doubled", "pairwise")}
    for shape in SENSITIVITY_SHAPES:
        v = IC.exposure_variants(IC.XYZ_CLASSES[cls](shape, 1))
        for name in unseen:
            same = IC.same_bits(v[name], v["sequential"])
            if (cls, name, shape) in COINCIDENT:
                assert same, "%s %s at %s: no longer a coincidence, drop it from COINCIDENT" % (cls, name, shape)
            elif same:
                unseen[name].append((shape, v["sequential"]))
    for name, where in unseen.items():
        if (cls, name) in INSENSITIVE:
            assert where, "%s sees a %s pixel at every size: drop it from INSENSITIVE" % (cls, name)
        else:
            assert not where, (name, where[:6])


@pytest.mark.parametrize("shape", [(2047, 1), (4097, 1), (37, 101), (333, 127), (1919, 1079)], ids=IC.shape_id)
def test_numpy_exposure_is_the_oracles(shape):
    for cls, fn in IC.XYZ_CLASSES.items():
        xyz = fn(shape, 1)
        _, _, mx = O.tonemap(xyz, shape[0], shape[1])
        assert IC.same_bits(np.float32(mx), IC.exposure_variants(xyz)["sequential"]), cls


def test_synthetic_classes_hold_what_they_claim():
    shape = (1919, 1079)
    mx = {}
    for cls, fn in IC.XYZ_CLASSES.items():
        xyz = fn(shape, 1)
        assert xyz.dtype == np.float32 and xyz.shape == (shape[0] * shape[1], 3)
        assert IC.same_bits(xyz, fn(shape, 1)) and not IC.same_bits(xyz, fn(shape, 2)) or cls == "constant", cls
        mx[cls] = IC.exposure_variants(xyz)["sequential"]
    assert np.isinf(mx["yy_overflow"]) and np.isnan(mx["sum_overflow"]) and not np.isfinite(mx["nonfinite_y"])
    assert np.isfinite(mx["loguniform"]) and np.isfinite(mx["outliers"]) and np.isfinite(mx["denormal"])
    d = IC.xyz_denormal(shape, 1)
    assert np.all((d > 0) & (d < np.finfo(np.float32).tiny))
    nf = IC.xyz_negative_nonfinite(shape, 1)
    assert np.isnan(nf).any() and np.isposinf(nf).any() and np.isneginf(nf).any() and (nf < 0).any()
    assert np.isfinite(nf[:, 1]).all() and (np.signbit(nf) & (nf == 0)).any()
    for n in (1, 17, 2048 + 33, 2047):
        lt = IC.xyz_lone_tail((n, 1), 1)
        (lit,) = np.flatnonzero(lt[:, 1])
        tail = IC.exposure_path(n)["tail"]
        assert lit >= n - max(tail, 1)
    # a constant image whose variance rounds negative (NaN) is among the seeds the GPU test uses
    nan_seen = any(np.isnan(IC.exposure_variants(IC.xyz_constant(s, 1))["sequential"]) for s in IC.SHAPES)
    assert nan_seen


def test_kahan_states_are_adversarial():
    acc, comp, pxs = IC.kahan_states((333, 127), 1)
    assert comp.any() and not np.isnan(comp).any()
    a, c = acc.copy(), comp.copy()
    for px in pxs:
        O.accumulate(a, c, px)
    fin = np.isfinite(a) & np.isfinite(c)
    assert (c[fin] != 0).mean() > 0.5                                         # the compensation carries low bits
    assert np.isnan(a).any() and (a == 0).any()                               # non-finite tails and exact cancellation
    # the tail values sit at the end of the buffer: in the gather kernel's scalar tail when (3 n) & 3 != 0
    assert not np.isfinite(np.concatenate([p.reshape(-1)[-9:] for p in pxs])).all()


def test_edge_path_fixture_holds_what_it_claims(oscene):
    entries = IC.load_edge_paths()
    assert 6 <= len(entries) <= 32
    seen = 0
    for seed, stream, path, flags, reaches in entries:
        words = np.zeros(4, np.uint32)
        O.lib().oracle_rng_block(seed, stream, path, 0, O.ptr(words))
        c = O.math_f32("closed01", words[:3].view(np.float32)).reshape(1, 3)
        assert IC.edge_flags(c)[0] == flags and flags != 0, (seed, stream, path)
        ph, _ = oscene.render(*IC.EDGE_SHAPES[0], seed, stream, path, 1)
        assert int(ph["probability"][0] > 0) == reaches, (seed, stream, path)
        if flags & (IC.EDGE_X_MINUS | IC.EDGE_X_PLUS):
            assert abs(ph["x"][0]) == 1.0
        if flags & IC.EDGE_WL_380:
            assert ph["wavelength"][0] == 380.0
        if flags & IC.EDGE_WL_780:
            assert ph["wavelength"][0] == 780.0
        seen |= flags
    assert seen == sum(IC.EDGE_NAMES)                                        # every end of every draw
    assert any(e[4] for e in entries)                                        # and some of them reach the splat
