"""tests/_feature_oracle.py itself, without a GPU: its splat for signed per-sample colours against _image_cases' splat of photons bit for
bit, its bound against float32 sums of signed terms taken in other orders, and the films' samples and the stats of records made by
hand."""
import numpy as np

import _feature_oracle as FO
import _image_cases as IC


def _records(n, seed):
    """Records no scene made: every kind, albedos of zero, screen positions on and beyond the film's edge."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, FO.FEATURE_DTYPE)
    rec["x"] = rng.uniform(-1, 1, n)
    rec["y"] = rng.uniform(-1, 1, n) / np.float32(16 / 9)
    rec["x"][:4], rec["y"][:4] = (-1, 1, 0.5, -0.25), (0.5625, -0.5625, 0, 0.25)
    rec["wavelength"] = rng.uniform(380, 780, n)
    rec["kind"] = rng.integers(0, 4, n)
    surface = (rec["kind"] == FO.EMITTER) | (rec["kind"] == FO.DIFFUSE)
    rec["albedo"] = np.where(surface, rng.uniform(0, 1, n) * (rng.random(n) < 0.9), 0)
    nrm = rng.normal(size=(n, 3))
    nrm[:8, 0], nrm[8:16, 2] = 0.0, -0.0
    rec["normal"] = np.where(surface[:, None], nrm / np.linalg.norm(nrm, axis=1, keepdims=True), 0)
    rec["depth"] = rng.uniform(0, 60, n) * (rec["kind"] != FO.VOID)
    rec["segments"] = rng.integers(1, 12, n)
    rec["object"] = np.where(surface, rng.integers(0, 300, n), FO.NONE)
    return rec


def test_the_albedo_film_is_the_plot_of_its_photons_bit_for_bit():
    for (w, h), n in (((16, 9), 5000), ((64, 36), 3000), ((1, 1), 10), ((37, 101), 999)):
        rec = _records(n, w)
        photons = FO.albedo_photons(rec)
        assert 0 < len(photons) < n and (photons["probability"] != 0).all()
        got, want = FO.film(w, h, rec, "albedo"), IC.splat(w, h, photons)
        for a, b, what in zip(got, want, ("image", "k", "S", "exact")):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (w, h, what)
        idx, terms = FO.splat_terms(w, h, *FO.film_samples(rec, "albedo"))
        idx2, terms2 = IC.splat_terms(w, h, photons)
        assert idx.tobytes() == idx2.tobytes() and terms.tobytes() == terms2.tobytes()
        assert FO.splat_bound(got[1], got[2]).tobytes() == IC.splat_bound(want[1], want[2]).tobytes()


def test_the_films_take_the_samples_the_contract_names():
    rec = _records(2000, 5)
    surface = (rec["kind"] == FO.EMITTER) | (rec["kind"] == FO.DIFFUSE)
    x, y, c = FO.film_samples(rec, "normal")
    assert len(x) == int(surface.sum()) and c.tobytes() == rec["normal"][surface].tobytes()
    x, y, c = FO.film_samples(rec, "aux")
    assert len(x) == len(rec) and (c[:, 0] == 1).all() and c[:, 1].tobytes() == rec["depth"].tobytes()
    assert (c[:, 2] == rec["segments"]).all() and c.dtype == np.float32
    x, y, c = FO.film_samples(rec, "albedo")
    assert len(x) == int((rec["albedo"] != 0).sum()) < int(surface.sum())
    # the weights of a sample add up to one: the aux film's first component sums to the number of paths
    img, k, s, exact = FO.film(64, 36, rec, "aux")
    assert abs(exact[:, 0].sum() - len(rec)) < 1e-3 * len(rec)


def test_the_bound_holds_for_signed_terms_in_any_order():
    """The normal film's terms have both signs.  Sums of the same float32 terms in shuffled orders, each add rounded to float32,
    stay within (k - 1) 2^-24 S of the exact sum on every pixel component, and a component with at most two terms has one value."""
    w, h = 16, 9
    rec = _records(6000, 11)
    x, y, colours = FO.film_samples(rec, "normal")
    assert (colours < 0).any() and (colours > 0).any()
    idx, terms = FO.splat_terms(w, h, x, y, colours)
    want, k, s, exact = FO.splat(w, h, x, y, colours)
    assert k.max() > 100 and (np.abs(exact) < 0.5 * s)[k > 10].any()      # cancellation: the bound is in S, not in the sum
    flat_idx, flat_terms = idx.reshape(-1), terms.reshape(-1, 3)
    rng = np.random.default_rng(3)
    for order in (np.arange(len(flat_idx))[::-1], rng.permutation(len(flat_idx)), np.argsort(flat_terms[:, 0], kind="stable")):
        img = np.zeros((w * h, 3), np.float32)
        np.add.at(img, flat_idx[order], flat_terms[order])
        bad, excess = FO.splat_violations(img, want, k, s, exact)
        assert not len(bad), (bad[:8], excess)
    # a film that lost one sample is caught
    img, _, _, _ = FO.splat(w, h, x[1:], y[1:], colours[1:])
    assert len(FO.splat_violations(img, want, k, s, exact)[0])
    # few terms: the bits
    x2, y2, c2 = x[:3], y[:3], colours[:3]
    want2, k2, s2, exact2 = FO.splat(320, 180, x2, y2, c2)
    assert k2.max() <= 2 and not len(FO.splat_violations(want2, want2, k2, s2, exact2)[0])
    off = want2.copy()
    off[np.unravel_index(np.argmax(k2), k2.shape)] *= np.float32(1 + 2.0 ** -23)
    assert len(FO.splat_violations(off, want2, k2, s2, exact2)[0]) == 1


def test_stats_are_counted_from_the_records_and_add_up():
    rec = _records(1000, 2)
    whole, a, b = FO.stats_of(rec), FO.stats_of(rec[:333]), FO.stats_of(rec[333:])
    assert whole["paths"] == 1000 and sum(whole["kinds"]) == 1000 and whole["segments"] == int(rec["segments"].sum())
    assert FO.add_stats(a, b) == whole
    f = FO.Features(rec)
    assert f.prefix(333)[1] == a and f.span(333, 1000) == b and f.prefix(333)[0].tobytes() == rec[:333].tobytes()
