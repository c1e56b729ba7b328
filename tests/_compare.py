"""How the tests of the ray and film calls compare: records byte for byte (padding and reserved fields included), path results for
their own consistency, a film against the CPU oracle's plot of the same photons, and two estimators by their means.  pytest does
not rewrite the asserts of this module, so each carries the values it compares."""
import numpy as np

import robigo_luculenta_amd as R
import _image_cases as IC
import _oracle as O

NONE = R.RL_OBJECT_NONE


def assert_same(got, want, what):
    """Two record arrays hold the same bytes; the message names the first row that differs."""
    if got.tobytes() != want.tobytes():
        rows = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %d: got %r want %r" % (what, len(rows), len(got), rows[0],
                                                                                          got[rows[0]], want[rows[0]]))


def assert_same_bytes(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape)
    if got.tobytes() != want.tobytes():
        rows = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d rays differ, first %d: got %d want %d" % (what, len(rows), len(got), rows[0], got[rows[0]],
                                                                                       want[rows[0]]))


def assert_consistent(res):
    """end and object agree with value: only a path that ended on a light carries a value, and only it names an object."""
    emit = res["end"] == R.RL_PATH_END_EMITTER
    bad = np.flatnonzero((res["object"] != NONE) != emit)
    assert not len(bad), ("object against end", bad[:8], res[bad[:8]])
    bad = np.flatnonzero(~emit & (res["value"] != 0))
    assert not len(bad), ("a value without an emitter", bad[:8], res[bad[:8]])
    bad = np.flatnonzero(~np.isin(res["end"], [R.RL_PATH_END_VOID, R.RL_PATH_END_EMITTER, R.RL_PATH_END_ROULETTE]))
    assert not len(bad), ("end", bad[:8], res[bad[:8]])
    bad = np.flatnonzero(~(res["segments"] >= 1))
    assert not len(bad), ("segments", bad[:8], res[bad[:8]])


def assert_film(got, w, h, photons, what=""):
    """`got` is the plot of `photons` onto a cleared buffer, by the project's tolerance."""
    want = O.plot(w, h, photons)
    scale = np.abs(want).max()
    img, k, s, exact = IC.splat(w, h, photons)
    assert IC.same_bits(img, want), (what, IC.first_difference(img, want))   # the restatement is the oracle's plot
    bad, excess = IC.splat_violations(got, want, k, s, exact)
    print("%s: max |got - want| %.3e (image max %.3e), per-pixel violations %d, worst excess %.3e"
          % (what, float(np.abs(got - want).max()) if got.size else 0.0, scale, len(bad), excess))
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6 * scale), what
    assert not len(bad), (what, bad[:8], excess)
    return want


def assert_means_agree(light_values, path_values, what):
    """|mean a - mean b| <= 5 combined standard errors, each from the samples themselves."""
    a, b = np.asarray(light_values, np.float64), np.asarray(path_values, np.float64)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("%s: light %.6g path %.6g diff %.3g se %.3g" % (what, a.mean(), b.mean(), a.mean() - b.mean(), se))
    assert a.mean() > 0 and b.mean() > 0, what
    assert abs(a.mean() - b.mean()) <= 5 * se, (what, a.mean(), b.mean(), se)
