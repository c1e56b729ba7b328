"""Inputs of the relight film's tests (tests/test_relight.py, tests/test_gpu_relight.py, tools/relight_gain.py): shapes, node and
group counts, synthetic records and tables, films, gains and matrices, and the re-trace case, all deterministic.  Test-only."""
import functools

import numpy as np

import _relight_oracle as RO
import _spectral_cases as SC

# (w, h): one pixel; one pixel high; a small square; the demo's aspect; odd sizes over several workgroups of pixels
SHAPES = [(1, 1), (5, 1), (3, 3), (16, 9), (33, 17)]
NODES = [2, 5, 81]
GROUPS = [1, 3, 16]
N_OBJECTS = 41                                  # of the synthetic tables: no multiple of anything
FILMS = ["loguniform", "with_zeros", "nonfinite"]
GAINS = ["ones", "null", "signed", "solo", "nonfinite"]
MATRICES = ["cie", "signed"]
# the re-trace case: the demo's sun sphere from 6504 K, intensity 1 to 3200 K, intensity 0.5
SUN, SUN_FROM, SUN_TO = 0, (6504.0, 1.0), (3200.0, 0.5)
RETRACE = dict(w=64, h=36, n=1 << 16, seed=1, stream=0, first=0)


def combinations():
    return [(w, h, n, g) for (w, h) in SHAPES for n in NODES for g in GROUPS]


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def table(n_groups, n_objects=N_OBJECTS):
    """One byte per object: every group from 0 to n_groups - 1 at least once where there is room, DROP on about a fifth."""
    g = np.random.default_rng([_seed("table"), n_groups, n_objects])
    out = g.integers(0, n_groups, n_objects).astype(np.uint8)
    out[g.random(n_objects) < 0.2] = RO.DROP
    where = g.permutation(n_objects)
    out[where[:min(n_groups, n_objects - 1)]] = np.arange(min(n_groups, n_objects - 1))
    out[where[-1]] = RO.DROP
    return out


def synthetic_records(w, h, n_objects=N_OBJECTS, n=3000):
    """(samples, results) no renderer makes: _spectral_cases.synthetic_photons' x, y, wavelength and value (edge wavelengths, borders,
    zero and negative values, NaN and infinities), an object over 0 .. n_objects - 1 and, on a tenth, n_objects - 1, n_objects,
    n_objects + 1, 255, 256, 2^31, 2^32 - 2 and RL_OBJECT_NONE; ray, segments and end hold noise, which nothing reads."""
    ph = SC.synthetic_photons(w, h, n)
    g = np.random.default_rng([_seed("records"), w, h, n_objects])
    samples, results = np.zeros(n, RO.SAMPLE_DTYPE), np.zeros(n, RO.RESULT_DTYPE)
    samples["x"], samples["y"], samples["ray"]["wavelength"] = ph["x"], ph["y"], ph["wavelength"]
    samples["ray"]["origin"], samples["ray"]["direction"] = g.normal(size=(n, 3)), g.normal(size=(n, 3))
    samples["reserved0"], samples["reserved1"] = g.integers(0, 1 << 32, n, dtype=np.uint64), g.integers(0, 1 << 32, n, dtype=np.uint64)
    results["value"] = ph["probability"]
    results["object"] = g.integers(0, n_objects, n)
    odd = np.array([n_objects - 1, n_objects, n_objects + 1, 255, 256, 1 << 31, RO.NONE - 1, RO.NONE], np.uint32)
    rows = g.permutation(n)[:n // 10]
    results["object"][rows] = odd[np.arange(len(rows)) % len(odd)]
    results["segments"], results["end"] = g.integers(0, 1 << 32, n, dtype=np.uint64), g.integers(0, 1 << 32, n, dtype=np.uint64)
    return samples, results


def film(kind, w, h, n_nodes, n_groups):
    """(n_groups, n_nodes, h, w) float32 to upload: _spectral_cases.film of as many planes."""
    return SC.film(kind, w, h, n_nodes * n_groups).reshape(n_groups, n_nodes, h, w)


def gains(kind, n_groups, n_nodes):
    """(n_groups, n_nodes) float32, or None for "null"."""
    g = np.random.default_rng([_seed(kind), n_groups, n_nodes])
    if kind == "null":
        return None
    if kind == "ones":
        return np.ones((n_groups, n_nodes), np.float32)
    if kind == "solo":                                   # the last group alone
        out = np.zeros((n_groups, n_nodes), np.float32)
        out[-1] = 1.0
        return out
    out = g.uniform(-2.0, 2.0, (n_groups, n_nodes)).astype(np.float32)
    if kind == "nonfinite":
        flat = out.reshape(-1)
        flat[g.permutation(len(flat))[:4]] = np.array([np.nan, np.inf, -np.inf, 0.0], np.float32)[:min(4, len(flat))]
    return out


def matrix(kind, n_nodes):
    return SC.matrix(kind, n_nodes)


def demo_descriptions():
    """(objects A, objects B, camera): the demo scene, and the demo scene with the sun sphere at SUN_TO."""
    import _oracle as O
    objs, cam = O.demo_scene_desc()
    assert objs["material_kind"][SUN] == RO.BLACK_BODY and tuple(objs["m"][SUN][:2]) == SUN_FROM
    changed = objs.copy()
    changed["m"][SUN][:2] = SUN_TO
    return objs, changed, cam


@functools.lru_cache(maxsize=None)
def retrace():
    """The re-trace case on the CPU oracles: (samples, results A, results B) of RETRACE's paths, read-only."""
    import _direct_oracle as DO
    import _path_oracle as P
    a, b, cam = demo_descriptions()
    c = RETRACE
    camera = DO.oracle_camera_samples(a, cam, c["w"], c["h"], c["seed"], c["stream"], c["first"], c["n"])
    samples = np.zeros(c["n"], RO.SAMPLE_DTYPE)
    samples["ray"]["origin"], samples["ray"]["direction"] = camera["ray"]["origin"], camera["ray"]["direction"]
    samples["ray"]["wavelength"], samples["x"], samples["y"] = camera["ray"]["wavelength"], camera["x"], camera["y"]
    out = [samples]
    for objs in (a, b):
        r = P.PathOracle(objs, cam).render_rays(samples["ray"]["origin"], samples["ray"]["direction"], samples["ray"]["wavelength"],
                                                c["seed"], c["stream"], c["first"]).view(RO.RESULT_DTYPE)
        out.append(r)
    for array in out:
        array.setflags(write=False)
    return tuple(out)


def sun_gains(n_nodes=81):
    return RO.gains_black_body(n_nodes, *SUN_FROM, *SUN_TO)


def retrace_figures():
    """The re-trace case on the oracles: (gap, bound, data, rounding, B's XYZ film), each (w * h, 3) float64."""
    import _image_cases as IC
    c = RETRACE
    w, h = c["w"], c["h"]
    samples, a, b = retrace()
    objs, _, _ = demo_descriptions()
    n_groups = 3
    table = RO.groups_of(objs, n_groups)
    film = RO.splat(w, h, 81, n_groups, samples, a, table)[0]
    gains = np.ones((n_groups, 81), np.float32)
    gains[table[SUN]] = sun_gains()
    cie = matrix("cie", 81)
    relit = RO.mix(film, gains, cie).astype(np.float64)
    retraced = IC.splat(w, h, RO.photons_of(samples, b))[0].reshape(-1, 3).astype(np.float64)
    bound, data, rounding = RO.retrace_bound(w, h, samples, a, b, SUN, gains[table[SUN]], cie, n_groups)
    return np.abs(relit - retraced), bound, data, rounding, retraced
