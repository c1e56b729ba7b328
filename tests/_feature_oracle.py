"""rl_scene_render_features' contract, composed twice from what the tests already have -- once on the CPU oracles alone (the
camera samples of _direct_oracle, _step_oracle with NO_ROULETTE and hits) and once from the public GPU calls (camera_rays,
begin_paths, step_path_list with NO_ROULETTE and hits over the list of paths still in their chain).  Both give the records, and
with them the stats per path, so that one run over n paths answers for every prefix and span of them, and the three films' terms.
The splat of _image_cases (splat, splat_bound, splat_violations) is restated here for arbitrary signed per-sample colours.  Nothing
is built at import."""
import numpy as np

import _image_cases as IC

LIVE, NONE = 0xffffffff, 0xffffffff
END_VOID, END_EMITTER = 0, 1
NO_ROULETTE = 1
VOID, EMITTER, DIFFUSE, LIMIT = range(4)
DIFFUSE_GREY, DIFFUSE_COLOURED = 1, 2      # RL_MATERIAL_DIFFUSE_GREY, RL_MATERIAL_DIFFUSE_COLOURED
MAX_SEGMENTS = 64                          # max_segments = 0
FILMS = ("albedo", "normal", "aux")
FEATURE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("wavelength", "<f4"), ("albedo", "<f4"), ("normal", "<f4", 3), ("depth", "<f4"),
                          ("object", "<u4"), ("segments", "<u4"), ("kind", "<u4"), ("reserved", "<u4")])
PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])
assert FEATURE_DTYPE.itemsize == 48


def stats_of(records):
    """RlFeatureStats of the paths whose records these are, as Scene.render_features returns it."""
    return {"paths": len(records), "segments": int(records["segments"].astype(np.int64).sum()),
            "kinds": [int((records["kind"] == k).sum()) for k in range(4)]}


def add_stats(a, b):
    return {"paths": a["paths"] + b["paths"], "segments": a["segments"] + b["segments"], "kinds": [x + y for x, y in zip(a["kinds"], b["kinds"])]}


class Features:
    """What a feature render of n paths must produce: `records` (n RlFeatureSample records); a path's record depends on its own index
    only, so a prefix or a span of the records is the run of that prefix or span."""

    def __init__(self, records):
        self.records = records

    def prefix(self, n):
        return self.records[:n], stats_of(self.records[:n])

    def span(self, lo, hi):
        return stats_of(self.records[lo:hi])


def _compose(camera, materials, hit_dtype, begin, step, first, max_segments):
    """The loop the contract names.  begin(rays, first) -> states; step(states, hits, list) steps the listed states in place with
    RL_STEP_NO_ROULETTE and hits.  materials: the material kind of every object, in description order."""
    n = len(camera)
    materials = np.asarray(materials, np.int64)
    st = begin(np.ascontiguousarray(camera["ray"]), first)
    hits = np.zeros(n, hit_dtype)
    hits["object"] = NONE
    rec = np.zeros(n, FEATURE_DTYPE)
    rec["x"], rec["y"], rec["wavelength"] = camera["x"], camera["y"], camera["ray"]["wavelength"]
    rec["object"] = NONE
    lst = np.arange(n, dtype=np.uint32)
    limit = max_segments or MAX_SEGMENTS
    for segment in range(1, limit + 1):
        if not len(lst):
            break
        arriving = st["direction"][lst].astype(np.float32)       # the state's direction before the step
        step(st, hits, lst)
        assert (st["segments"][lst] == segment).all()
        if segment == 1:
            rec["depth"] = np.where(hits["object"] != NONE, hits["distance"], np.float32(0))
        end, obj = st["end"][lst], hits["object"][lst]
        material = np.where(obj != NONE, materials[np.minimum(obj, len(materials) - 1)], -1)
        kind = np.full(len(lst), -1, np.int64)                   # -1: the path goes on
        if segment == limit:
            kind[:] = LIMIT
        kind[(material == DIFFUSE_GREY) | (material == DIFFUSE_COLOURED)] = DIFFUSE
        kind[end == END_EMITTER] = EMITTER
        kind[end == END_VOID] = VOID                             # (the first rule that applies: written last)
        done = kind >= 0
        rows, surface = lst[done], (kind[done] == EMITTER) | (kind[done] == DIFFUSE)
        rec["kind"][rows], rec["segments"][rows] = kind[done], segment
        rec["albedo"][rows] = np.where(surface, st["intensity"][rows], np.float32(0))
        rec["object"][rows] = np.where(surface, obj[done], NONE)
        d, nrm = arriving[done], hits["normal"][rows].astype(np.float32)
        with np.errstate(all="ignore"):
            facing = d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1] + d[:, 2] * nrm[:, 2] < 0     # rl_bounce's `facing`, in float32
        turned = np.where(facing[:, None], nrm, -nrm)
        rec["normal"][rows] = np.where(surface[:, None], turned, np.float32(0))
        lst = lst[~done]
    assert not len(lst)
    return Features(rec)


def cpu_features(objs, cam, w, h, seed, stream, first, n, max_segments, camera=None):
    """The contract on the CPU oracles alone, for the camera of a w x h film (camera: its samples, where the caller has them)."""
    import _direct_oracle as DO
    import _step_oracle as S
    if camera is None:
        camera = DO.oracle_camera_samples(objs, cam, w, h, seed, stream, first, n)
    stepper = S.StepOracle(objs, cam)

    def step(st, hits, lst):
        sub, sub_hits = st[lst], hits[lst]
        stepper.step(sub, seed, stream, flags=NO_ROULETTE, hits=sub_hits)
        st[lst], hits[lst] = sub, sub_hits

    return _compose(camera, stepper.objs["material_kind"], S.HIT_DTYPE, S.begin, step, first, max_segments)


def gpu_loop(scene, objs, w, h, seed, stream, first, n, max_segments, fetch=0):
    """The same composition from the public GPU calls; objs is the description the scene was made from."""
    import robigo_luculenta_amd as R
    camera = scene.camera_rays(w, h, seed, stream, first, n)

    def step(st, hits, lst):
        scene.step_path_list(st, seed, stream, list=lst, n_list=len(lst), fetch=fetch, flags=NO_ROULETTE, hits=hits)

    return _compose(camera, np.asarray(objs)["material_kind"], R.HIT_DTYPE, scene.begin_paths, step, first, max_segments)


# ---- the films ----------------------------------------------------------------------------------------------------------

def albedo_photons(records):
    """The photons {x, y, albedo, wavelength} whose rl_plot_unit_plot_photons is the albedo film."""
    with np.errstate(invalid="ignore"):
        on = records["albedo"] != 0
    ph = np.zeros(int(on.sum()), PHOTON_DTYPE)
    ph["x"], ph["y"], ph["probability"], ph["wavelength"] = records["x"][on], records["y"][on], records["albedo"][on], records["wavelength"][on]
    return ph


def film_samples(records, film):
    """(x, y, colours float32 (m, 3)) of the samples the film named `film` takes from these records."""
    if film == "albedo":
        with np.errstate(invalid="ignore"):
            on = records["albedo"] != 0
        colours = IC.tristimulus(records["wavelength"][on]) * records["albedo"][on].astype(np.float32)[:, None]
    elif film == "normal":
        on = (records["kind"] == EMITTER) | (records["kind"] == DIFFUSE)
        colours = records["normal"][on]
    else:
        on = np.ones(len(records), bool)
        colours = np.stack([np.ones(len(records), np.float32), records["depth"], records["segments"].astype(np.float32)], axis=1)
    return records["x"][on], records["y"][on], np.ascontiguousarray(colours, np.float32).reshape(-1, 3)


def splat_terms(w, h, x, y, colours):
    """_image_cases.splat_terms for samples that bring their own colour: pixel indices (n, 4) and float32 contributions (n, 4, 3),
    in the reference's order."""
    f = np.float32
    aspect = f(w) / f(h)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    px = (x * f(0.5) + f(0.5)) * (f(w) - f(1.0))
    py = (y * aspect * f(0.5) + f(0.5)) * (f(h) - f(1.0))
    px1 = np.clip(np.floor(px).astype(np.int64), 0, w - 1)
    px2 = np.clip(np.ceil(px).astype(np.int64), 0, w - 1)
    py1 = np.clip(np.floor(py).astype(np.int64), 0, h - 1)
    py2 = np.clip(np.ceil(py).astype(np.int64), 0, h - 1)
    cx = px - px1.astype(np.float32)
    cy = py - py1.astype(np.float32)
    one = f(1.0)
    wts = np.stack([(one - cx) * (one - cy), cx * (one - cy), (one - cx) * cy, cx * cy], axis=1)
    idx = np.stack([py1 * w + px1, py1 * w + px2, py2 * w + px1, py2 * w + px2], axis=1)
    return idx, (np.asarray(colours, np.float32)[:, None, :] * wts[:, :, None]).astype(np.float32)


def splat(w, h, x, y, colours, image=True):
    """(image float32 (w * h, 3) summed in sample order, k int (w * h, 3): the nonzero terms of each pixel component, S float64: the
    sum of their magnitudes, exact float64: their sum) -- _image_cases.splat for signed colours.  image=False: the image is the
    exact sum rounded, for films of so many samples that only the bound is asked of them."""
    idx, terms = splat_terms(w, h, x, y, colours)
    idx, terms = idx.reshape(-1), terms.reshape(-1, 3)
    k, s, exact = np.zeros((w * h, 3), np.int64), np.zeros((w * h, 3), np.float64), np.zeros((w * h, 3), np.float64)
    for c in range(3):      # (bincount adds in sample order, as np.add.at does)
        t = terms[:, c].astype(np.float64)
        k[:, c] = np.bincount(idx, weights=(t != 0), minlength=w * h).astype(np.int64)
        s[:, c] = np.bincount(idx, weights=np.abs(t), minlength=w * h)
        exact[:, c] = np.bincount(idx, weights=t, minlength=w * h)
    if image:
        img = np.zeros((w * h, 3), np.float32)
        np.add.at(img, idx, terms)
    else:
        img = exact.astype(np.float32)
    return img, k, s, exact


def splat_bound(k, s):
    """Any order of k float32 adds onto zero, of either sign, lands within (k - 1) 2^-24 S of the exact sum: k - 1 of the adds
    round, each by at most 2^-24 of a partial sum, and no partial sum exceeds S in magnitude.  (The 1e-6 covers the float64 sum's
    own error.)  With k <= 2 every order gives the same bits."""
    return (k - 1).clip(0).astype(np.float64) * 2.0 ** -24 * s * (1 + 1e-6)


def splat_violations(got, want, k, s, exact):
    """Indices (pixel, component) where got is not within splat_bound of the exact sum, or (k <= 2) not want's bits; and the worst
    excess."""
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - exact)
    bound = splat_bound(k, s)
    bad = np.where(k <= 2, got.view(np.uint32) != np.asarray(want, np.float32).view(np.uint32), ~(d <= bound))
    return np.argwhere(bad), (float((d - bound)[bad].max()) if bad.any() else 0.0)


def film(w, h, records, name, image=True):
    """splat() of the film named `name` for these records."""
    return splat(w, h, *film_samples(records, name), image=image)


def assert_film(got, w, h, records, name, what="", bound_only=False):
    """`got` (w * h, 3) is that film of `records` plotted onto a cleared buffer: rtol 2e-5 and the per-pixel bound.  bound_only: the
    per-pixel bound alone, against the exact sum -- for films with tens of thousands of terms per component, where two float32
    orders of the same terms lie further apart than rtol 2e-5 by chance and only the derived bound is certain."""
    want, k, s, exact = film(w, h, records, name, image=not bound_only)
    scale = float(np.abs(want).max()) if want.size else 0.0
    bad, excess = splat_violations(got, want, k, s, exact)
    print("%s %s: max |got - want| %.3e (film max %.3e, up to %d terms), per-pixel violations %d, worst excess %.3e"
          % (what, name, float(np.abs(got - want).max()) if got.size else 0.0, scale, int(k.max()) if k.size else 0, len(bad), excess))
    if not bound_only:
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6 * scale), (what, name)
    assert not len(bad), (what, name, bad[:8], excess)
    return want
