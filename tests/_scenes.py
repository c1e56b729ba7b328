"""Scene descriptions by name for the tests of the ray calls: the built-in scenes, random scenes at the sizes that reach every kernel
variant, the degenerate sphere layouts, the same with emitters to sample, and a small closed scene for the estimator's mean.  Every
call builds its description anew: tests write into the arrays they get back."""
import numpy as np

import robigo_luculenta_amd as R
import _oracle as O
import _random_scene as RS

SCENES = ["demo", "demo-2500", "glass", "random-seed-1", "random-seed-2", "random-seed-3", "many-prisms", "tables-prisms",
          "degenerate-same", "degenerate-line", "degenerate-zero_radius", "degenerate-huge_spread", "degenerate-infinite",
          "random-6000", "random-20000"]


def _scene(name):
    """(objects, camera) of the scene `name`; KeyError for a name that is none."""
    if name == "demo":
        return R.builtin_scene_desc(R.SCENE_DEMO)
    if name == "demo-2500":
        return R.builtin_scene_desc(R.SCENE_DEMO, 2500)
    if name == "glass":
        return R.builtin_scene_desc(R.SCENE_GLASS_STRESS)
    if name.startswith("random-seed-"):
        seed = int(name.rsplit("-", 1)[1])
        return RS.random_scene(seed, n_spheres=[40, 300, 700][seed % 3], n_prisms=6 + seed % 5)
    if name == "many-prisms":
        return RS.random_scene(22, n_spheres=60, n_prisms=70)
    if name == "tables-prisms":
        return RS.random_scene(77, n_spheres=3000, n_prisms=48, n_planes=2, n_circles=3, n_parabs=1)
    if name == "random-6000":
        return RS.random_scene(41, n_spheres=6000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1)
    if name == "random-20000":
        return RS.random_scene(35, n_spheres=20000, n_prisms=12, n_planes=2, n_circles=3, n_parabs=1)
    if name.startswith("degenerate-"):   # 57 spheres from a generator of their own: not the 57 of the tests that make four sizes from one
        objs0, cam = R.builtin_scene_desc(R.SCENE_DEMO)
        proto, rest = objs0[objs0["surface_kind"] == 0][:1], objs0[objs0["surface_kind"] != 0]
        return np.concatenate([rest, RS.degenerate_spheres(proto, name.split("-", 1)[1], 57, np.random.default_rng(7))]), cam
    raise KeyError(name)


def _with_lights(objs, rng):
    """A description with a few more black-body spheres and discs appended, discs with normals next to +z and -z among them."""
    extra = np.zeros(6, objs.dtype)
    extra["material_kind"] = 0
    extra["m"] = [(rng.uniform(3000, 9000), rng.uniform(0.3, 1.0), 0) for _ in range(6)]
    extra["surface_kind"] = [0, 0, 2, 2, 2, 2]
    extra["f"][:, 0] = rng.uniform(1.0, 5.0, 6)
    for k in range(2):
        extra["v0"][k] = rng.normal(0, 14, 3)
    for k, nrm in ((2, rng.normal(size=3)), (3, (3e-3, 2e-3, 1.0)), (4, (-2e-3, 4e-3, -1.0)), (5, (0.02, 0.0, 1.0))):
        nrm = np.asarray(nrm, np.float64)
        extra["v0"][k] = (nrm / np.linalg.norm(nrm)).astype(np.float32)
        extra["v1"][k] = rng.normal(0, 16, 3)
    assert (np.abs(extra["v0"][3:5, 2]) > 0.9999).all() and abs(extra["v0"][5, 2]) < 0.9999, extra["v0"][3:6, 2]
    return np.concatenate([objs, extra])


def _lit_scene(name):
    """_scene(name) with emitters to sample: the random scenes get a few more (_with_lights)."""
    objs, cam = _scene(name)
    if name.startswith("random") or name.endswith("prisms"):
        objs = _with_lights(np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), np.random.default_rng(len(name)))
    return np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), cam


def closed_scene(occluder):
    """A diffuse-grey floor z = 0 under a black ceiling, one sphere light, one disc light and, optionally, a sphere between the
    floor's origin and the lights."""
    rows = [
        (1, 1, (0, 0, 1), (0, 0, 0), 0.0, (0.7, 0, 0)),                 # the floor: a diffuse-grey plane
        (0, 0, (1.5, 0.5, 4.0), (0, 0, 0), 0.8, (6000.0, 1.0, 0)),      # a sphere light
        (2, 0, (0, 0, -1), (-2.0, 1.0, 5.0), 1.5, (4500.0, 0.8, 0)),    # a disc light facing down
        (0, 1, (0, 0, 0), (0, 0, 0), 40.0, (0.0, 0, 0)),                # a black (reflectance 0) shell around everything
    ]
    if occluder:
        rows.append((0, 1, (0.6, 0.3, 2.0), (0, 0, 0), 0.5, (0.0, 0, 0)))   # a black sphere in front of part of both lights
    objs = np.zeros(len(rows), R.OBJECT_DTYPE)
    for o, (sk, mk, v0, v1, f0, m) in zip(objs, rows):
        o["surface_kind"], o["material_kind"], o["v0"], o["v1"], o["m"] = sk, mk, v0, v1, m
        o["f"][0] = f0
    return objs, O.demo_scene_desc()[1]
