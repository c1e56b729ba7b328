"""Scene descriptions by name for the tests of the ray calls: the built-in scenes, random scenes at the sizes that reach every kernel
variant, the degenerate sphere layouts, parts of the built-in scenes without their walls, the same with emitters to sample, and a small closed scene for the estimator's mean.  Every
call builds its description anew: tests write into the arrays they get back."""
import numpy as np

import robigo_luculenta_amd as R
import _oracle as O
import _random_scene as RS

SCENES = ["demo", "demo-2500", "glass", "random-seed-1", "random-seed-2", "random-seed-3", "many-prisms", "tables-prisms",
          "degenerate-same", "degenerate-line", "degenerate-zero_radius", "degenerate-huge_spread", "degenerate-infinite",
          "random-6000", "random-20000"]


# The shapes of a description that rl_scan_wave's code paths depend on and no scene above has (tests/test_scene_shapes.py holds each
# to the shape named here): the built-in room with one normal off z / a seventh small primitive / a plane in front of its
# paraboloids, random scenes under a permutation of the whole description at the sizes of the four table shapes, and permuted scenes
# whose objects coincide across the kernel's tables.
SHAPE_SCENES = ["room-tilted", "room-plus-disc", "room-reordered", "shuffled-40", "shuffled-300", "shuffled-3000", "shuffled-6000",
                "coincident-300", "coincident-3000"]


# Parts of the built-in descriptions for rays from far outside (tests/_cases.py: far_rays_at and its kin): the walls of the closed
# room stop nearly every such ray before a prism, so these leave them out.  glass-spheres-prisms keeps the glass-stress scene's
# 66 prisms -- 40 or more, so it runs the kernels' CYL variants and their cylinder bound.
# demo-open is the built-in scene without its plane and paraboloids: lights, spheres and prisms that a camera far outside can see.
FAR_SUBSETS = {"demo-prisms": ("demo", (4,)), "demo-spheres-prisms": ("demo", (0, 4)), "demo-prisms-paraboloids": ("demo", (3, 4)),
               "glass-spheres-prisms": ("glass", (0, 4)), "demo-open": ("demo", (0, 2, 4))}


def camera_moved_back(cam, back, telescope=False):
    """A copy of the camera record `cam` translated `back` units back along its view axis (it looks at the scene's origin from
    dist0); with `telescope`, its field of view narrowed to half of what shows the same part of the scene as before."""
    moved = type(cam).from_buffer_copy(bytes(cam))
    moved.dist0 = cam.dist0 + back
    if telescope:
        moved.fov_over_pi = 0.5 * cam.fov_over_pi * cam.dist0 / (cam.dist0 + back)
    return moved


def _room(change):
    """The built-in scene with its small primitives changed: "tilted" (the second circle's normal a hair off z), "plus-disc" (a
    seventh small primitive, a circle in the first circle's own plane and overlapping it, appended behind everything) or
    "reordered" (the first plane in the place of the first paraboloid, then the paraboloids last to first, then the rest)."""
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE).copy()
    kinds = objs["surface_kind"]
    circles = np.flatnonzero(kinds == 2)
    if change == "tilted":
        k = int(circles[1])
        nrm = np.array((3e-3, 2e-3, 1.0), np.float64) * (-1.0 if objs["v0"][k, 2] < 0 else 1.0)
        objs["v0"][k] = (nrm / np.linalg.norm(nrm)).astype(np.float32)
    elif change == "plus-disc":
        disc = objs[circles[:1]].copy()       # coplanar with the first circle and overlapping it: the ordered loop meets exact ties
        disc["v1"][0, :2] += disc["f"][0, 0] * np.float32(0.75)
        disc["material_kind"], disc["m"] = 3, (0.1, 0.0, 0.0)
        objs = np.concatenate([objs, disc])
    elif change == "reordered":
        small = np.flatnonzero((kinds >= 1) & (kinds <= 3))
        parabs, plane = np.flatnonzero(kinds == 3), int(np.flatnonzero(kinds == 1)[0])
        order = [plane] + list(parabs[::-1]) + [int(k) for k in small if kinds[k] != 3 and k != plane]
        objs[small] = objs[order]
    else:
        raise KeyError(change)
    return objs, cam


def _shuffled(n_spheres):
    """A random scene of n_spheres spheres and its light under a seeded permutation of the whole description: surface kinds
    interleave, planes precede paraboloids, the light stands anywhere."""
    objs, cam = RS.random_scene(500 + n_spheres, n_spheres=n_spheres, n_prisms=12, n_planes=2, n_circles=3, n_parabs=2)
    return objs[np.random.default_rng([n_spheres, 1]).permutation(len(objs))], cam


def _coincident(n_spheres):
    """A random scene with a coincident copy, of another material kind, of every plane, circle, paraboloid and prism and of a
    tenth of its spheres, and a circle of radius 30 in each plane's own plane, permuted: equal distances to objects of different
    tables, which only the object numbers decide (scene.rs:51) and whose winner shows in the path that follows.
    The seeds are ones at which a copied sphere stands in the camera's view (it sees a handful of the large ones): at least a
    tenth of the camera rays' first hits tie exactly, which tests/test_scene_shapes.py holds them to."""
    objs, cam = RS.random_scene({300: 1201, 3000: 3908}[n_spheres], n_spheres=n_spheres, n_prisms=12, n_planes=2, n_circles=3, n_parabs=2)
    rng = np.random.default_rng([n_spheres, 2])
    kinds = objs["surface_kind"]
    spheres = np.flatnonzero(kinds == 0)
    copies = objs[np.concatenate([np.flatnonzero(kinds != 0), rng.choice(spheres, len(spheres) // 10, replace=False)])].copy()
    diffuse = copies["material_kind"] != 1     # a copy is diffuse, a diffuse object's copy a mirror
    copies["material_kind"] = np.where(diffuse, 1, 3)
    copies["m"] = 0.0
    copies["m"][:, 0] = np.where(diffuse, 0.8, 0.1)
    discs = objs[kinds == 1].copy()            # same normal (v0) and offset point (v1) as the plane
    discs["surface_kind"], discs["material_kind"], discs["m"] = 2, 3, (0.2, 0.0, 0.0)
    discs["f"][:, 0] = 30.0
    everything = np.concatenate([objs, copies, discs])
    return everything[rng.permutation(len(everything))], cam


def _scene(name):
    """(objects, camera) of the scene `name`; KeyError for a name that is none."""
    if name in SHAPE_SCENES:
        family, what = name.split("-", 1)
        if family == "room":
            return _room(what)
        if family == "shuffled":
            return _shuffled(38 if what == "40" else int(what))   # 38 and the light: 39 spheres, the most that get no clusters
        return _coincident(int(what))
    if name in FAR_SUBSETS:
        whole, kinds = FAR_SUBSETS[name]
        objs, cam = _scene(whole)
        objs = np.ascontiguousarray(objs).view(R.OBJECT_DTYPE)
        return objs[np.isin(objs["surface_kind"], kinds)].copy(), cam
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
