"""Scene descriptions by name for the tests of the ray calls: the built-in scenes, random scenes at the sizes that reach every kernel
variant, the degenerate sphere layouts, parts of the built-in scenes without their walls, the same with emitters to sample, a small closed scene for the estimator's mean,
and the scenes at the staging thresholds and with many prisms or small primitives (EXTREME_SCENES).  Every
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


# Descriptions at the sizes where the library's choices flip and far beyond the counts of prisms and small primitives of every scene
# above (tests/test_scene_extremes.py holds each to its shape and to the property it is named for; its docstring has the table).
# The two edge-* pairs are found with the host mirror when first asked for (_thresholds), never written down; edge-tables-open is
# edge-tables with nine prisms fewer, so that the tables are staged in an open launch of the trace kernel as well.
EXTREME_SMALL = {  # name: (planes, circles, paraboloids, order of the small primitives)
    "small-0": (0, 0, 0, "lists"), "small-1p": (1, 0, 0, "lists"), "small-1q": (0, 0, 1, "lists"), "small-64": (32, 32, 0, "lists"),
    "small-65": (33, 32, 0, "lists"), "small-200": (100, 100, 0, "lists"), "parabs-65": (0, 0, 65, "lists"),
    "small-mixed-130": (33, 32, 65, "interleaved"), "small-mixed-130-ordered": (33, 32, 65, "paraboloids-first")}
EXTREME_PRISMS = {"prisms-39": 39, "prisms-40": 40, "prisms-41": 41, "prisms-300": 300, "prisms-1000": 1000}
EXTREME_PRISM_SEEDS = {"prisms-39": 9309, "prisms-40": 9322, "prisms-41": 9318, "prisms-300": 9500, "prisms-1000": 10200}
MINIMAL_SCENES = ["min-sphere-emitter", "min-prism", "min-plane", "min-emitters"]
EXTREME_SCENES = (["edge-whole", "edge-whole+1", "edge-tables", "edge-tables+1", "edge-tables-open"] + list(EXTREME_PRISMS) + ["prisms-stack-200"] +
                  list(EXTREME_SMALL) + ["planes-coincident-50"] + MINIMAL_SCENES)
# Seeds whose glowing walls do not stand in front of the camera at the counts found.  (Most seeds' do at N*: rl_flatten_scene prices
# its cull tables on the scene's own camera paths, a scene whose paths all end on a wall at once gets the smallest table, and the
# largest count that is still staged whole is then one of those.  tests/test_scene_extremes.py holds the paths to 1.5 segments.)
EDGE_WHOLE_SEED, EDGE_TABLES_SEED, EDGE_TABLES_SPHERES = 9141, 9108, 3000
_THRESHOLDS = {}


def _edge_whole(n_spheres):
    return RS.random_scene(EDGE_WHOLE_SEED, n_spheres=n_spheres, n_prisms=6)


def _edge_tables(n_prisms, n_circles=2):
    return RS.random_scene(EDGE_TABLES_SEED, n_spheres=EDGE_TABLES_SPHERES, n_prisms=n_prisms, n_circles=n_circles)


def _thresholds():
    """{"N": the largest sphere count at which _edge_whole is staged whole, "P": the largest prism count at which _edge_tables'
    tables are staged, "C": the largest number of circles with which they still are at P, "lds": the LDS bytes a plain launch asks
    for at N, N + 1, P and P + 1 (the last two with C circles)}, by tests/_mirror.py's statement of the staging rule on the host
    mirror's layout figures: a bisection and, for the spheres, a walk over the next 16 counts, since the planner's padding does
    not make the sizes strictly monotonic.  Prisms come to the tables three at a time, 2.6 KB a group, so P alone stops up to that far below
    the limit; a circle takes 32 bytes, and C of them bring the request to the last 512-byte step.  Found once per process."""
    if not _THRESHOLDS:
        import _mirror as M
        from _boundary import _ocam

        def stage(make, count):
            objs, cam = make(count)
            return M.predicted_stage(M.layout(M.Scene(objs.view(O.OBJECT_DTYPE), _ocam(cam))))

        def largest(make, lo, hi, ok, walk=0):
            """The largest count in [lo, hi) for which ok(stage) holds, lo being one and hi none; then the first of the next `walk`
            counts above it that holds too, if any, and so on."""
            assert ok(stage(make, lo)[0]) and not ok(stage(make, hi)[0]), (lo, hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if ok(stage(make, mid)[0]) else (lo, mid)
            k = lo + 1
            while k <= lo + walk:
                if ok(stage(make, k)[0]):
                    lo = k
                k += 1
            return lo

        # (brackets from the sizes: 32 KB hold the records of fewer than 1,200 spheres, and the 61 records of a prism group --
        # 17 and 2 of the cylinder per prism, 4 bounds -- under 34 times; a flattening of 3,000 spheres takes a second)
        n = largest(_edge_whole, 400, 1200, lambda s: s == M.STAGE_ALL, walk=16)
        p = largest(_edge_tables, 40, 104, lambda s: s != M.STAGE_NONE)
        c = largest(lambda k: _edge_tables(p, k), 2, 98, lambda s: s != M.STAGE_NONE)
        _THRESHOLDS.update({"N": n, "P": p, "C": c, "lds": (stage(_edge_whole, n)[1], stage(_edge_whole, n + 1)[1],
                                                            stage(lambda k: _edge_tables(k, c), p)[1], stage(lambda k: _edge_tables(k, c), p + 1)[1])})
    return _THRESHOLDS


def _materials(rng, objs):
    """RS.random_scene's mix of materials for records made here: all six kinds, planes glow -- and three paraboloids in ten, so that
    a cage of paraboloids alone ends paths on a light as a cage of planes does."""
    kinds = rng.choice([0, 1, 2, 3, 4, 5], size=len(objs), p=[0.05, 0.2, 0.25, 0.15, 0.15, 0.2])
    glow = rng.random(len(objs)) < 0.3
    for o, mk, lit in zip(objs, kinds, glow):
        mk = 0 if o["surface_kind"] == 1 or (o["surface_kind"] == 3 and lit) else int(mk)
        o["material_kind"] = mk
        o["m"] = {0: (rng.uniform(3000, 9000), rng.uniform(0.3, 1.0), 0), 1: (rng.uniform(0.3, 0.95), 0, 0),
                  2: (rng.uniform(0.5, 0.95), rng.uniform(400, 750), rng.uniform(20, 80)),
                  3: (rng.uniform(0.0, 0.5), 0, 0), 4: (0, 0, 0), 5: (0, 0, 0)}[mk]


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _small_primitives(rng, n_planes, n_circles, n_parabs):
    """(planes, circles, paraboloids) around the camera, which stands 50 units from the origin: walls 75 to 125 units out, discs
    among the spheres as RS.random_scene places them, and paraboloids of random axes and foci with the vertex 60 to 100 units out and
    the focus 40 to 120 further (the scene is on the convex side, as it is on the built-in room's floor).  The walls, and the
    paraboloids, come from the farthest to the nearest: the nearest of a cage always shows a face, so the last record of a long
    table is one the rays reach."""
    planes, circles, parabs = np.zeros(n_planes, O.OBJECT_DTYPE), np.zeros(n_circles, O.OBJECT_DTYPE), np.zeros(n_parabs, O.OBJECT_DTYPE)
    for o, dist in zip(planes, np.sort(rng.uniform(75, 125, n_planes))[::-1]):
        nrm = _unit(rng)
        o["surface_kind"], o["v0"], o["v1"] = 1, nrm, nrm * dist
    for o in circles:
        o["surface_kind"], o["v0"], o["v1"], o["f"][0] = 2, _unit(rng), rng.normal(0, 20, 3), rng.uniform(3, 12)
    for o, dist in zip(parabs, np.sort(rng.uniform(60, 100, n_parabs))[::-1]):
        nrm = _unit(rng)
        if n_parabs == 1:     # one alone stands behind the scene as the camera (at y < 0 < z) sees it, 30 units out: a tenth of the hits
            nrm, dist = nrm * (-1.0 if nrm[2] - nrm[1] > 0 else 1.0), 30.0
        o["surface_kind"], o["v0"], o["v1"], o["f"][0] = 3, nrm, nrm * dist + rng.normal(0, 4, 3), rng.uniform(40, 120) * (1 + (n_parabs == 1))
    for part in (planes, circles, parabs):
        _materials(rng, part)
    return planes, circles, parabs


def _extreme(name):
    """(objects, camera) of the scene `name` of EXTREME_SCENES."""
    rng = np.random.default_rng([0xe87, EXTREME_SCENES.index(name)])
    if name.startswith("edge-whole"):
        return _edge_whole(_thresholds()["N"] + name.endswith("+1"))
    if name == "edge-tables-open":   # three prism groups fewer: room for the 2,064 bytes an open launch of the trace kernel adds
        return _edge_tables(_thresholds()["P"] - 9, _thresholds()["C"])
    if name.startswith("edge-tables"):
        return _edge_tables(_thresholds()["P"] + name.endswith("+1"), _thresholds()["C"])
    if name in EXTREME_PRISMS:
        return RS.random_scene(EXTREME_PRISM_SEEDS[name], n_spheres=60, n_prisms=EXTREME_PRISMS[name])
    if name == "prisms-stack-200":
        objs, cam = RS.random_scene(9301, n_spheres=60, n_prisms=200)
        for k in np.flatnonzero(objs["surface_kind"] == 4):
            o = objs[k]                                # (a view of the record: written in place)
            centre = _unit(rng) * 0.5 * rng.random() ** (1 / 3)
            o["f"][3] = rng.uniform(40, 90)            # long enough for its bound to cover the camera's field of view from 50 units
            o["v1"] = centre - 0.5 * float(o["f"][3]) * o["v0"].astype(np.float64)    # v1 is the centre of the base, v0 the axis
        return objs, cam
    if name in EXTREME_SMALL:
        n_planes, n_circles, n_parabs, order = EXTREME_SMALL[name]
        objs, cam = RS.random_scene(9400 + EXTREME_SCENES.index(name), n_spheres=60, n_prisms=6, n_planes=0, n_circles=0, n_parabs=0)
        planes, circles, parabs = _small_primitives(rng, n_planes, n_circles, n_parabs)
        flat = np.concatenate([circles, planes])        # one table on the device: the walls stand at its end
        if order == "interleaved":
            small = np.zeros(len(flat) + len(parabs), O.OBJECT_DTYPE)
            small[0::2], small[1::2] = parabs, flat     # (65 and 65)
        else:
            small = np.concatenate([parabs, flat])
        return np.concatenate([objs, small]), cam
    if name == "planes-coincident-50":
        objs, cam = RS.random_scene(9500, n_spheres=60, n_prisms=6, n_planes=0, n_circles=0, n_parabs=0)
        nrm = np.array((0.2, -0.3, 1.0)) / np.linalg.norm((0.2, -0.3, 1.0))
        same = np.zeros(100, O.OBJECT_DTYPE)
        same["v0"], same["v1"] = nrm, nrm * -14.0
        same["surface_kind"][:50], same["surface_kind"][50:] = 1, 2
        same["f"][50:, 0] = 30.0
        for k, o in enumerate(same):                    # six materials; an emitter ends the path, the others send it on differently
            mk = k % 6
            o["material_kind"] = mk
            o["m"] = [(5000.0 + 40 * k, 0.6, 0), (0.4 + 0.005 * k, 0, 0), (0.8, 450.0 + 3 * k, 40.0), (0.1 + 0.004 * k, 0, 0), (0, 0, 0), (0, 0, 0)][mk]
        everything = np.concatenate([objs, same])
        return everything[rng.permutation(len(everything))], cam
    cam = O.demo_scene_desc()[1]
    rows = {"min-sphere-emitter": [(0, 0, (0, 0, 0), (0, 0, 0), (5.0, 0, 0, 0), (6000.0, 1.0, 0))],
            "min-prism": [(4, 4, (0, 0, 1), (0, 0, -12), (12.0, 0.8, 0.3, 24.0), (0, 0, 0))],
            "min-plane": [(1, 1, (0, 0.8, 0.6), (0, -2.4, -1.8), (0, 0, 0, 0), (0.7, 0, 0))],   # (its horizon crosses the camera's view)
            "min-emitters": [(0, 0, (6, 0, 2), (0, 0, 0), (3.0, 0, 0, 0), (6000.0, 1.0, 0)), (0, 0, (-5, 3, -1), (0, 0, 0), (2.0, 0, 0, 0), (4000.0, 0.8, 0)),
                             (0, 0, (0, -6, 4), (0, 0, 0), (2.5, 0, 0, 0), (8000.0, 0.5, 0)), (2, 0, (0, 0, 1), (0, 0, -6), (9.0, 0, 0, 0), (5000.0, 0.7, 0)),
                             (2, 0, (0.6, 0, 0.8), (-8, 4, 3), (4.0, 0, 0, 0), (7000.0, 0.9, 0)), (2, 0, (0, 1, 0), (3, 9, 0), (5.0, 0, 0, 0), (3500.0, 1.0, 0))]}[name]
    objs = np.zeros(len(rows), O.OBJECT_DTYPE)
    for o, (sk, mk, v0, v1, f, m) in zip(objs, rows):
        o["surface_kind"], o["material_kind"], o["v0"], o["v1"], o["f"], o["m"] = sk, mk, v0, v1, f, m
    return objs, cam


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
    if name in EXTREME_SCENES:
        return _extreme(name)
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
