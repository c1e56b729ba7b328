"""The scenes of tests/_scenes.py's EXTREME_SCENES, on the host: each description has the shape it is named for -- counts, flags,
prism groups and their remainder, the cylinder bound on or off, a third table level or none, the stage the library's rule picks
under LDS fetch -- and really has the property that makes it worth running; and the host mirror's plain C++ scan renders the
oracle's photons on every one, so that a planner fault shows here, before a kernel runs.  No GPU:
tests/test_gpu_scene_extremes.py runs every kernel family on the same scenes and holds the stage predicted here to the variant the
library launches.

    scene                    spheres  prisms (records)  cylinders  planes+circles  paraboloids  ordered  stage under LDS fetch
    edge-whole               N* + 1   6 (6)             no         4               1            no       whole, within 512 B of 160 KB
    edge-whole+1             N* + 2   6 (6)             no         4               1            no       tables
    edge-tables              3,001    P* (P* padded)    yes        2 + C*          1            no       tables, within 512 B of 160 KB
    edge-tables+1            3,001    P* + 1            yes        2 + C*          1            no       none
    edge-tables-open         3,001    P* - 9            yes        2 + C*          1            no       tables, in an open launch too
    prisms-39                61       39 (39)           no         4               1            no       whole
    prisms-40                61       40 (42)           yes        4               1            no       whole (one group of one prism)
    prisms-41                61       41 (42)           yes        4               1            no       whole (one group of two)
    prisms-300               61       300 (300)         yes        4               1            no       none (82 KB of prism records)
    prisms-1000              61       1000 (1002)       yes        4               1            no       none
    prisms-stack-200         61       200 (201)         yes        4               1            no       none (54 KB of prism records)
    small-0                  61       6 (6)             no         0               0            yes      whole
    small-1p                 61       6 (6)             no         1               0            yes      whole
    small-1q                 61       6 (6)             no         0               1            yes      whole
    small-64                 61       6 (6)             no         64              0            yes      whole
    small-65                 61       6 (6)             no         65              0            yes      whole
    small-200                61       6 (6)             no         200             0            yes      whole
    parabs-65                61       6 (6)             no         0               65           yes      whole
    small-mixed-130          61       6 (6)             no         65              65           no       whole
    small-mixed-130-ordered  61       6 (6)             no         65              65           yes      whole
    planes-coincident-50     61       6 (6)             no         100             0            yes      whole
    min-sphere-emitter       1        0                 no         0               0            yes      whole
    min-prism                0        1 (3)             no         0               0            yes      whole
    min-plane                0        0                 no         1               0            yes      whole
    min-emitters             3        0                 no         3               0            yes      whole

(spheres: RS.random_scene's light is one of them.  N*, P* and C* are found by bisection with the mirror, tests/_scenes.py:
_thresholds, and printed by test_the_staging_thresholds: at the time of writing 668 spheres, and 81 prisms with 7 circles, both
scenes asking for exactly 163,840 bytes of LDS; their successors ask for 134,656 (tables) and 131,072 (nothing staged).  Prisms
come to the tables a group of three at a time, so P* alone stops up to a kilobyte short of the limit: C* circles of 32 bytes fill
the request up to its last 512-byte step.  The whole scene and the per-wave scratch share 160 KB, and the scratch of a 16-wave
workgroup is 128 KB: what is staged has 32 KB, 24 KB where the cull table has a third level.  A prism takes 17 records of 16 bytes
and its share of the cull table, so the tables of about a hundred prisms are the most that fit, and prisms-300 and
prisms-stack-200 run the variants that stage nothing, as prisms-1000 does.)

What each scene is there for, held by the oracle alone (ray_sets' camera and bounce families, 2,048 rays each):
    prisms-*                 at least 10 % of the rays of either family hit a prism first
    prisms-stack-200         a camera ray passes the level-1 bounds of at least 100 prisms on average
    small-*, parabs-65       at least 10 % of first hits are small primitives; with 65 and more of them, at least 1 % are one whose
                             position in its table is 64 or beyond
    planes-coincident-50     at least 10 % of hits tie exactly with another object
    min-*                    hits and misses both occur
    edge-*                   the stage differs within each pair, and the lower scene asks for all but at most 512 bytes of the LDS
    every scene but min-*    a camera path has at least 1.5 segments on average (no glowing wall stands in front of the camera)"""
import zlib

import numpy as np
import pytest

import _mirror as M
import _oracle as O
from _boundary import _ocam
from _cases import oracle_hits, ray_sets, tied_hits
from _scenes import EXTREME_PRISMS, EXTREME_SCENES, EXTREME_SMALL, MINIMAL_SCENES, SCENES, SHAPE_SCENES, _scene, _thresholds

NONE = 0xffffffff
WHOLE, TABLES, NOTHING = M.STAGE_ALL, M.STAGE_TABLES, M.STAGE_NONE
#        name: (spheres, prisms, prism records, planes and circles, paraboloids, small_ordered, stage under LDS fetch)
SHAPES = {"prisms-39": (61, 39, 39, 4, 1, False, WHOLE), "prisms-40": (61, 40, 42, 4, 1, False, WHOLE),
          "prisms-41": (61, 41, 42, 4, 1, False, WHOLE), "prisms-300": (61, 300, 300, 4, 1, False, NOTHING),
          "prisms-1000": (61, 1000, 1002, 4, 1, False, NOTHING), "prisms-stack-200": (61, 200, 201, 4, 1, False, NOTHING),
          "small-0": (61, 6, 6, 0, 0, True, WHOLE), "small-1p": (61, 6, 6, 1, 0, True, WHOLE), "small-1q": (61, 6, 6, 0, 1, True, WHOLE),
          "small-64": (61, 6, 6, 64, 0, True, WHOLE), "small-65": (61, 6, 6, 65, 0, True, WHOLE),
          "small-200": (61, 6, 6, 200, 0, True, WHOLE), "parabs-65": (61, 6, 6, 0, 65, True, WHOLE),
          "small-mixed-130": (61, 6, 6, 65, 65, False, WHOLE), "small-mixed-130-ordered": (61, 6, 6, 65, 65, True, WHOLE),
          "planes-coincident-50": (61, 6, 6, 100, 0, True, WHOLE), "min-sphere-emitter": (1, 0, 0, 0, 0, True, WHOLE),
          "min-prism": (0, 1, 3, 0, 0, True, WHOLE), "min-plane": (0, 0, 0, 1, 0, True, WHOLE), "min-emitters": (3, 0, 0, 3, 0, True, WHOLE)}
_CASES = {}


class _Case:
    pass


class _OracleQueries:
    """The one call ray_sets makes on a scene, answered by the oracle."""

    def __init__(self, so):
        self.so = so

    def intersect(self, o, d):
        return oracle_hits(self.so, o, d)


def _case(name):
    """Scene `name` in the oracle and the mirror, its layout figures, and the oracle's first hits for ray_sets' camera and bounce
    families at 2,048 rays; made once, no test writes into it."""
    if name not in _CASES:
        c = _Case()
        objs, cam = _scene(name)
        c.objs, c.cam = np.ascontiguousarray(objs).view(O.OBJECT_DTYPE), _ocam(cam)
        c.so, c.sm = O.Scene(c.objs, c.cam), M.Scene(c.objs, c.cam)
        c.lay = M.layout(c.sm)
        sets = ray_sets(_OracleQueries(c.so), c.objs, c.cam, np.random.default_rng(zlib.crc32(name.encode())), 2048)
        c.sets = {kind: sets[kind] for kind in ("camera", "bounce")}
        c.want = {kind: oracle_hits(c.so, o, d) for kind, (o, d) in c.sets.items()}
        _CASES[name] = c
    return _CASES[name]


def _first_hits(c, kind):
    """(surface kinds of the objects hit first by family `kind`, their object numbers, rays in the family)."""
    obj = c.want[kind]["object"]
    obj = obj[obj != NONE]
    return c.objs["surface_kind"][obj], obj, len(c.want[kind])


def test_the_table_above_names_every_extreme_scene():
    edges = [n for n in EXTREME_SCENES if n.startswith("edge-")]
    assert len(edges) == 5 and not set(SHAPES) & set(edges) and set(SHAPES) | set(edges) == set(EXTREME_SCENES)
    assert len(set(EXTREME_SCENES)) == len(EXTREME_SCENES) == 25 and not set(EXTREME_SCENES) & set(SCENES + SHAPE_SCENES)
    assert set(EXTREME_PRISMS) | set(EXTREME_SMALL) | set(MINIMAL_SCENES) < set(SHAPES)


def test_the_staging_thresholds():
    """N*, P* and the four LDS requests, printed; within each pair the stage differs and nothing else the kernel variants or the
    scan's loops depend on does; the lower scene of each pair asks for all the LDS but at most 512 bytes."""
    th = _thresholds()
    lays = {name: _case(name).lay for name in EXTREME_SCENES if name.startswith("edge-")}
    stages = {name: M.predicted_stage(lay) for name, lay in lays.items()}
    # an open launch of the trace kernel has 2,064 bytes less: at the thresholds it stages one step less than a plain launch
    assert [M.predicted_stage(lays[n], open_launch=True)[0] for n in ("edge-whole", "edge-tables")] == [TABLES, NOTHING]
    print("N* = %d spheres beside the light: LDS %d bytes staged whole, %d at N* + 1 (tables); P* = %d prisms beside %d spheres and %d "
          "circles: LDS %d bytes with the tables staged, %d at P* + 1 (nothing staged)" % ((th["N"],) + th["lds"][:2] + (th["P"], 3000, th["C"]) + th["lds"][2:]))
    assert tuple(stages[n][1] for n in ("edge-whole", "edge-whole+1", "edge-tables", "edge-tables+1")) == th["lds"]
    assert [stages[n][0] for n in ("edge-whole", "edge-whole+1", "edge-tables", "edge-tables+1")] == [WHOLE, TABLES, TABLES, NOTHING]
    for low in ("edge-whole", "edge-tables"):
        assert M.LDS_BYTES - 512 < stages[low][1] <= M.LDS_BYTES, (low, stages[low])
    a, b = lays["edge-whole"], lays["edge-whole+1"]
    same = ("n_prism_records", "n_prisms", "n_prism_groups", "prism_cylinders", "n_planes", "n_parabs", "n_cluster_supers")
    assert all(a[k] == b[k] for k in same) and a["n_cluster_supers"] == 0 and a["prism_cylinders"] == 0, (a, b)
    assert int((_case("edge-whole").objs["surface_kind"] == 0).sum()) == th["N"] + 1 == int((_case("edge-whole+1").objs["surface_kind"] == 0).sum()) - 1
    a, b = lays["edge-tables"], lays["edge-tables+1"]
    assert (a["n_prisms"], b["n_prisms"]) == (th["P"], th["P"] + 1) and a["n_planes"] == b["n_planes"] == 2 + th["C"], (a, b)
    assert a["prism_cylinders"] == b["prism_cylinders"] == 1 and a["n_cluster_supers"] == b["n_cluster_supers"], (a, b)
    # the scratch the rule was applied with: a third level's ring T counts as scratch (8 KB of a 16-wave workgroup's 160)
    assert M.scratch_bytes(a) == 16 * 8192 + (16 * 512 if a["n_cluster_supers"] else 0)


@pytest.mark.parametrize("name", EXTREME_SCENES)
def test_mirror_renders_the_oracles_photons_and_the_planner_gives_the_shape_claimed(name):
    c = _case(name)
    kinds, lay = c.objs["surface_kind"], c.lay
    n = 8192 if len(c.objs) < 500 else 2048
    want, segs = c.so.render(320, 180, 7, 1, 12345, n, threads=16)
    got, segs2 = c.sm.render(320, 180, 7, 1, 12345, n)
    assert segs == segs2 and got.tobytes() == want.tobytes(), name
    has_light = bool((c.objs["material_kind"] == 0).any())
    assert bool((want["probability"] > 0).any()) == has_light, name         # (a scene without an emitter renders black, and only that one)
    print("%s: %.2f segments a path, %.1f %% of the photons are not black" % (name, segs / n, 100.0 * (want["probability"] > 0).mean()))
    assert name.startswith("min-") or segs >= 1.5 * n, (name, segs, n)    # (no glowing wall in front of the camera ends every path at once)
    # no record lost or made: the flattened tables hold what the description does, plus the dummies of short prism groups
    assert lay["n_prisms"] == int((kinds == 4).sum()) and lay["n_planes"] == int(((kinds == 1) | (kinds == 2)).sum()), (name, lay)
    assert lay["n_parabs"] == int((kinds == 3).sum()) and M.small_counts(c.sm) == (lay["n_parabs"], lay["n_planes"]), (name, lay)
    assert lay["n_prism_records"] == 3 * lay["n_prism_groups"] and lay["n_prism_groups"] == -(-lay["n_prisms"] // 3), (name, lay)
    assert lay["prism_cylinders"] == int(lay["n_bounded_prisms"] >= 40) and lay["n_bounded_prisms"] <= lay["n_prisms"], (name, lay)
    assert len(M.prism_cylinders(c.sm)) == (lay["n_prism_records"] if lay["prism_cylinders"] else 0), name
    assert lay["n_cluster_supers"] == len(M.super_bounds(c.sm)[0]), name
    assert lay["staged_bytes"] <= lay["blob_bytes"] < lay["staged_bytes"] + 81 * 16 + 32 and lay["table_bytes"] < lay["staged_bytes"], (name, lay)
    n_small_parabs, n_small_planes = lay["n_parabs"], lay["n_planes"]
    first_plane = int(np.flatnonzero((kinds == 1) | (kinds == 2))[0]) if n_small_planes else len(kinds)
    last_parab = int(np.flatnonzero(kinds == 3)[-1]) if n_small_parabs else -1
    assert M.small_ordered(c.sm) == (last_parab < first_plane), name
    stage, lds = M.predicted_stage(lay)
    print("%s: %r -> stage %d, %d bytes of LDS" % (name, lay, stage, lds))
    if name in SHAPES:
        spheres, prisms, records, planes, parabs, ordered, want_stage = SHAPES[name]
        assert (int((kinds == 0).sum()), lay["n_prisms"], lay["n_prism_records"], planes, parabs, M.small_ordered(c.sm), stage) == \
            (spheres, prisms, records, lay["n_planes"], lay["n_parabs"], ordered, want_stage), (name, lay, stage)
        assert lay["n_cluster_supers"] == 0 and (lay["n_clusters"] > 0) == (spheres >= 40), (name, lay)
    else:
        assert (lay["n_prisms"], lay["n_planes"], lay["n_parabs"], M.small_ordered(c.sm)) == \
            ((6, 4) if "whole" in name else (_thresholds()["P"] + name.endswith("+1") - 9 * name.endswith("-open"), 2 + _thresholds()["C"])) + (1, False), (name, lay)
        if name == "edge-tables-open":     # the tables are staged in an open launch of the trace kernel too, beside 40 prisms or more
            assert M.predicted_stage(lay, open_launch=True)[0] == stage == TABLES and lay["prism_cylinders"] == 1, (name, lay)
    # the rule's other inputs: an open launch of the trace kernel carries 2,064 bytes more scratch, global fetch stages nothing
    assert M.predicted_stage(lay, open_launch=True)[0] <= stage and M.predicted_stage(lay, lds_fetch=False)[0] == NOTHING


def test_the_prism_remainders_are_the_ones_named():
    """39 prisms: 13 full groups and no cylinders; 40: the switch, and a last group of one with two dummies; 41: a last group of two
    with one."""
    for name, (groups, dummies, cyl) in {"prisms-39": (13, 0, 0), "prisms-40": (14, 2, 1), "prisms-41": (14, 1, 1)}.items():
        lay = _case(name).lay
        assert (lay["n_prism_groups"], lay["n_prism_records"] - lay["n_prisms"], lay["prism_cylinders"]) == (groups, dummies, cyl), (name, lay)
        assert lay["n_bounded_prisms"] == lay["n_prisms"], (name, lay)     # (every one counts for the switch)
        b, n_clusters = M.bounds(_case(name).sm)
        assert len(b) - n_clusters == lay["n_prism_records"] and int((b[n_clusters:, 3] == -np.inf).sum()) == dummies, name
        per_group = np.sort((b[n_clusters:, 3] == -np.inf).reshape(-1, 3).sum(axis=1))[::-1]
        assert per_group[0] == dummies and not per_group[1:].any(), (name, per_group)      # ONE short group: of one prism, of two


@pytest.mark.parametrize("name", list(EXTREME_PRISMS) + ["prisms-stack-200"])
def test_a_tenth_of_the_camera_and_bounce_rays_hit_a_prism_first(name):
    c = _case(name)
    for kind in ("camera", "bounce"):
        hit_kinds, _, n = _first_hits(c, kind)
        share = float((hit_kinds == 4).sum()) / n
        print("%s %s: %d rays, %.1f %% hit a prism first" % (name, kind, n, 100 * share))
        assert n >= 256 and share >= 0.10, (name, kind, share)


def test_a_camera_ray_passes_a_hundred_prism_bounds_of_the_stack():
    """From the mirror's level-1 bounds {centre, radius^2}: the ray's line comes within the radius ahead of the origin."""
    c = _case("prisms-stack-200")
    b, n_clusters = M.bounds(c.sm)
    b = b[n_clusters:].astype(np.float64)
    b = b[b[:, 3] != -np.inf]
    assert len(b) == 200
    o, d = (a.astype(np.float64) for a in c.sets["camera"])
    co = b[None, :, :3] - o[:, None, :]
    along = np.einsum("rpk,rk->rp", co, d)
    dist2 = (co * co).sum(axis=2) - along * along
    passes = ((dist2 <= b[None, :, 3]) & (along > 0)).sum(axis=1)
    centres = c.objs["v1"][c.objs["surface_kind"] == 4] + 0.5 * c.objs["f"][c.objs["surface_kind"] == 4][:, 3:4] * c.objs["v0"][c.objs["surface_kind"] == 4]
    print("prisms-stack-200: a camera ray passes %.1f prism bounds on average (least %d, most %d)" % (passes.mean(), passes.min(), passes.max()))
    assert np.linalg.norm(centres, axis=1).max() <= 0.5 + 1e-5 and passes.mean() >= 100.0, passes.mean()


@pytest.mark.parametrize("name", [n for n in EXTREME_SMALL if n != "small-0"])
def test_a_tenth_of_first_hits_are_small_primitives_and_the_65th_is_among_them(name):
    """Over the camera and bounce families together.  A primitive's position in its table is its rank among the description's
    planes and circles, or among its paraboloids: the tables are filled in object order."""
    c = _case(name)
    kinds = c.objs["surface_kind"]
    flat, parab = (kinds == 1) | (kinds == 2), kinds == 3
    position = np.where(flat, np.cumsum(flat) - 1, np.where(parab, np.cumsum(parab) - 1, -1))
    obj = np.concatenate([_first_hits(c, kind)[1] for kind in ("camera", "bounce")])
    small = float((position[obj] >= 0).mean())
    beyond = float((position[obj] >= 64).mean())
    print("%s: %d first hits, %.1f %% small primitives, %.1f %% at table position 64 or beyond" % (name, len(obj), 100 * small, 100 * beyond))
    assert len(obj) >= 1024 and small >= 0.10, (name, small)
    if max(c.lay["n_planes"], c.lay["n_parabs"]) >= 65:
        assert beyond >= 0.01, (name, beyond)
    if name == "small-mixed-130":          # both tables reach their 65th record
        assert (position[obj][kinds[obj] == 3] >= 64).any() and (position[obj][kinds[obj] != 3] >= 64).any(), name


def test_small_0_has_no_small_primitive_at_all():
    c = _case("small-0")
    assert not np.isin(c.objs["surface_kind"], (1, 2, 3)).any() and (c.lay["n_planes"], c.lay["n_parabs"]) == (0, 0)
    assert (c.want["camera"]["object"] != NONE).any() and (c.want["camera"]["object"] == NONE).any()


def test_a_tenth_of_the_hits_on_the_coincident_planes_tie_exactly():
    c = _case("planes-coincident-50")
    kinds, mats = c.objs["surface_kind"], c.objs["material_kind"]
    same = np.flatnonzero((kinds == 1) | (kinds == 2))
    assert len(same) == 100 and len(np.unique(c.objs["v0"][same], axis=0)) == 1 and len(np.unique(c.objs["v1"][same], axis=0)) == 1
    assert (kinds[same] == 1).sum() == 50 and len(set(mats[same].tolist())) == 6 and (np.diff(same) > 1).any()   # (permuted among the rest)
    o, d = c.sets["camera"][0][:512], c.sets["camera"][1][:512]
    want = c.want["camera"][:512]
    hit = want["object"] != NONE
    tied = tied_hits(c.so, want, o, d)
    share = float(tied[hit].mean())
    winners = want["object"][hit & tied]
    print("planes-coincident-50: %d hits, %.1f %% tied; the winners %s" % (hit.sum(), 100 * share, np.unique(winners)))
    assert hit.sum() >= 256 and share >= 0.10, share
    assert np.isin(winners, same).all() and set(np.unique(winners).tolist()) <= {int(same[kinds[same] == 1].min()), int(same.min())}


@pytest.mark.parametrize("name", MINIMAL_SCENES)
def test_hits_and_misses_both_occur_on_a_minimal_scene(name):
    c = _case(name)
    hit = c.want["camera"]["object"] != NONE
    print("%s: %d objects, %d of %d camera rays hit" % (name, len(c.objs), hit.sum(), len(hit)))
    assert 0.02 < hit.mean() < 0.98, (name, hit.mean())
    emitters = int((c.objs["material_kind"] == 0).sum())
    assert emitters == {"min-sphere-emitter": 1, "min-prism": 0, "min-plane": 0, "min-emitters": 6}[name]
