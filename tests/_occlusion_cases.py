"""Ray sets for Scene.occluded beyond those of Scene.intersect (tests/test_gpu_occlusion.py): shadow rays from first hits towards
points on the scene's black-body objects, and short rays from first hits in uniform directions.  Host arithmetic only (numpy): the
first hits come from whoever calls, so the sets can be made from the CPU oracle's hits."""
import numpy as np

NONE = 0xffffffff
BLACK_BODY = 0
SPHERE, PLANE, CIRCLE = 0, 1, 2
OFFSET = np.float32(1e-5)
PROBES = 16


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def start_points(directions, hits):
    """Where a secondary ray leaves a first hit: the hit's position moved 1e-5 along the normal, to the side the ray came from
    (f32).  Misses are dropped: returns (origins, that side's unit normals, the mask of hits)."""
    m = hits["object"] != NONE
    n = hits["normal"][m].astype(np.float32)
    facing = np.sign(-(n * directions[m]).sum(axis=1, dtype=np.float32)).astype(np.float32)
    facing[facing == 0] = 1
    out = facing[:, None] * n
    return np.ascontiguousarray(hits["position"][m] + OFFSET * out, dtype=np.float32), out, m


def light_points(objs, rng, origins):
    """One point on the scene's black-body objects per origin.  Even rows: on an object drawn uniformly among them -- on a sphere's
    surface (half of those lie behind the sphere itself), within a circle, on a plane within 10 units of its offset point, and
    the offset point v1 itself for the other surfaces.  Odd rows: the point of the NEAREST black-body sphere that faces the origin.
    (n, 3) float64; objects with non-finite data are left out, and a scene without a usable emitter aims at its origin."""
    n = len(origins)
    lights = objs[objs["material_kind"] == BLACK_BODY]
    ok = np.isfinite(lights["v0"]).all(axis=1) & np.isfinite(lights["v1"]).all(axis=1) & np.isfinite(lights["f"][:, 0])
    lights = lights[ok]
    if not len(lights):
        return np.zeros((n, 3))
    pick = lights[rng.integers(0, len(lights), n)]
    kind = pick["surface_kind"]
    u = _unit(rng, n)
    v0, v1, r = pick["v0"].astype(np.float64), pick["v1"].astype(np.float64), pick["f"][:, 0].astype(np.float64)
    pts = v1.copy()
    sph = kind == SPHERE
    pts[sph] = v0[sph] + r[sph, None] * u[sph]
    flat = (kind == PLANE) | (kind == CIRCLE)
    # a random in-plane offset: u without its component along the normal, scaled
    nrm = v0 / np.maximum(np.linalg.norm(v0, axis=1, keepdims=True), 1e-30)
    inplane = u - (u * nrm).sum(axis=1, keepdims=True) * nrm
    reach = np.where(kind == CIRCLE, r, 10.0) * rng.random(n)
    pts[flat] = (v1 + reach[:, None] * inplane)[flat]
    balls = lights[(lights["surface_kind"] == SPHERE) & (lights["f"][:, 0] > 0)]
    if len(balls):
        c, rad = balls["v0"].astype(np.float64), balls["f"][:, 0].astype(np.float64)
        odd = np.arange(n) % 2 == 1
        o = origins[odd].astype(np.float64)
        near = np.zeros(len(o), np.int64)
        for lo in range(0, len(o), 16384):   # (in chunks: millions of origins x a thousand spheres)
            oc = o[lo:lo + 16384]
            d2 = (oc * oc).sum(axis=1)[:, None] - 2.0 * (oc @ c.T) + (c * c).sum(axis=1)[None, :]
            near[lo:lo + 16384] = np.abs(np.sqrt(np.maximum(d2, 0.0)) - rad[None, :]).argmin(axis=1)   # distance to each sphere's surface
        out = o - c[near]
        out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-30)
        pts[odd] = c[near] + rad[near, None] * out
    return pts


def _aim(o, points):
    """Directions (normalised in f32) and distances (f32) from origins o to points."""
    to = (points.astype(np.float32) - o).astype(np.float32)
    dist = np.sqrt((to * to).sum(axis=1, dtype=np.float32), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (to / dist[:, None]).astype(np.float32), dist


def seen_light_points(objs, origins, outward, rng, oracle):
    """For every origin a point on a black-body object that the CPU oracle says it sees, where probing finds one: up to PROBES
    directions in the hemisphere around `outward` are cast with oracle(origins, directions) -> HIT records, and the first whose
    nearest hit lies on a black-body object gives that hit's position.  Among thousands of spheres no ray aimed at an emitter
    reaches it by chance; this way some do.  Returns (points, found)."""
    n = len(origins)
    points, found = np.zeros((n, 3)), np.zeros(n, bool)
    emits = objs["material_kind"] == BLACK_BODY
    for _ in range(PROBES):
        todo = np.flatnonzero(~found)
        if not len(todo):
            break
        d = outward[todo].astype(np.float64) + 0.95 * _unit(rng, len(todo))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        hits = oracle(origins[todo], d)
        lit = hits["object"] != NONE
        lit[lit] = emits[hits["object"][lit]]
        points[todo[lit]] = hits["position"][lit]
        found[todo[lit]] = True
    return points, found


def shadow_rays(objs, directions, hits, rng, oracle=None):
    """(origins, directions, t_max): from the first hits towards light_points(); t_max is the distance to the point and the
    direction is normalised, both in f32 -- so the ray ends on the emitter's surface, within rounding.  With oracle (the CPU
    oracle's Scene::intersect for given rays) every fourth ray aims at a point of an emitter that seen_light_points() found
    visible from it, where it found one."""
    o, outward, m = start_points(directions, hits)
    points = light_points(objs, rng, o)
    if oracle is not None:
        rows = np.flatnonzero(np.arange(len(o)) % 4 == 1)
        seen, found = seen_light_points(objs, o[rows], outward[rows], rng, oracle)
        points[rows[found]] = seen[found]
    to, dist = _aim(o, points)
    keep = dist > 0
    return o[keep], np.ascontiguousarray(to[keep]), dist[keep]


def short_rays(directions, hits, rng):
    """(origins, directions, t_max): from the first hits in uniform directions, t_max drawn from (0, 1)."""
    o, outward, m = start_points(directions, hits)
    t = rng.random(len(o)).astype(np.float32)
    t[t == 0] = np.float32(0.5)
    return o, _unit(rng, len(o)).astype(np.float32), t
