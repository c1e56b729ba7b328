"""ctypes view of tests/host_mirror (the kernel's per-path header compiled with g++).  Test-only."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "host_mirror", "_build", "librl_mirror.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "host_mirror")], check=True)
        L = C.CDLL(SO)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.mirror_scene_create.restype = vp
        L.mirror_scene_create.argtypes = [vp, u32, vp]
        L.mirror_scene_destroy.argtypes = [vp]
        L.mirror_builtin_desc.restype = u32
        L.mirror_builtin_desc.argtypes = [C.c_int, C.c_int, vp, u32, vp]
        L.mirror_render.argtypes = [vp, u32, u32, u64, u32, u64, u64, vp, vp]
        L.mirror_plot.argtypes = [vp, u32, u32, vp, u64]
        L.mirror_prism_fast_check.argtypes = [vp, u64, u64, vp]
        L.mirror_prism_fast_check_band.argtypes = [vp, u64, u64, C.c_double, C.c_double, vp]
        L.mirror_prism_fast_check_paths.argtypes = [vp, u32, u32, u64, u32, u64, u64, vp]
        L.mirror_prism_cylinders.restype = u32
        L.mirror_prism_cylinders.argtypes = [vp, vp, u32]
        L.mirror_cull_counts.argtypes = [vp, u32, u32, u64, u32, u64, u64, vp]
        L.mirror_prism_pairs.restype = u64
        L.mirror_prism_pairs.argtypes = [vp, u64, u64, vp, vp, vp, u64]
        L.mirror_prism_pairs_band.restype = u64
        L.mirror_prism_pairs_band.argtypes = [vp, u64, u64, C.c_double, C.c_double, vp, vp, vp, u64]
        _lib = L
    return _lib


def builtin_desc(which, param=0):
    cam = O.RlCameraDesc()
    n = lib().mirror_builtin_desc(which, param, None, 0, C.byref(cam))
    objs = np.zeros(n, dtype=O.OBJECT_DTYPE)
    lib().mirror_builtin_desc(which, param, O.ptr(objs), n, C.byref(cam))
    return objs, cam


class Scene:
    def __init__(self, objs, cam):
        self.objs = np.ascontiguousarray(objs)
        self.h = lib().mirror_scene_create(O.ptr(self.objs), len(self.objs), C.byref(cam))
        assert self.h

    def __del__(self):
        try:
            lib().mirror_scene_destroy(self.h)
        except Exception:
            pass

    def render(self, w, h, seed, stream, first, n):
        photons = np.zeros(n, dtype=O.PHOTON_DTYPE)
        segs = C.c_uint64(0)
        lib().mirror_render(self.h, w, h, seed, stream, first, n, O.ptr(photons), C.byref(segs))
        return photons, segs.value


def prism_fast_check(scene, trials, seed, band=None):
    """rl_hex_prism_fast against rl_hex_prism on random and adversarial (prism, ray) pairs of `scene`:
    {pairs, decided hits, decided misses, undecided, decided-but-different (must be 0), tree hits}.
    With band = (lo, hi): on unit rays from 10^lo .. 10^hi units away from the prism instead, a quarter of the origins displaced
    along one axis only, three quarters of the directions aimed into the prism's bound from the rounded origin."""
    counts = np.zeros(6, dtype=np.uint64)
    if band is not None:
        lib().mirror_prism_fast_check_band(scene.h, trials, seed, float(band[0]), float(band[1]), O.ptr(counts))
    else:
        lib().mirror_prism_fast_check(scene.h, trials, seed, O.ptr(counts))
    return dict(zip(("pairs", "hits", "misses", "undecided", "wrong", "tree_hits"), (int(c) for c in counts)))


def prism_fast_check_paths(scene, w, h, seed, stream, first, n):
    """The same comparison on the (prism, ray) pairs that paths [first, first + n) produce."""
    counts = np.zeros(6, dtype=np.uint64)
    lib().mirror_prism_fast_check_paths(scene.h, w, h, seed, stream, first, n, O.ptr(counts))
    return dict(zip(("pairs", "hits", "misses", "undecided", "wrong", "tree_hits"), (int(c) for c in counts)))


def prism_pairs(scene, trials, seed, band=None):
    """The adversarial (prism, ray) pairs of prism_fast_check, or the pairs of its `band`, as data: prism numbers, rays (n x 6), the
    tree's {t bits, half-space}."""
    prisms = np.zeros(trials, dtype=np.uint32)
    rays = np.zeros((trials, 6), dtype=np.float32)
    tree = np.zeros((trials, 2), dtype=np.uint32)
    if band is not None:
        n = lib().mirror_prism_pairs_band(scene.h, trials, seed, float(band[0]), float(band[1]), O.ptr(prisms), O.ptr(rays), O.ptr(tree), trials)
    else:
        n = lib().mirror_prism_pairs(scene.h, trials, seed, O.ptr(prisms), O.ptr(rays), O.ptr(tree), trials)
    return prisms[:n], rays[:n], tree[:n]


def prism_cylinders(scene, cap=4096):
    """The prisms' second bound as (n, 8) floats {point on the axis, radius, unit axis, 0}; empty when the scene does not use it."""
    out = np.zeros((cap, 8), dtype=np.float32)
    n = lib().mirror_prism_cylinders(scene.h, O.ptr(out), cap)
    return out[:n]


def plot(w, h, photons):
    buffer = np.zeros((h * w, 3), dtype=np.float32)
    photons = np.ascontiguousarray(photons)
    lib().mirror_plot(O.ptr(buffer), w, h, O.ptr(photons), len(photons))
    return buffer


def small_ordered(scene):
    """RlFlatScene::small_ordered of `scene`: the kernel may take `t < best.t` for scene.rs:51's tie rule among the small primitives."""
    L = lib()
    L.mirror_small_ordered.restype = C.c_int
    L.mirror_small_ordered.argtypes = [C.c_void_p]
    return bool(L.mirror_small_ordered(scene.h))


def small_axis_z(scene):
    """RlFlatScene::small_axis_z of `scene`: every paraboloid's, plane's and circle's normal lies along z."""
    L = lib()
    L.mirror_small_axis_z.restype = C.c_int
    L.mirror_small_axis_z.argtypes = [C.c_void_p]
    return bool(L.mirror_small_axis_z(scene.h))


def small_counts(scene):
    """(paraboloids, planes and circles) in `scene`'s flattened tables: the n_parabs and n_planes the kernel's scan branches on."""
    L = lib()
    L.mirror_small_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    a, b = C.c_uint32(0), C.c_uint32(0)
    L.mirror_small_counts(scene.h, C.byref(a), C.byref(b))
    return a.value, b.value


def super_bounds(scene, cap=4096):
    """The third level of `scene`'s cull table: ((n, 4) floats {centre, radius^2} per super, cluster groups per super); n = 0 for a
    two-level table."""
    L = lib()
    L.mirror_super_bounds.restype = C.c_uint32
    L.mirror_super_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    sup, sg = np.zeros((cap, 4), np.float32), C.c_uint32(0)
    n = L.mirror_super_bounds(scene.h, O.ptr(sup), cap, C.byref(sg))
    assert n <= cap
    return sup[:n], sg.value


def bounds(scene, cap=1 << 16):
    """The level-1 bounds of `scene`'s cull table as ((n, 4) floats {centre, radius^2}, number of cluster bounds in front): the
    sphere clusters' first, then one per prism record (a dummy prism's radius^2 is -inf)."""
    L = lib()
    L.mirror_bounds.restype = C.c_uint32
    L.mirror_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    out, nc = np.zeros((cap, 4), np.float32), C.c_uint32(0)
    n = L.mirror_bounds(scene.h, O.ptr(out), cap, C.byref(nc))
    assert n <= cap
    return out[:n], nc.value


LAYOUT_FIELDS = ("staged_bytes", "blob_bytes", "table_bytes", "n_prism_records", "n_prisms", "n_prism_groups", "prism_cylinders",
                 "n_planes", "n_parabs", "n_cluster_supers", "n_clusters", "n_direct", "n_bounded_prisms")


def layout(scene):
    """mirror_layout of `scene` as a dict over LAYOUT_FIELDS: RlFlatScene::staged_bytes(), the bytes of the blob rl_scene_create
    makes of the flat scene and of its tables (the records [off_planes, off_objects)), and the counts the kernel variants and the
    scan's loops depend on.  n_prisms counts the description's prisms, n_prism_records those and the dummies that fill short groups,
    n_bounded_prisms the ones whose bound is finite: the count rl_flatten_scene's cylinder switch is made on."""
    L = lib()
    L.mirror_layout.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(len(LAYOUT_FIELDS), np.uint64)
    L.mirror_layout(scene.h, O.ptr(out))
    return dict(zip(LAYOUT_FIELDS, (int(v) for v in out)))


# ---- the staging rule (rl_api.hip: stage_of), stated once for the tests -----------------------------------------------------------

STAGE_NONE, STAGE_TABLES, STAGE_ALL = 0, 1, 2
LDS_BYTES = 160 * 1024
_CONSTANTS = None


def launch_constants():
    """{block, wave_scratch, open_cap} as the product's kernel header states them (RL_TRACE_BLOCK, sizeof(RlWaveScratch) by its
    static_assert, RL_OPEN_CAP): read from csrc/rl_kernels.hip.h, which only hipcc compiles, so that no figure is repeated here."""
    global _CONSTANTS
    if _CONSTANTS is None:
        import re
        with open(os.path.join(HERE, "..", "robigo_luculenta_amd", "csrc", "rl_kernels.hip.h")) as f:
            text = f.read()
        found = {}
        for key, pattern in (("block", r"#define RL_TRACE_BLOCK (\d+)"), ("wave_scratch", r"static_assert\(sizeof\(RlWaveScratch\) == (\d+)"),
                             ("open_cap", r"#define RL_OPEN_CAP (\d+)u")):
            m = re.findall(pattern, text)
            assert len(m) == 1, (key, m)
            found[key] = int(m[0])
        _CONSTANTS = found
    return _CONSTANTS


def scratch_bytes(lay, open_launch=False):
    """The LDS a launch asks for beside what it stages: one RlWaveScratch per wave of the workgroup; 512 bytes per wave of ring T
    where the cull table has a third level (ring_t_bytes); and, in an open launch of the trace kernel, one RlOpenWg (two uint32 per
    job slot and four more)."""
    c = launch_constants()
    waves = c["block"] // 64
    return waves * c["wave_scratch"] + (waves * 512 if lay["n_cluster_supers"] else 0) + ((2 * c["open_cap"] + 4) * 4 if open_launch else 0)


def predicted_stage(lay, lds_fetch=True, open_launch=False):
    """(stage, LDS bytes the launch asks for) as stage_of decides them for a scene of layout `lay`: under RL_FETCH_LDS the whole blob,
    rounded up to 512 bytes, if it fits in 160 KB beside the scratch and the cull table has no third level; else the tables, rounded
    likewise, if they do; else nothing.  Nothing under RL_FETCH_GLOBAL."""
    scratch = scratch_bytes(lay, open_launch)
    if not lds_fetch:
        return STAGE_NONE, scratch
    whole, tables = (lay["blob_bytes"] + 511) & ~511, (lay["table_bytes"] + 511) & ~511
    if lay["n_cluster_supers"] == 0 and whole + scratch <= LDS_BYTES:
        return STAGE_ALL, whole + scratch
    if tables + scratch <= LDS_BYTES:
        return STAGE_TABLES, tables + scratch
    return STAGE_NONE, scratch


def axis_z_check(seed, n):
    """rl_paraboloid_t<AXIS_Z> / rl_plane_t<AXIS_Z> against the general forms: (cases, hits compared, differences, cases with a zero n.d / n.o)."""
    L = lib()
    L.mirror_axis_z_check.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    c = np.zeros(4, np.uint64)
    L.mirror_axis_z_check(seed, n, O.ptr(c))
    return tuple(int(x) for x in c)


def parab_check(seed, n):
    """The paraboloid's one-division form against the reference's selection: (cases, admitted, hits, disagreements, rejected tiny numerators)."""
    L = lib()
    L.mirror_parab_check.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    c = np.zeros(5, np.uint64)
    L.mirror_parab_check(seed, n, O.ptr(c))
    return tuple(int(x) for x in c)


def cull_counts(scene, w, h, seed, stream, first, n):
    """What the kernel's sphere pass does with `scene`'s cull table on the segments of paths [first, first + n), counted on
    the host: per segment the (group, ray), (cluster, ray) and (member, ray) pairs that pass, and the table's shape."""
    c = np.zeros(8, dtype=np.uint64)
    lib().mirror_cull_counts(scene.h, w, h, seed, stream, first, n, O.ptr(c))
    seg = float(c[0])
    return {"segments": int(c[0]), "groups": int(c[1]), "group_pairs": float(c[2]) / seg, "cluster_pairs": float(c[3]) / seg,
            "member_pairs": float(c[4]) / seg, "clusters": int(c[5]), "clusters_per_group": int(c[6]), "members_per_cluster": int(c[7])}
