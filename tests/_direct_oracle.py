"""rl_plot_unit_render_direct's contract, composed twice from what the tests already have -- once on the CPU oracles alone
(camera, _step_oracle, _light_oracle, _light_film_oracle) and once from the public GPU calls (camera_rays, begin_paths,
step_path_list with hits, light_paths) -- with the call's RlDirectStats counted from the sample statuses.  Both keep every photon's
path and every count per path, so that one run over n paths answers for every prefix of them.  Nothing is built at import."""
import ctypes as C

import numpy as np

import _light_film_oracle as FO

LIVE, NONE = 0xffffffff, 0xffffffff
END_EMITTER, END_LIMIT = 1, 3
SKIPPED, BACKFACING, OCCLUDED, VISIBLE = range(4)
MAX_SEGMENTS = 4096      # max_segments = 0
STATS = ("paths", "segments", "light_samples", "shadow_rays", "visible", "endings_kept", "endings_dropped")
RESULT_DTYPE = np.dtype([("value", "<f4"), ("segments", "<u4"), ("object", "<u4"), ("end", "<u4")])
CAMERA_DTYPE = np.dtype([("ray", [("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")]),
                         ("x", "<f4"), ("y", "<f4"), ("reserved0", "<u4"), ("reserved1", "<u4")])
assert RESULT_DTYPE.itemsize == 16 and CAMERA_DTYPE.itemsize == 48


class Direct:
    """What a direct render of n paths must produce: `results` (n RlPathResult records), the film's `photons` in call order with
    the path (0 .. n - 1) each comes from, every sample `status` seen, and the stats per path."""

    def __init__(self, results, photons, rows, per_path, statuses):
        self.results, self.photons, self.rows, self.per_path, self.statuses = results, photons, rows, per_path, statuses

    def prefix(self, n):
        """(results, photons, stats) of the first n paths alone: a path's draws depend on its own index only."""
        stats = {name: int(self.per_path[name][:n].sum()) for name in STATS}
        return self.results[:n], self.photons[self.rows < n], stats

    def span(self, lo, hi):
        """The stats of paths lo .. hi - 1."""
        return {name: int(self.per_path[name][lo:hi].sum()) for name in STATS}


def _compose(camera, emitters, hit_dtype, begin, step, light, first, max_segments):
    """The loop rl_plot_unit_render_samples_direct's contract names.  begin(rays, first) -> states; step(states, hits, list, n_list)
    steps the listed states in place with hits and returns the live ones' list; light(states, hits, list, n_list) -> samples."""
    n = len(camera)
    st = begin(np.ascontiguousarray(camera["ray"]), first)
    hits = np.zeros(n, hit_dtype)
    hits["object"] = NONE
    sampled = np.zeros(n, np.uint8)
    per_path = {name: np.zeros(n, np.int64) for name in STATS}
    per_path["paths"][:] = 1
    photons, rows, statuses = [np.zeros(0, FO.PHOTON_DTYPE)], [np.zeros(0, np.int64)], set()
    lst, n_list = None, n
    for _ in range(max_segments or MAX_SEGMENTS):
        if n_list == 0:
            break
        named = FO.listed_states(n, lst, n_list)
        per_path["segments"][named] += 1
        live = step(st, hits, lst, n_list)
        samples = light(st, hits, lst, n_list)
        status = samples["status"][named]
        statuses.update(int(s) for s in np.unique(status))
        per_path["light_samples"][named] += status != SKIPPED
        per_path["shadow_rays"][named] += (status == OCCLUDED) | (status == VISIBLE)
        per_path["visible"][named] += status == VISIBLE
        ending = (st["end"][named] == END_EMITTER) & (st["value"][named] != 0)
        counted = (sampled[named] != 0) & np.isin(st["object"][named], np.asarray(emitters, dtype=np.uint32))
        per_path["endings_kept"][named] += ending & ~counted
        per_path["endings_dropped"][named] += ending & counted
        ph, from_rows, sampled = FO.film_photon_rows(st, samples, emitters, camera, sampled, lst, n_list)
        photons.append(ph)
        rows.append(from_rows)
        lst, n_list = live, len(live)
    # what rl_scene_render_rays writes for a path, from the state the loop left: a state that is still live used up max_segments
    live = st["end"] == LIVE
    results = np.zeros(n, RESULT_DTYPE)
    results["value"], results["segments"] = np.where(live, np.float32(0), st["value"]), st["segments"]
    results["object"], results["end"] = np.where(live, NONE, st["object"]), np.where(live, END_LIMIT, st["end"])
    return Direct(results, np.concatenate(photons), np.concatenate(rows), per_path, statuses)


def oracle_camera_samples(objs, cam, w, h, seed, stream, first, n):
    """rl_scene_camera_rays on the CPU: the first ray of each path from the host compile of the kernel's path header
    (mirror_dump_rays), the wavelength and the film position from the oracle's render of the same paths, which records them with
    every photon (trace_unit.rs:151-168)."""
    import _mirror as M
    import _oracle as O
    ms = M.Scene(objs, cam)
    dump = M.lib().mirror_dump_rays
    dump.restype = C.c_uint64
    dump.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    rays6 = np.zeros((n, 6), np.float32)
    for i in range(n):
        assert dump(ms.h, w, h, seed, stream, first + i, 1, rays6[i].ctypes.data, 1) == 1
    drawn, _ = O.Scene(objs, cam).render(w, h, seed, stream, first, n, threads=16)
    camera = np.zeros(n, CAMERA_DTYPE)
    camera["ray"]["origin"], camera["ray"]["direction"], camera["ray"]["wavelength"] = rays6[:, :3], rays6[:, 3:], drawn["wavelength"]
    camera["x"], camera["y"] = drawn["x"], drawn["y"]
    return camera


def cpu_direct(objs, cam, w, h, seed, stream, first, n, max_segments):
    """The contract on the CPU oracles alone, for the camera of a w x h film."""
    import _light_oracle as LO
    import _step_oracle as S
    camera = oracle_camera_samples(objs, cam, w, h, seed, stream, first, n)
    stepper, occluder = S.StepOracle(objs, cam), LO.Occluder(objs, cam)

    def step(st, hits, lst, n_list):
        named = FO.listed_states(len(st), lst, n_list)
        sub, sub_hits = st[named], hits[named]
        stepper.step(sub, seed, stream, hits=sub_hits)
        st[named], hits[named] = sub, sub_hits
        return named[sub["end"] == LIVE].astype(np.uint32)

    def light(st, hits, lst, n_list):
        return LO.light_paths(occluder, st, hits, seed, stream, list=lst, n_list=n_list)

    return _compose(camera, LO.emitters(objs), S.HIT_DTYPE, S.begin, step, light, first, max_segments)


def gpu_loop(scene, w, h, seed, stream, first, n, max_segments, fetch=0):
    """The same composition from the public GPU calls (the loop of public calls of tests/test_gpu_light_film.py, without a plot
    unit: the photons are the rule's, tests/_light_film_oracle.py): (camera samples, Direct)."""
    camera = scene.camera_rays(w, h, seed, stream, first, n)

    def step(st, hits, lst, n_list):
        return scene.step_path_list(st, seed, stream, list=lst, n_list=n_list, fetch=fetch, hits=hits)

    def light(st, hits, lst, n_list):
        return scene.light_paths(st, hits, seed, stream, list=lst, n_list=n_list, fetch=fetch)

    import robigo_luculenta_amd as R
    return camera, _compose(camera, scene.emitters(), R.HIT_DTYPE, scene.begin_paths, step, light, first, max_segments)
