"""robigo_luculenta_amd -- MI355X-native hot path of the spectral path tracer robigo-luculenta.

A thin ctypes mirror of the reference's unit structs over the C ABI (include/robigo_luculenta.h).
Class and method names follow the Rust sources: TraceUnit.render / PlotUnit.plot, clear /
GatherUnit.accumulate, save / TonemapUnit.tonemap / TaskScheduler.get_new_task.  All arithmetic
runs in hand-written gfx950 kernels; numpy is used only to hold downloaded buffers."""
import ctypes as C

import numpy as np

from ._lib import (RlAppConfig, RlAppStats, RlCameraDesc, RlCameraSample, RlError, RlIntersection, RlMappedPhoton, RlObjectDesc, RlPathResult,
                   RlPathState, RL_PATH_LIVE, RL_STEP_NO_ROULETTE, RlRay, RlRayHit, RlSceneDesc, RlSpectralRay, RlTask, RlVector3, check, lib, RL_OBJECT_NONE, RL_PATH_END_EMITTER,
                   RL_PATH_END_INVALID, RL_PATH_END_LIMIT, RL_PATH_END_ROULETTE, RL_PATH_END_VOID, RL_PATH_MAX_SEGMENTS,
                   RL_PATH_MAX_SEGMENTS_CAP, RL_TASK_MAX_UNITS, RlLightSample, RlDirectStats, RL_LIGHT_SKIPPED, RL_LIGHT_BACKFACING, RL_LIGHT_OCCLUDED,
                   RL_LIGHT_VISIBLE, RlFeatureSample, RlFeatureStats, RL_FEATURE_VOID, RL_FEATURE_EMITTER, RL_FEATURE_DIFFUSE, RL_FEATURE_LIMIT,
                   RL_FEATURE_MAX_SEGMENTS, RlDenoiseParams, RL_DENOISE_ITERATIONS, RL_DENOISE_MAX_ITERATIONS,
                   RL_SPECTRAL_MAX_NODES, RlErrorStats, RlErrorTarget, RlAppErrorStats, RL_ERROR_TILE, RlAdaptiveStats,
                   RlWavelengthSampling, RlRobustParams, RlRobustStats, RL_ROBUST_MAX_BUCKETS, RL_ROBUST_NEXT,
                   RL_RELIGHT_MAX_GROUPS, RL_RELIGHT_DROP, RL_GLARE_MAX_TAPS)

PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])
OBJECT_DTYPE = np.dtype([("surface_kind", "<u4"), ("material_kind", "<u4"), ("v0", "<f4", 3), ("v1", "<f4", 3),
                         ("f", "<f4", 4), ("m", "<f4", 3)])
# Scene.intersect's records: RlRay (32 bytes) and RlRayHit (48 bytes) of include/robigo_luculenta.h
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("distance", "<f4"), ("object", "<u4"),
                      ("reserved", "<u4")])
# Scene.camera_rays / render_rays records: RlSpectralRay (32 bytes), RlCameraSample (48 bytes) and RlPathResult (16 bytes)
SPECTRAL_RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])
CAMERA_SAMPLE_DTYPE = np.dtype([("ray", SPECTRAL_RAY_DTYPE), ("x", "<f4"), ("y", "<f4"), ("reserved0", "<u4"), ("reserved1", "<u4")])
PATH_RESULT_DTYPE = np.dtype([("value", "<f4"), ("segments", "<u4"), ("object", "<u4"), ("end", "<u4")])
# Scene.begin_paths / step_paths records: RlPathState (64 bytes)
PATH_STATE_DTYPE = np.dtype([("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("intensity", "<f4"),
                             ("continue_chance", "<f4"), ("segments", "<u4"), ("end", "<u4"), ("value", "<f4"), ("path_index", "<u8"),
                             ("object", "<u4"), ("reserved", "<u4")])
# Scene.light_paths records: RlLightSample (32 bytes)
LIGHT_SAMPLE_DTYPE = np.dtype([("direction", "<f4", 3), ("distance", "<f4"), ("value", "<f4"), ("weight", "<f4"), ("emitter", "<u4"),
                               ("status", "<u4")])
# Scene.render_features records: RlFeatureSample (48 bytes)
FEATURE_SAMPLE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("wavelength", "<f4"), ("albedo", "<f4"), ("normal", "<f4", 3), ("depth", "<f4"),
                                 ("object", "<u4"), ("segments", "<u4"), ("kind", "<u4"), ("reserved", "<u4")])
NUMBER_OF_PHOTONS = 1024 * 512  # trace_unit.rs:67

SCENE_DEMO, SCENE_GLASS_STRESS = 0, 1
FEATURE_VOID, FEATURE_EMITTER, FEATURE_DIFFUSE, FEATURE_LIMIT = RL_FEATURE_VOID, RL_FEATURE_EMITTER, RL_FEATURE_DIFFUSE, RL_FEATURE_LIMIT
FETCH_LDS, FETCH_GLOBAL = 0, 1
TASK_SLEEP, TASK_TRACE, TASK_PLOT, TASK_GATHER, TASK_TONEMAP = range(5)


def device_pci_bus_id(device=0):
    """PCI bus id of a visible device (rl_device_pci_bus_id)."""
    buf = C.create_string_buffer(64)
    check(lib.rl_device_pci_bus_id(device, buf, 64))
    return buf.value.decode()


def device_count():
    return lib.rl_device_count()


def version():
    return lib.rl_version().decode()


def build_id():
    return lib.rl_build_id().decode()


def builtin_scene_desc(which=SCENE_DEMO, param=0):
    """Object array (OBJECT_DTYPE) and camera of a built-in scene (app.rs:166-363)."""
    n = C.c_uint32(0)
    cam = RlCameraDesc()
    lib.rl_scene_builtin_desc(which, param, None, 0, C.byref(n), C.byref(cam))
    if n.value == 0:
        raise RlError(-1, "unknown built-in scene %r" % (which,))
    objs = np.zeros(n.value, dtype=OBJECT_DTYPE)
    check(lib.rl_scene_builtin_desc(which, param, objs.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(cam)))
    return objs, cam


def save_scene_desc(path, objects, camera):
    """Writes a scene description file (RLSC v1, see include/robigo_luculenta.h)."""
    objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
    desc = RlSceneDesc(len(objects), objects.ctypes.data_as(C.c_void_p), RlCameraDesc.from_buffer_copy(bytes(camera)))
    check(lib.rl_scene_desc_save(path.encode(), C.byref(desc)))


def load_scene_desc(path):
    n = C.c_uint32(0)
    cam = RlCameraDesc()
    rc = lib.rl_scene_desc_load(path.encode(), None, 0, C.byref(n), C.byref(cam))
    if rc not in (0, -1) or (rc == -1 and n.value == 0):
        check(rc)
    objs = np.zeros(n.value, dtype=OBJECT_DTYPE)
    check(lib.rl_scene_desc_load(path.encode(), objs.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(cam)))
    return objs, cam


def _n_bytes(t):
    """Size in bytes of a device buffer: anything with numel(), element_size() and data_ptr(), e.g. a torch tensor."""
    return t.numel() * t.element_size()


def _device_ptr(t):
    """The address of a device buffer, or None for a buffer that is not given."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _host_ptr(a):
    """The address of a numpy array, or None for an array that is not given."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _has_room(n, *rooms):
    """Whether each (device buffer, record size) of `rooms` whose buffer is given holds at least n records."""
    return all(t is None or _n_bytes(t) >= n * size for t, size in rooms)


def _record_count(buf, dtype, message, *rooms):
    """n, when device buffer `buf` holds n whole records of `dtype` and there is room for n in each of `rooms` (_has_room);
    ValueError(message) otherwise."""
    n = _n_bytes(buf) // dtype.itemsize
    if _n_bytes(buf) != n * dtype.itemsize or not _has_room(n, *rooms):
        raise ValueError(message)
    return n


def _host_list(list, n_list, n_states):
    """A host call's `list` and `n_list` as (None or a contiguous uint32 array, the number of entries): n_list defaults to the
    list's length, or to n_states for the identity list."""
    if list is None:
        return None, n_states if n_list is None else n_list
    list = np.ascontiguousarray(list, dtype=np.uint32)
    if n_list is None:
        n_list = len(list)
    if list.ndim != 1 or n_list > len(list):
        raise ValueError("list must be a one-dimensional array of at least n_list indices")
    return list, n_list


def _device_list(list, n_list, n_states):
    """n_list of a device call: by default what the device buffer `list` holds, or n_states for the identity list."""
    if n_list is None:
        n_list = n_states if list is None else _n_bytes(list) // 4
    if not _has_room(n_list, (list, 4)):
        raise ValueError("list must have room for n_list 4-byte indices")
    return n_list


class _Handle:
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            type(self)._destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene(_Handle):
    """scene.rs:23-35; immutable after creation."""
    _destroy = lib.rl_scene_destroy

    def __init__(self, objects, camera, device=0):
        super().__init__()
        self.objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        camera = RlCameraDesc.from_buffer_copy(bytes(camera))  # accept any 40-byte camera record
        desc = RlSceneDesc(len(self.objects), self.objects.ctypes.data_as(C.c_void_p), camera)
        check(lib.rl_scene_create(C.byref(desc), device, C.byref(self._h)))
        self.device = device

    @classmethod
    def builtin(cls, which=SCENE_DEMO, param=0, device=0):
        objs, cam = builtin_scene_desc(which, param)
        return cls(objs, cam, device)

    def intersect(self, origins, directions, t_max=np.inf, fetch=FETCH_LDS):
        """Scene::intersect (scene.rs:39-60) for n rays on the scene's device (rl_scene_intersect).  origins, directions: (n, 3)
        float32; t_max: a scalar or n values (only hits with distance < t_max count).  Returns an (n,) HIT_DTYPE array: object
        (RL_OBJECT_NONE on a miss), distance, position, normal, tangent."""
        origins = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        directions = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(origins) != len(directions):
            raise ValueError("origins and directions differ in length")
        rays = np.zeros(len(origins), dtype=RAY_DTYPE)
        rays["origin"] = origins
        rays["direction"] = directions
        rays["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (len(rays),))
        hits = np.empty(len(rays), dtype=HIT_DTYPE)
        check(lib.rl_scene_intersect(self._h, fetch, rays.ctypes.data_as(C.c_void_p), len(rays), hits.ctypes.data_as(C.c_void_p)))
        return hits

    def intersect_device(self, rays, hits, fetch=FETCH_LDS):
        """rl_scene_intersect_device: `rays` and `hits` are device buffers on the scene's device with data_ptr() (e.g. torch
        tensors) holding n RAY_DTYPE records and room for n HIT_DTYPE records; n is taken from the sizes in bytes."""
        n = _record_count(rays, RAY_DTYPE, "rays must hold whole 32-byte records and hits room for as many 48-byte ones",
                          (hits, HIT_DTYPE.itemsize))
        check(lib.rl_scene_intersect_device(self._h, fetch, C.c_void_p(rays.data_ptr()), n, C.c_void_p(hits.data_ptr())))

    def occluded(self, origins, directions, t_max=np.inf, fetch=FETCH_LDS):
        """rl_scene_occluded: is there a hit with distance < t_max on each of n rays -- would intersect() report an object?
        origins, directions: (n, 3) float32; t_max: a scalar or n values.  Returns an (n,) uint8 array of 1 (blocked) and 0."""
        origins = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        directions = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(origins) != len(directions):
            raise ValueError("origins and directions differ in length")
        rays = np.zeros(len(origins), dtype=RAY_DTYPE)
        rays["origin"] = origins
        rays["direction"] = directions
        rays["t_max"] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (len(rays),))
        out = np.empty(len(rays), dtype=np.uint8)
        check(lib.rl_scene_occluded(self._h, fetch, rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p)))
        return out

    def occluded_device(self, rays, occluded, fetch=FETCH_LDS):
        """rl_scene_occluded_device: `rays` and `occluded` are device buffers on the scene's device with data_ptr() (e.g. torch
        tensors) holding n RAY_DTYPE records and room for n bytes; n is taken from the rays' size in bytes."""
        n = _record_count(rays, RAY_DTYPE, "rays must hold whole 32-byte records and occluded room for as many bytes", (occluded, 1))
        check(lib.rl_scene_occluded_device(self._h, fetch, C.c_void_p(rays.data_ptr()), n, C.c_void_p(occluded.data_ptr())))

    def camera_rays(self, width, height, seed, stream, first, n):
        """rl_scene_camera_rays: the camera half of paths first .. first + n - 1 of (seed, stream) for a width x height image --
        the ray, its wavelength and the screen position x, y that rl_trace_unit_render gives those paths.  Returns an (n,)
        CAMERA_SAMPLE_DTYPE array."""
        samples = np.empty(n, dtype=CAMERA_SAMPLE_DTYPE)
        check(lib.rl_scene_camera_rays(self._h, width, height, seed, stream, first, n, samples.ctypes.data_as(C.c_void_p)))
        return samples

    def camera_rays_device(self, width, height, seed, stream, first, samples):
        """rl_scene_camera_rays_device: fills a device buffer with data_ptr() (e.g. a torch tensor) with as many
        CAMERA_SAMPLE_DTYPE records as it holds whole."""
        n = _n_bytes(samples) // CAMERA_SAMPLE_DTYPE.itemsize
        check(lib.rl_scene_camera_rays_device(self._h, width, height, seed, stream, first, n, C.c_void_p(samples.data_ptr())))

    def render_rays(self, origins, directions, wavelengths, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0):
        """TraceUnit::render_ray (trace_unit.rs:81-132) for n caller-supplied rays as paths first .. first + n - 1 of (seed,
        stream) (rl_scene_render_rays).  origins, directions: (n, 3) float32, directions used as given; wavelengths: a scalar or n
        values in nm.  Returns an (n,) PATH_RESULT_DTYPE array: value, segments, object (the emitter, or RL_OBJECT_NONE), end
        (RL_PATH_END_*).  max_segments 0 means RL_PATH_MAX_SEGMENTS."""
        origins = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        directions = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if len(origins) != len(directions):
            raise ValueError("origins and directions differ in length")
        rays = np.zeros(len(origins), dtype=SPECTRAL_RAY_DTYPE)
        rays["origin"] = origins
        rays["direction"] = directions
        rays["wavelength"] = np.broadcast_to(np.asarray(wavelengths, dtype=np.float32), (len(rays),))
        return self.render_spectral_rays(rays, seed, stream, first, fetch, max_segments)

    def render_spectral_rays(self, rays, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0):
        """render_rays for an (n,) SPECTRAL_RAY_DTYPE array (e.g. camera_rays(...)["ray"])."""
        rays = np.ascontiguousarray(rays, dtype=SPECTRAL_RAY_DTYPE)
        results = np.empty(len(rays), dtype=PATH_RESULT_DTYPE)
        check(lib.rl_scene_render_rays(self._h, fetch, seed, stream, first, max_segments, rays.ctypes.data_as(C.c_void_p), len(rays),
                                       results.ctypes.data_as(C.c_void_p)))
        return results

    def render_rays_device(self, rays, results, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0):
        """rl_scene_render_rays_device: `rays` and `results` are device buffers on the scene's device with data_ptr() (e.g. torch
        tensors) holding n SPECTRAL_RAY_DTYPE records and room for n PATH_RESULT_DTYPE records; n is taken from the sizes in bytes."""
        n = _record_count(rays, SPECTRAL_RAY_DTYPE, "rays must hold whole 32-byte records and results room for as many 16-byte ones",
                          (results, PATH_RESULT_DTYPE.itemsize))
        check(lib.rl_scene_render_rays_device(self._h, fetch, seed, stream, first, max_segments, C.c_void_p(rays.data_ptr()), n,
                                              C.c_void_p(results.data_ptr())))

    def begin_paths(self, rays, first=0):
        """rl_scene_begin_paths: an (n,) SPECTRAL_RAY_DTYPE array as the (n,) PATH_STATE_DTYPE states of paths first .. first + n - 1
        before their first segment (end RL_PATH_LIVE; RL_PATH_END_INVALID for a wavelength that is not finite)."""
        rays = np.ascontiguousarray(rays, dtype=SPECTRAL_RAY_DTYPE)
        states = np.empty(len(rays), dtype=PATH_STATE_DTYPE)
        check(lib.rl_scene_begin_paths(self._h, first, rays.ctypes.data_as(C.c_void_p), len(rays), states.ctypes.data_as(C.c_void_p)))
        return states

    def begin_paths_device(self, rays, states, first=0):
        """rl_scene_begin_paths_device: `rays` and `states` are device buffers on the scene's device with data_ptr() (e.g. torch
        tensors) holding n SPECTRAL_RAY_DTYPE records and room for n PATH_STATE_DTYPE records; n is taken from the sizes in bytes."""
        n = _record_count(rays, SPECTRAL_RAY_DTYPE, "rays must hold whole 32-byte records and states room for as many 64-byte ones",
                          (states, PATH_STATE_DTYPE.itemsize))
        check(lib.rl_scene_begin_paths_device(self._h, first, C.c_void_p(rays.data_ptr()), n, C.c_void_p(states.data_ptr())))

    def step_paths(self, states, seed, stream, fetch=FETCH_LDS, flags=0, hits=None):
        """rl_scene_step_paths: one segment for every live state of an (n,) PATH_STATE_DTYPE array, in place (the array must be
        contiguous).  hits: None, or an (n,) HIT_DTYPE array that receives the segment's hit of every stepped state.  flags: 0 or
        RL_STEP_NO_ROULETTE.  Returns `states`."""
        if states.dtype != PATH_STATE_DTYPE or not states.flags.c_contiguous or not states.flags.writeable:
            raise ValueError("states must be a contiguous, writeable PATH_STATE_DTYPE array")
        if hits is not None and (hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous or len(hits) < len(states)):
            raise ValueError("hits must be a contiguous HIT_DTYPE array with room for every state")
        check(lib.rl_scene_step_paths(self._h, fetch, seed, stream, flags, _host_ptr(states), len(states), _host_ptr(hits)))
        return states

    def step_paths_device(self, states, seed, stream, fetch=FETCH_LDS, flags=0, hits=None):
        """rl_scene_step_paths_device: `states` is a device buffer on the scene's device with data_ptr() (e.g. a torch tensor)
        holding n PATH_STATE_DTYPE records, stepped in place; `hits` None or a device buffer with room for n HIT_DTYPE records."""
        n = _record_count(states, PATH_STATE_DTYPE, "states must hold whole 64-byte records and hits room for as many 48-byte ones",
                          (hits, HIT_DTYPE.itemsize))
        check(lib.rl_scene_step_paths_device(self._h, fetch, seed, stream, flags, _device_ptr(states), n, _device_ptr(hits)))

    def step_path_list(self, states, seed, stream, list=None, n_list=None, fetch=FETCH_LDS, flags=0, hits=None):
        """rl_scene_step_path_list: one segment, in place, for the live states of an (n,) PATH_STATE_DTYPE array that `list` names
        (an array of indices, converted to uint32; entries >= n are skipped), or for states 0 .. n_list - 1 when list is None
        (n_list defaults to n).  hits: None, or an (n,) HIT_DTYPE array indexed by state.  Returns the indices of the listed states
        that are live after the step, in the list's order, as a uint32 array."""
        if states.dtype != PATH_STATE_DTYPE or not states.flags.c_contiguous or not states.flags.writeable:
            raise ValueError("states must be a contiguous, writeable PATH_STATE_DTYPE array")
        if hits is not None and (hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous or len(hits) < len(states)):
            raise ValueError("hits must be a contiguous HIT_DTYPE array with room for every state")
        list, n_list = _host_list(list, n_list, len(states))
        live = np.empty(n_list, dtype=np.uint32)
        n_live = C.c_uint32(0)
        check(lib.rl_scene_step_path_list(self._h, fetch, seed, stream, flags, _host_ptr(states), len(states), _host_ptr(list), n_list,
                                          _host_ptr(hits), _host_ptr(live), C.byref(n_live)))
        return live[:n_live.value].copy()

    def step_path_list_device(self, states, seed, stream, list, n_list, live_list, fetch=FETCH_LDS, flags=0, hits=None):
        """rl_scene_step_path_list_device: `states` is a device buffer on the scene's device with data_ptr() (e.g. a torch tensor)
        holding n PATH_STATE_DTYPE records; `list` None (states 0 .. n_list - 1) or a device buffer of at least n_list uint32
        indices; `live_list` None or a device buffer with room for n_list of them (it may be `list`); `hits` None or a device buffer
        with room for n HIT_DTYPE records.  Returns n_live."""
        n = _record_count(states, PATH_STATE_DTYPE, "states must hold whole 64-byte records and hits room for as many 48-byte ones",
                          (hits, HIT_DTYPE.itemsize))
        if not _has_room(n_list, (list, 4), (live_list, 4)):
            raise ValueError("list and live_list must have room for n_list 4-byte indices")
        n_live = C.c_uint32(0)
        check(lib.rl_scene_step_path_list_device(self._h, fetch, seed, stream, flags, _device_ptr(states), n, _device_ptr(list), n_list,
                                                 _device_ptr(hits), _device_ptr(live_list), C.byref(n_live)))
        return n_live.value

    def emitters(self):
        """rl_scene_emitters: the object indices of the scene's sampleable emitters (black-body spheres and circles), in scan
        order, as a uint32 array."""
        n = C.c_uint32(0)
        lib.rl_scene_emitters(self._h, None, 0, C.byref(n))
        out = np.zeros(n.value, dtype=np.uint32)
        check(lib.rl_scene_emitters(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def light_paths(self, states, hits, seed, stream, list=None, n_list=None, fetch=FETCH_LDS, samples=None):
        """rl_scene_light_paths: one direct-light sample for the states of an (n,) PATH_STATE_DTYPE array that `list` names (an
        array of indices, converted to uint32; entries >= n are skipped), or for states 0 .. n_list - 1 when list is None (n_list
        defaults to n).  hits: the (n,) HIT_DTYPE array the step wrote, indexed by state.  samples: None (a zeroed array is made),
        or an (n,) LIGHT_SAMPLE_DTYPE array whose records of the listed states are overwritten.  Returns `samples`."""
        if states.dtype != PATH_STATE_DTYPE or not states.flags.c_contiguous:
            raise ValueError("states must be a contiguous PATH_STATE_DTYPE array")
        if hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous or len(hits) < len(states):
            raise ValueError("hits must be a contiguous HIT_DTYPE array with room for every state")
        if samples is None:
            samples = np.zeros(len(states), dtype=LIGHT_SAMPLE_DTYPE)
        if samples.dtype != LIGHT_SAMPLE_DTYPE or not samples.flags.c_contiguous or not samples.flags.writeable or len(samples) < len(states):
            raise ValueError("samples must be a contiguous, writeable LIGHT_SAMPLE_DTYPE array with room for every state")
        list, n_list = _host_list(list, n_list, len(states))
        check(lib.rl_scene_light_paths(self._h, fetch, seed, stream, _host_ptr(states), len(states), _host_ptr(list), n_list, _host_ptr(hits),
                                       _host_ptr(samples)))
        return samples

    def light_paths_device(self, states, hits, samples, seed, stream, list=None, n_list=None, fetch=FETCH_LDS):
        """rl_scene_light_paths_device: `states`, `hits` and `samples` are device buffers on the scene's device with data_ptr()
        (e.g. torch tensors) holding n PATH_STATE_DTYPE records, n HIT_DTYPE records and room for n LIGHT_SAMPLE_DTYPE records;
        `list` None (states 0 .. n_list - 1, n_list defaults to n) or a device buffer of at least n_list uint32 indices."""
        n = _record_count(states, PATH_STATE_DTYPE,
                          "states must hold whole 64-byte records, hits room for as many 48-byte ones and samples for as many 32-byte ones",
                          (hits, HIT_DTYPE.itemsize), (samples, LIGHT_SAMPLE_DTYPE.itemsize))
        n_list = _device_list(list, n_list, n)
        check(lib.rl_scene_light_paths_device(self._h, fetch, seed, stream, _device_ptr(states), n, _device_ptr(list), n_list, _device_ptr(hits),
                                              _device_ptr(samples)))

    def render_features(self, width, height, seed, stream, first, n, max_segments=0, fetch=FETCH_LDS, albedo=None, normal=None, aux=None,
                        records=None):
        """rl_scene_render_features: the denoising guides of camera paths first .. first + n - 1 of `stream` under `seed` for a
        width x height image, in one launch.  `albedo`, `normal` and `aux` are None or three distinct PlotUnits of that size on
        the scene's device; each receives its film's splats on top of what it holds.  `records`, if given, is a device buffer on
        the scene's device with data_ptr() (e.g. a torch tensor) with room for n FEATURE_SAMPLE_DTYPE records.  Returns the call's
        RlFeatureStats as a dict of exact counts: paths, segments and kinds (a list indexed by FEATURE_VOID .. FEATURE_LIMIT)."""
        if records is not None and not _has_room(n, (records, FEATURE_SAMPLE_DTYPE.itemsize)):
            raise ValueError("records must have room for a 48-byte record for every path")
        stats = RlFeatureStats()
        check(lib.rl_scene_render_features(self._h, fetch, width, height, seed, stream, first, n, max_segments,
                                           *[u.handle if u is not None else None for u in (albedo, normal, aux)], _device_ptr(records),
                                           C.byref(stats)))
        return {"paths": int(stats.paths), "segments": int(stats.segments), "kinds": [int(k) for k in stats.kinds]}


WAVELENGTH_BINS = 256


def wavelength_importance_cie1931():
    """rl_wavelength_importance_cie1931: x-bar + y-bar + z-bar of the CIE 1931 observer at its 81 nodes, float64."""
    out = np.zeros(81, dtype=np.float64)
    check(lib.rl_wavelength_importance_cie1931(_host_ptr(out)))
    return out


def _wavelength_importance(importance):
    """An importance as the entry points take it: None, "cie", or values at equally spaced wavelengths from 380 to 780 nm."""
    if importance is None:
        return None
    if isinstance(importance, str):
        if importance != "cie":
            raise ValueError("a named wavelength importance must be 'cie'")
        return wavelength_importance_cie1931()
    return np.ascontiguousarray(importance, dtype=np.float64).reshape(-1)


class WavelengthTable(_Handle):
    """Wavelength importance sampling (rl_wavelength_table_*): 257 quantiles and 256 weights made of an importance over 380-780 nm.
    A TraceUnit draws its wavelengths from it after set_wavelengths; the table must outlive those renders."""
    _destroy = lib.rl_wavelength_table_destroy

    def __init__(self, importance="cie", uniform_share=0.1, n_nodes=None, device=0):
        """importance: "cie", values at n_nodes equally spaced wavelengths, or None (uniform; n_nodes then defaults to 2)."""
        super().__init__()
        g = _wavelength_importance(importance)
        if n_nodes is None:
            n_nodes = len(g) if g is not None else 2
        if g is not None and len(g) != n_nodes:
            raise ValueError("importance must hold n_nodes values")
        check(lib.rl_wavelength_table_create(device, _host_ptr(g), n_nodes, uniform_share, C.byref(self._h)))
        self.device = device

    def download(self):
        """(quantiles float32[257], weights float32[256]) read back from the device."""
        q, w = np.zeros(WAVELENGTH_BINS + 1, dtype=np.float32), np.zeros(WAVELENGTH_BINS, dtype=np.float32)
        check(lib.rl_wavelength_table_download(self._h, _host_ptr(q), _host_ptr(w)))
        return q, w


class TraceUnit(_Handle):
    """trace_unit.rs:51-168."""
    _destroy = lib.rl_trace_unit_destroy

    def __init__(self, id, width, height, n_photons=NUMBER_OF_PHOTONS, device=0):
        super().__init__()
        check(lib.rl_trace_unit_create(device, id, width, height, n_photons, C.byref(self._h)))
        self.id, self.width, self.height, self.n_photons, self.device = id, width, height, n_photons, device

    def set_fetch(self, fetch):
        check(lib.rl_trace_unit_set_fetch(self._h, fetch))

    def set_wavelengths(self, table):
        """rl_trace_unit_set_wavelengths: a WavelengthTable for subsequent renders, or None for the reference's uniform draw."""
        check(lib.rl_trace_unit_set_wavelengths(self._h, table.handle if table is not None else None))
        self._wavelengths = table  # (kept alive with the unit)

    def render(self, scene, seed=1, stream=0, first_path_index=0):
        check(lib.rl_trace_unit_render(self._h, scene.handle, seed, stream, first_path_index))

    def render_begin(self, scene, seed=1, stream=0, first_path_index=0):
        """First half of render(): the call is appended to the device's open launch; render_end() waits for it."""
        check(lib.rl_trace_unit_render_begin(self._h, scene.handle, seed, stream, first_path_index))

    def render_fused_begin(self, scene, plot_unit, n_paths, seed=1, stream=0, first_path_index=0):
        check(lib.rl_trace_unit_render_fused_begin(self._h, scene.handle, plot_unit.handle, seed, stream, first_path_index, n_paths))

    def render_end(self):
        check(lib.rl_trace_unit_render_end(self._h))

    def render_async(self, scene, seed=1, stream=0, first_path_index=0):
        check(lib.rl_trace_unit_render_async(self._h, scene.handle, seed, stream, first_path_index))

    def render_fused(self, scene, plot_unit, n_paths, seed=1, stream=0, first_path_index=0):
        check(lib.rl_trace_unit_render_fused(self._h, scene.handle, plot_unit.handle, seed, stream, first_path_index,
                                             n_paths))

    def render_fused_sync(self, scene, plot_unit, n_paths, seed=1, stream=0, first_path_index=0):
        """Blocking fused render; the calls of several threads share open launches (rl_trace_unit_render_fused_sync)."""
        check(lib.rl_trace_unit_render_fused_sync(self._h, scene.handle, plot_unit.handle, seed, stream, first_path_index, n_paths))

    def sync(self):
        check(lib.rl_trace_unit_sync(self._h))

    @property
    def mapped_photons(self):
        out = np.zeros(self.n_photons, dtype=PHOTON_DTYPE)
        check(lib.rl_trace_unit_photons(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stats(self):
        """(paths, segments, kernel_ms) accumulated since creation."""
        p, s, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        check(lib.rl_trace_unit_stats(self._h, C.byref(p), C.byref(s), C.byref(ms)))
        return p.value, s.value, ms.value


class PlotUnit(_Handle):
    """plot_unit.rs:23-102."""
    _destroy = lib.rl_plot_unit_destroy

    def __init__(self, id, width, height, device=0, external_xyz=None):
        super().__init__()
        check(lib.rl_plot_unit_create(device, id, width, height, C.c_void_p(external_xyz or 0), C.byref(self._h)))
        self.id, self.width, self.height, self.device = id, width, height, device

    def plot(self, trace_units):
        arr = (C.c_void_p * len(trace_units))(*[t.handle for t in trace_units])
        check(lib.rl_plot_unit_plot(self._h, arr, len(trace_units)))

    def clear(self):
        check(lib.rl_plot_unit_clear(self._h))

    def sync(self):
        check(lib.rl_plot_unit_sync(self._h))

    def reduce(self, comm, root=0):
        """The GatherUnit-time exchange: sum of every rank's buffer onto `root` (ncclReduce on the unit's stream)."""
        check(lib.rl_plot_unit_reduce(self._h, comm.handle, root))

    def exchange_stats(self):
        """(exchanges so far, device milliseconds they took): rl_plot_unit_exchange_stats."""
        n, ms = C.c_uint64(0), C.c_double(0.0)
        check(lib.rl_plot_unit_exchange_stats(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def add(self, other):
        """self += other (same device)."""
        check(lib.rl_plot_unit_add(self._h, other.handle))

    def device_buffer(self):
        p = C.c_void_p()
        check(lib.rl_plot_unit_device_buffer(self._h, C.byref(p)))
        return p.value

    @property
    def tristimulus_buffer(self):
        out = np.zeros((self.height * self.width, 3), dtype=np.float32)
        check(lib.rl_plot_unit_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def upload(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(self.height * self.width, 3)
        check(lib.rl_plot_unit_upload(self._h, xyz.ctypes.data_as(C.c_void_p)))

    def plot_photons(self, photons):
        """PlotUnit::plot(&[MappedPhoton]) (plot_unit.rs:87-95) for an (n,) PHOTON_DTYPE array of the caller's
        (rl_plot_unit_plot_photons): added onto the buffer, complete on return.  A photon whose x or y is not finite is skipped."""
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        check(lib.rl_plot_unit_plot_photons(self._h, photons.ctypes.data_as(C.c_void_p), len(photons)))

    def plot_photons_device(self, photons):
        """rl_plot_unit_plot_photons_device: `photons` is a device buffer on the unit's device with data_ptr() (e.g. a torch tensor);
        as many PHOTON_DTYPE records as it holds whole are plotted."""
        n = _n_bytes(photons) // PHOTON_DTYPE.itemsize
        check(lib.rl_plot_unit_plot_photons_device(self._h, C.c_void_p(photons.data_ptr()), n))

    def render_samples(self, scene, samples, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0, results=True):
        """Scene.render_rays with a film (rl_plot_unit_render_samples): samples[i]["ray"] of an (n,) CAMERA_SAMPLE_DTYPE array is
        traced as path first + i of (seed, stream) and a path that ends with a value is splatted at samples[i]["x"], ["y"] into
        this unit, complete on return.  Returns the (n,) PATH_RESULT_DTYPE array Scene.render_spectral_rays gives for the same
        rays, or None with results=False (then only the film is written)."""
        samples = np.ascontiguousarray(samples, dtype=CAMERA_SAMPLE_DTYPE)
        out = np.empty(len(samples), dtype=PATH_RESULT_DTYPE) if results else None
        check(lib.rl_plot_unit_render_samples(self._h, scene.handle, fetch, seed, stream, first, max_segments,
                                              samples.ctypes.data_as(C.c_void_p), len(samples),
                                              out.ctypes.data_as(C.c_void_p) if results else None))
        return out

    def render_samples_device(self, scene, samples, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0, results=None):
        """rl_plot_unit_render_samples_device: `samples` (and `results`, if given) are device buffers on the unit's device with
        data_ptr() (e.g. torch tensors) holding n CAMERA_SAMPLE_DTYPE records and room for n PATH_RESULT_DTYPE records; n is taken
        from the sizes in bytes."""
        n = _record_count(samples, CAMERA_SAMPLE_DTYPE, "samples must hold whole 48-byte records and results room for as many 16-byte ones",
                          (results, PATH_RESULT_DTYPE.itemsize))
        check(lib.rl_plot_unit_render_samples_device(self._h, scene.handle, fetch, seed, stream, first, max_segments, _device_ptr(samples), n,
                                                     _device_ptr(results)))

    def render_adaptive(self, adaptive, scene, seed, stream, first_path_index=0, fetch=FETCH_LDS, max_segments=0):
        """rl_plot_unit_render_adaptive: renders the whole plan of AdaptiveUnit `adaptive` as paths first_path_index .. of (seed,
        stream): its samples traced as Scene.render_rays_device traces them and splatted with their tiles' weights, complete on
        return.  The buffer then holds an unbiased estimate of what as many uniform paths would sum to."""
        check(lib.rl_plot_unit_render_adaptive(self._h, adaptive.handle, scene.handle, fetch, seed, stream, first_path_index, max_segments))

    def light_paths(self, scene, states, hits, camera, seed, stream, list=None, n_list=None, fetch=FETCH_LDS, sampled=None, samples=None):
        """Scene.light_paths with a film (rl_plot_unit_light_paths): the states of an (n,) PATH_STATE_DTYPE array that `list`
        names (or states 0 .. n_list - 1) are sampled as Scene.light_paths samples them, and a visible sample's value, or the
        value of a state that ended on a light that was not counted at the vertex before, is splatted at camera[i]["x"], ["y"] of
        an (n,) CAMERA_SAMPLE_DTYPE array, complete on return.  sampled: None (nothing is dropped or recorded) or an (n,) uint8
        array, read and rewritten in place for the listed states.  samples: None, or an (n,) LIGHT_SAMPLE_DTYPE array that receives
        the listed states' records.  Returns `samples`."""
        if states.dtype != PATH_STATE_DTYPE or not states.flags.c_contiguous:
            raise ValueError("states must be a contiguous PATH_STATE_DTYPE array")
        n = len(states)
        if hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous or len(hits) < n:
            raise ValueError("hits must be a contiguous HIT_DTYPE array with room for every state")
        if camera.dtype != CAMERA_SAMPLE_DTYPE or not camera.flags.c_contiguous or len(camera) < n:
            raise ValueError("camera must be a contiguous CAMERA_SAMPLE_DTYPE array with a record for every state")
        if sampled is not None and (sampled.dtype != np.uint8 or not sampled.flags.c_contiguous or not sampled.flags.writeable or len(sampled) < n):
            raise ValueError("sampled must be a contiguous, writeable uint8 array with a byte for every state")
        if samples is not None and (samples.dtype != LIGHT_SAMPLE_DTYPE or not samples.flags.c_contiguous or not samples.flags.writeable or len(samples) < n):
            raise ValueError("samples must be a contiguous, writeable LIGHT_SAMPLE_DTYPE array with room for every state")
        list, n_list = _host_list(list, n_list, n)
        check(lib.rl_plot_unit_light_paths(self._h, scene.handle, fetch, seed, stream, _host_ptr(states), n, _host_ptr(list), n_list, _host_ptr(hits),
                                           _host_ptr(camera), _host_ptr(sampled), _host_ptr(samples)))
        return samples

    def light_paths_device(self, scene, states, hits, camera, seed, stream, list=None, n_list=None, fetch=FETCH_LDS, sampled=None, samples=None):
        """rl_plot_unit_light_paths_device: `states`, `hits` and `camera` (and `sampled`, `samples`, `list`, if given) are device
        buffers on the unit's device with data_ptr() (e.g. torch tensors) holding n PATH_STATE_DTYPE, HIT_DTYPE and
        CAMERA_SAMPLE_DTYPE records, n bytes, room for n LIGHT_SAMPLE_DTYPE records and at least n_list uint32 indices."""
        n = _record_count(states, PATH_STATE_DTYPE,
                          "states must hold whole 64-byte records, hits room for as many 48-byte ones and camera as many 48-byte ones",
                          (hits, HIT_DTYPE.itemsize), (camera, CAMERA_SAMPLE_DTYPE.itemsize))
        if not _has_room(n, (sampled, 1), (samples, LIGHT_SAMPLE_DTYPE.itemsize)):
            raise ValueError("sampled must have a byte and samples room for a 32-byte record for every state")
        n_list = _device_list(list, n_list, n)
        check(lib.rl_plot_unit_light_paths_device(self._h, scene.handle, fetch, seed, stream, _device_ptr(states), n, _device_ptr(list), n_list,
                                                  _device_ptr(hits), _device_ptr(camera), _device_ptr(sampled), _device_ptr(samples)))

    def render_samples_direct(self, scene, samples, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0, results=True):
        """render_samples with direct light (rl_plot_unit_render_samples_direct): the same paths, and at every diffuse vertex one
        direct-light sample is splatted as well, each light counted once.  Returns what render_samples returns."""
        samples = np.ascontiguousarray(samples, dtype=CAMERA_SAMPLE_DTYPE)
        out = np.empty(len(samples), dtype=PATH_RESULT_DTYPE) if results else None
        check(lib.rl_plot_unit_render_samples_direct(self._h, scene.handle, fetch, seed, stream, first, max_segments,
                                                     samples.ctypes.data_as(C.c_void_p), len(samples),
                                                     out.ctypes.data_as(C.c_void_p) if results else None))
        return out

    def render_samples_direct_device(self, scene, samples, seed, stream, first=0, fetch=FETCH_LDS, max_segments=0, results=None):
        """rl_plot_unit_render_samples_direct_device: the buffers of render_samples_device."""
        n = _record_count(samples, CAMERA_SAMPLE_DTYPE, "samples must hold whole 48-byte records and results room for as many 16-byte ones",
                          (results, PATH_RESULT_DTYPE.itemsize))
        check(lib.rl_plot_unit_render_samples_direct_device(self._h, scene.handle, fetch, seed, stream, first, max_segments, _device_ptr(samples), n,
                                                            _device_ptr(results)))

    def render_direct(self, scene, seed, stream, first_path_index, n_paths, max_segments=0, fetch=FETCH_LDS, results=None):
        """Direct light over paths of the RNG in one launch (rl_plot_unit_render_direct): camera paths first_path_index ..
        first_path_index + n_paths - 1 of `stream` under `seed`, on this unit's image size, with render_samples_direct's film.
        `results`, if given, is a device buffer on the unit's device with data_ptr() (e.g. a torch tensor) with room for n_paths
        PATH_RESULT_DTYPE records.  Returns the call's RlDirectStats as a dict of exact counts."""
        if results is not None and not _has_room(n_paths, (results, PATH_RESULT_DTYPE.itemsize)):
            raise ValueError("results must have room for a 16-byte record for every path")
        stats = RlDirectStats()
        check(lib.rl_plot_unit_render_direct(self._h, scene.handle, fetch, seed, stream, first_path_index, n_paths, max_segments,
                                             _device_ptr(results), C.byref(stats)))
        return {name: int(getattr(stats, name)) for name, _ in RlDirectStats._fields_}


class GatherUnit(_Handle):
    """gather_unit.rs:24-92 (resume is explicit: load())."""
    _destroy = lib.rl_gather_unit_destroy

    def __init__(self, width, height, device=0):
        super().__init__()
        check(lib.rl_gather_unit_create(device, width, height, C.byref(self._h)))
        self.width, self.height, self.device = width, height, device

    def accumulate(self, plot_unit):
        """accumulate(&plot.tristimulus_buffer) then plot.clear() (app.rs:143-148)."""
        check(lib.rl_gather_unit_accumulate(self._h, plot_unit.handle))

    def allreduce(self, plot_unit, comm):
        """Task::Gather across ranks: reduce onto rank 0, which accumulates; the others clear (self may be None there)."""
        check(lib.rl_gather_unit_allreduce(self._h, plot_unit.handle, comm.handle))

    def sync(self):
        check(lib.rl_gather_unit_sync(self._h))

    def save(self, path="buffer.raw"):
        check(lib.rl_gather_unit_save(self._h, path.encode()))

    def load(self, path="buffer.raw"):
        check(lib.rl_gather_unit_load(self._h, path.encode()))

    def _download(self):
        t = np.zeros((self.height * self.width, 3), dtype=np.float32)
        c = np.zeros_like(t)
        check(lib.rl_gather_unit_download(self._h, t.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)))
        return t, c

    @property
    def tristimulus_buffer(self):
        return self._download()[0]

    @property
    def compensation_buffer(self):
        return self._download()[1]


def gather_allreduce(gather, plot_unit, comm):
    """rl_gather_unit_allreduce: Task::Gather across the ranks of `comm` (gather may be None on ranks other than 0)."""
    check(lib.rl_gather_unit_allreduce(gather.handle if gather is not None else None, plot_unit.handle, comm.handle))


class Comm(_Handle):
    """One rank of an RCCL communicator (rl_comm_*)."""
    _destroy = lib.rl_comm_destroy

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(lib.rl_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, world, rank, device=0):
        super().__init__()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib.rl_comm_init_rank(buf, world, rank, device, C.byref(self._h)))
        self.world, self.rank, self.device = world, rank, device

    def info(self):
        """{rank, world (as RCCL counts the communicator), rccl_version, library}: rl_comm_info."""
        rank, world, version = C.c_int(0), C.c_int(0), C.c_int(0)
        path = C.create_string_buffer(512)
        check(lib.rl_comm_info(self._h, C.byref(rank), C.byref(world), C.byref(version), path, 512))
        return {"rank": rank.value, "world": world.value, "rccl_version": version.value, "library": path.value.decode()}

    @classmethod
    def init_all(cls, devices):
        """One process, one rank per distinct device."""
        arr = (C.c_int * len(devices))(*devices)
        out = (C.c_void_p * len(devices))()
        check(lib.rl_comm_init_all(arr, len(devices), out))
        comms = []
        for i, d in enumerate(devices):
            c = cls.__new__(cls)
            _Handle.__init__(c)
            c._h = C.c_void_p(out[i])
            c.world, c.rank, c.device = len(devices), i, d
            comms.append(c)
        return comms


class TonemapUnit(_Handle):
    """tonemap_unit.rs:21-100."""
    _destroy = lib.rl_tonemap_unit_destroy

    def __init__(self, width, height, device=0):
        super().__init__()
        check(lib.rl_tonemap_unit_create(device, width, height, C.byref(self._h)))
        self.width, self.height, self.device = width, height, device

    def tonemap(self, gather_unit):
        check(lib.rl_tonemap_unit_tonemap(self._h, gather_unit.handle))

    @property
    def rgb_buffer(self):
        out = np.zeros((self.height * self.width, 3), dtype=np.uint8)
        check(lib.rl_tonemap_unit_rgb(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def srgb_float(self):
        """(clamped float sRGB before quantisation, max_intensity of find_exposure)."""
        out = np.zeros((self.height * self.width, 3), dtype=np.float32)
        mx = C.c_float(0)
        check(lib.rl_tonemap_unit_srgb_float(self._h, out.ctypes.data_as(C.c_void_p), C.byref(mx)))
        return out, mx.value


def denoise_params_default():
    """rl_denoise_params_default as a dict: iterations and the four sigmas (the keywords DenoiseUnit.denoise takes)."""
    p = RlDenoiseParams()
    check(lib.rl_denoise_params_default(C.byref(p)))
    return {"iterations": p.iterations, "sigma_colour": p.sigma_colour, "sigma_normal": p.sigma_normal, "sigma_depth": p.sigma_depth,
            "sigma_albedo": p.sigma_albedo}


def denoise_variance_params_default():
    """rl_denoise_variance_params_default as a dict (the keywords DenoiseUnit.denoise_variance takes)."""
    p = RlDenoiseParams()
    check(lib.rl_denoise_variance_params_default(C.byref(p)))
    return {"iterations": p.iterations, "sigma_colour": p.sigma_colour, "sigma_normal": p.sigma_normal, "sigma_depth": p.sigma_depth,
            "sigma_albedo": p.sigma_albedo}


class DenoiseUnit(_Handle):
    """The edge-avoiding a-trous filter over the guides of Scene.render_features (rl_denoise_unit_*)."""
    _destroy = lib.rl_denoise_unit_destroy

    def __init__(self, width, height, device=0):
        super().__init__()
        check(lib.rl_denoise_unit_create(device, width, height, C.byref(self._h)))
        self.width, self.height, self.device = width, height, device

    def denoise(self, image, albedo=None, normal=None, aux=None, *, dst, **params):
        """rl_denoise_unit_denoise: gather unit `image` filtered into gather unit `dst`, guided by the gather units that accumulated
        the films of Scene.render_features (each may be None); complete on return.  params: iterations, sigma_colour, sigma_normal,
        sigma_depth, sigma_albedo over denoise_params_default(); none given = the library's defaults.  Returns dst."""
        p = None
        if params:
            p = RlDenoiseParams()
            check(lib.rl_denoise_params_default(C.byref(p)))
            for name, value in params.items():
                if name not in ("iterations", "sigma_colour", "sigma_normal", "sigma_depth", "sigma_albedo"):
                    raise TypeError("denoise() got an unexpected keyword argument %r" % name)
                setattr(p, name, value)
        check(lib.rl_denoise_unit_denoise(self._h, image.handle, *[g.handle if g is not None else None for g in (albedo, normal, aux)],
                                          C.byref(p) if p is not None else None, dst.handle))
        return dst

    def denoise_variance(self, image, error, albedo=None, normal=None, aux=None, dst=None, variance=False, **params):
        """rl_denoise_unit_denoise_variance: denoise() with the variance of ErrorUnit `error` (at least two observations, of the
        plot buffers `image` gathered) as the colour term; sigma_colour is in standard deviations.  params are over
        denoise_variance_params_default().  Returns dst, or (dst, V as (height, width) float32: the variance of the denoised
        luminance) when `variance` is set."""
        if dst is None:
            raise TypeError("denoise_variance() needs dst, a gather unit")
        p = None
        if params:
            p = RlDenoiseParams()
            check(lib.rl_denoise_variance_params_default(C.byref(p)))
            for name, value in params.items():
                if name not in ("iterations", "sigma_colour", "sigma_normal", "sigma_depth", "sigma_albedo"):
                    raise TypeError("denoise_variance() got an unexpected keyword argument %r" % name)
                setattr(p, name, value)
        v = np.zeros((self.height, self.width), dtype=np.float32) if variance else None
        check(lib.rl_denoise_unit_denoise_variance(self._h, image.handle, *[g.handle if g is not None else None for g in (albedo, normal, aux)],
                                                   error.handle, C.byref(p) if p is not None else None, dst.handle,
                                                   v.ctypes.data_as(C.c_void_p) if variance else None))
        return (dst, v) if variance else dst

    def pass_ms(self):
        """Device milliseconds of the last denoise() or denoise_variance(): [the guide launch, pass 0, pass 1, ...]
        (rl_debug_denoise_pass_ms)."""
        out = (C.c_float * (1 + RL_DENOISE_MAX_ITERATIONS))()
        check(lib.rl_debug_denoise_pass_ms(self._h, out))
        return list(out)

    def variance_ms(self):
        """Device milliseconds of the V_0 launch of the last denoise_variance() (rl_debug_denoise_variance_ms)."""
        ms = C.c_float(0)
        check(lib.rl_debug_denoise_variance_ms(self._h, C.byref(ms)))
        return ms.value


def spectral_observer_cie1931(n_nodes=81):
    """rl_spectral_observer_cie1931: the (n_nodes, 3) float32 matrix whose row b is the library's CIE 1931 tristimulus of node b's
    wavelength, 380 + b * 400 / (n_nodes - 1) nm -- at 81 nodes the table itself.  Host arithmetic: needs no device."""
    out = np.zeros((max(int(n_nodes), 0), 3), dtype=np.float32)
    check(lib.rl_spectral_observer_cie1931(n_nodes, out.ctypes.data_as(C.c_void_p)))
    return out


class SpectralUnit(_Handle):
    """A film that keeps photons by wavelength: n_nodes planes of width x height floats (rl_spectral_unit_*), projected into a
    gather unit under any (n_nodes, 3) matrix."""
    _destroy = lib.rl_spectral_unit_destroy

    def __init__(self, width, height, n_nodes=81, device=0):
        super().__init__()
        check(lib.rl_spectral_unit_create(device, width, height, n_nodes, C.byref(self._h)))
        self.width, self.height, self.n_nodes, self.device = width, height, n_nodes, device

    def plot(self, trace_units):
        """rl_spectral_unit_plot: the photons of each trace unit's last un-fused render, in the film on return."""
        arr = (C.c_void_p * len(trace_units))(*[t.handle for t in trace_units])
        check(lib.rl_spectral_unit_plot(self._h, arr, len(trace_units)))

    def plot_photons(self, photons):
        """An (n,) PHOTON_DTYPE array of the caller's (rl_spectral_unit_plot_photons), or a device buffer on the unit's device with
        data_ptr() (e.g. a torch tensor; rl_spectral_unit_plot_photons_device: as many records as it holds whole): added onto the
        film, complete on return.  A photon whose x, y or wavelength is not finite is skipped."""
        if hasattr(photons, "data_ptr"):
            n = _n_bytes(photons) // PHOTON_DTYPE.itemsize
            check(lib.rl_spectral_unit_plot_photons_device(self._h, C.c_void_p(photons.data_ptr()), n))
            return
        photons = np.ascontiguousarray(photons, dtype=PHOTON_DTYPE)
        check(lib.rl_spectral_unit_plot_photons(self._h, photons.ctypes.data_as(C.c_void_p), len(photons)))

    def clear(self):
        check(lib.rl_spectral_unit_clear(self._h))

    def download(self):
        """The film: (n_nodes, height, width) float32."""
        out = np.zeros((self.n_nodes, self.height, self.width), dtype=np.float32)
        check(lib.rl_spectral_unit_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def upload(self, film):
        film = np.ascontiguousarray(film, dtype=np.float32).reshape(self.n_nodes, self.height, self.width)
        check(lib.rl_spectral_unit_upload(self._h, film.ctypes.data_as(C.c_void_p)))

    def project(self, matrix, dst):
        """rl_spectral_unit_project: gather unit `dst` = the film under the (n_nodes, 3) `matrix`, complete on return; its
        compensation buffer is zeroed, the film is left as it was.  Returns dst."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float32).reshape(self.n_nodes, 3)
        check(lib.rl_spectral_unit_project(self._h, matrix.ctypes.data_as(C.c_void_p), dst.handle))
        return dst

    def launch_ms(self):
        """Device milliseconds of (the last splat launch, the last projection launch) of this unit (rl_debug_spectral_ms)."""
        out = (C.c_float * 2)()
        check(lib.rl_debug_spectral_ms(self._h, out))
        return tuple(out)


def glare_psf_veil(taps, r0):
    """rl_glare_psf_veil: the (taps, taps) float32 veiling-glare point-spread function 1 / (q * sqrt(q)), q = 1 + d^2 / r0^2, d the
    distance from the centre in pixels; not normalised.  Host arithmetic: needs no device."""
    out = np.zeros((max(int(taps), 0), max(int(taps), 0)), dtype=np.float32)
    check(lib.rl_glare_psf_veil(taps, float(r0), out.ctypes.data_as(C.c_void_p)))
    return out


def glare_kernels_scaled(psf, lambda0, n_nodes, strength, taps):
    """rl_glare_kernels_scaled: the (n_nodes, taps, taps) float32 gather tables of GlareUnit.set_kernels from one square base
    point-spread function `psf` (odd side, sampled at pixel pitch for wavelength lambda0 nm): node b's is the function scaled by
    lambda_b / lambda0, point-flipped, normalised to sum 1 and mixed with a delta, strength * table + (1 - strength) at the centre.
    Host arithmetic: needs no device."""
    psf = np.ascontiguousarray(psf, dtype=np.float32)
    if psf.ndim != 2 or psf.shape[0] != psf.shape[1]:
        raise ValueError("glare_kernels_scaled: psf must be a square 2-d array, not %r" % (psf.shape,))
    out = np.zeros((max(int(n_nodes), 0), max(int(taps), 0), max(int(taps), 0)), dtype=np.float32)
    check(lib.rl_glare_kernels_scaled(psf.ctypes.data_as(C.c_void_p), psf.shape[0], float(lambda0), n_nodes, float(strength), taps,
                                      out.ctypes.data_as(C.c_void_p)))
    return out


class GlareUnit(_Handle):
    """One (taps, taps) gather table per spectral node, applied to a spectral unit's film and projected into a gather unit in one
    launch (rl_glare_unit_*): bloom, veiling glare, an aperture's diffraction pattern, each growing with wavelength."""
    _destroy = lib.rl_glare_unit_destroy

    def __init__(self, width, height, n_nodes, taps, device=0):
        super().__init__()
        check(lib.rl_glare_unit_create(device, width, height, n_nodes, taps, C.byref(self._h)))
        self.width, self.height, self.n_nodes, self.taps, self.device = width, height, n_nodes, taps, device

    def set_kernels(self, tables):
        """rl_glare_unit_set_kernels: (n_nodes, taps, taps) float32, entry [b, j, i] weighs node b of the film at (x + i - R,
        y + j - R); on the device on return.  May be set again."""
        tables = np.ascontiguousarray(tables, dtype=np.float32).reshape(self.n_nodes, self.taps, self.taps)
        check(lib.rl_glare_unit_set_kernels(self._h, tables.ctypes.data_as(C.c_void_p)))

    def apply(self, film, matrix, gather):
        """rl_glare_unit_apply: gather unit `gather` = spectral unit `film` convolved plane by plane with the tables and projected
        under the (n_nodes, 3) `matrix`, complete on return; its compensation buffer is zeroed, the film is left as it was.
        Returns gather."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float32).reshape(self.n_nodes, 3)
        check(lib.rl_glare_unit_apply(self._h, film.handle, matrix.ctypes.data_as(C.c_void_p), gather.handle))
        return gather

    def launch_ms(self):
        """Device milliseconds of the last apply's launch (rl_debug_glare_ms)."""
        ms = C.c_float(0)
        check(lib.rl_debug_glare_ms(self._h, C.byref(ms)))
        return ms.value


MATERIAL_BLACK_BODY = 0  # RL_MATERIAL_BLACK_BODY: kelvins = m[0], intensity = m[1]


def relight_gains_black_body(n_nodes, kelvins_from, intensity_from, kelvins_to, intensity_to):
    """rl_relight_gains_black_body: (n_nodes,) float32, what a finished path that ended on a black body of (kelvins_from,
    intensity_from) is multiplied by when that light becomes (kelvins_to, intensity_to), at each node's wavelength.  Host
    arithmetic: needs no device."""
    out = np.zeros(max(int(n_nodes), 0), dtype=np.float32)
    check(lib.rl_relight_gains_black_body(n_nodes, kelvins_from, intensity_from, kelvins_to, intensity_to, out.ctypes.data_as(C.c_void_p)))
    return out


def relight_groups(objects, n_groups):
    """The table RelightUnit.set_groups takes for an OBJECT_DTYPE array: black bodies get groups 0, 1, ... in scan order, those
    beyond n_groups - 1 share the last group; every other object gets RL_RELIGHT_DROP.  (objects,) uint8."""
    if not 1 <= n_groups <= RL_RELIGHT_MAX_GROUPS:
        raise ValueError("n_groups must be 1 .. RL_RELIGHT_MAX_GROUPS = %d" % RL_RELIGHT_MAX_GROUPS)
    lights = np.asarray(objects)["material_kind"] == MATERIAL_BLACK_BODY
    table = np.full(len(lights), RL_RELIGHT_DROP, dtype=np.uint8)
    table[lights] = np.minimum(np.arange(int(lights.sum())), n_groups - 1)
    return table


class RelightUnit(_Handle):
    """A film that keeps photons by wavelength and by light: n_groups cubes of n_nodes planes of width x height floats
    (rl_relight_unit_*), filled by a routed splat of traced camera samples and mixed into a gather unit under per-(group, node)
    gains and any (n_nodes, 3) observer, without a re-trace."""
    _destroy = lib.rl_relight_unit_destroy

    def __init__(self, width, height, n_nodes=81, n_groups=1, device=0):
        super().__init__()
        check(lib.rl_relight_unit_create(device, width, height, n_nodes, n_groups, C.byref(self._h)))
        self.width, self.height, self.n_nodes, self.n_groups, self.device = width, height, n_nodes, n_groups, device

    def set_groups(self, groups):
        """rl_relight_unit_set_groups: one byte per object of the scene's description, a group below n_groups or RL_RELIGHT_DROP
        (relight_groups makes one)."""
        groups = np.ascontiguousarray(groups, dtype=np.uint8)
        check(lib.rl_relight_unit_set_groups(self._h, groups.ctypes.data_as(C.c_void_p), len(groups)))

    def plot_results(self, samples, results):
        """(n,) CAMERA_SAMPLE_DTYPE and (n,) PATH_RESULT_DTYPE arrays of the caller's (rl_relight_unit_plot_results), or two device
        buffers on the unit's device with data_ptr() (e.g. torch tensors; rl_relight_unit_plot_results_device: as many records as
        `samples` holds whole, `results` with room for as many): each path's value goes into the cube of the light it ended on,
        complete on return."""
        if hasattr(samples, "data_ptr"):
            n = _record_count(samples, CAMERA_SAMPLE_DTYPE, "samples must hold whole 48-byte records and results as many 16-byte ones",
                              (results, PATH_RESULT_DTYPE.itemsize))
            check(lib.rl_relight_unit_plot_results_device(self._h, C.c_void_p(samples.data_ptr()), C.c_void_p(results.data_ptr()), n))
            return
        samples = np.ascontiguousarray(samples, dtype=CAMERA_SAMPLE_DTYPE)
        results = np.ascontiguousarray(results, dtype=PATH_RESULT_DTYPE)
        if len(samples) != len(results):
            raise ValueError("samples and results differ in length")
        check(lib.rl_relight_unit_plot_results(self._h, samples.ctypes.data_as(C.c_void_p), results.ctypes.data_as(C.c_void_p), len(samples)))

    def render(self, scene, seed, stream, first, n_paths, fetch=FETCH_LDS, max_segments=0):
        """rl_relight_unit_render: paths first .. first + n_paths - 1 of (seed, stream) -- camera samples, the path kernel, the
        routed splat -- in the film on return."""
        check(lib.rl_relight_unit_render(self._h, scene.handle, fetch, seed, stream, first, n_paths, max_segments))

    def clear(self):
        check(lib.rl_relight_unit_clear(self._h))

    def download(self):
        """The film: (n_groups, n_nodes, height, width) float32."""
        out = np.zeros((self.n_groups, self.n_nodes, self.height, self.width), dtype=np.float32)
        check(lib.rl_relight_unit_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def upload(self, film):
        film = np.ascontiguousarray(film, dtype=np.float32).reshape(self.n_groups, self.n_nodes, self.height, self.width)
        check(lib.rl_relight_unit_upload(self._h, film.ctypes.data_as(C.c_void_p)))

    def mix(self, gains, matrix, dst):
        """rl_relight_unit_mix: gather unit `dst` = the cubes under the (n_groups, n_nodes) `gains` (None: all 1) and the
        (n_nodes, 3) `matrix`, complete on return; its compensation buffer is zeroed, the film is left as it was.  Returns dst."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float32).reshape(self.n_nodes, 3)
        if gains is not None:
            gains = np.ascontiguousarray(gains, dtype=np.float32).reshape(self.n_groups, self.n_nodes)
        check(lib.rl_relight_unit_mix(self._h, _host_ptr(gains), matrix.ctypes.data_as(C.c_void_p), dst.handle))
        return dst

    def launch_ms(self):
        """Device milliseconds of (the last splat launch, the last render's last path launch, the last mix launch) of this unit
        (rl_debug_relight_ms)."""
        out = (C.c_float * 3)()
        check(lib.rl_debug_relight_ms(self._h, out))
        return tuple(out)


def _error_stats(stats):
    return {name: getattr(stats, name) for name, _ in RlErrorStats._fields_}


class ErrorUnit(_Handle):
    """The noise estimate (rl_error_unit_*): f64 sums S of y and Q of y^2 / n over the plot buffers shown to the unit just before
    they are gathered, and from them the standard error of the accumulated luminance per pixel and per 16 x 16 tile."""
    _destroy = lib.rl_error_unit_destroy

    def __init__(self, width, height, device=0):
        super().__init__()
        check(lib.rl_error_unit_create(device, width, height, C.byref(self._h)))
        self.width, self.height, self.device = width, height, device
        self.tiles_x, self.tiles_y = -(-width // RL_ERROR_TILE), -(-height // RL_ERROR_TILE)

    def clear(self):
        check(lib.rl_error_unit_clear(self._h))

    def observe(self, plot_unit, n_paths):
        """rl_error_unit_observe: the plot unit's buffer, the sum over n_paths independent paths, is one observation.  The buffer is
        left as it was: gather it afterwards.  Does not wait on the host."""
        check(lib.rl_error_unit_observe(self._h, plot_unit.handle, n_paths))

    def estimate(self, se=True, tiles=True):
        """rl_error_unit_estimate: (stats dict, se as (height, width) float32 or None, tiles as (tiles_y, tiles_x, 2) float64
        {t_se, t_y} or None).  Needs two observations."""
        stats = RlErrorStats()
        se_out = np.zeros((self.height, self.width), dtype=np.float32) if se else None
        tiles_out = np.zeros((self.tiles_y, self.tiles_x, 2), dtype=np.float64) if tiles else None
        check(lib.rl_error_unit_estimate(self._h, C.byref(stats), se_out.ctypes.data_as(C.c_void_p) if se else None,
                                         tiles_out.ctypes.data_as(C.c_void_p) if tiles else None))
        return _error_stats(stats), se_out, tiles_out

    def download(self):
        """(S, Q) as (height, width) float64 arrays, k, N."""
        s, q = np.zeros((self.height, self.width), dtype=np.float64), np.zeros((self.height, self.width), dtype=np.float64)
        k, n = C.c_uint64(0), C.c_uint64(0)
        check(lib.rl_error_unit_download(self._h, s.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), C.byref(k), C.byref(n)))
        return s, q, k.value, n.value

    def upload(self, sum_y, sum_q, observations, paths):
        s = np.ascontiguousarray(sum_y, dtype=np.float64).reshape(self.height, self.width)
        q = np.ascontiguousarray(sum_q, dtype=np.float64).reshape(self.height, self.width)
        check(lib.rl_error_unit_upload(self._h, s.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), observations, paths))

    def launch_ms(self):
        """Device milliseconds of (the last observe launch, the last estimate launch) of this unit (rl_debug_error_ms)."""
        out = (C.c_float * 2)()
        check(lib.rl_debug_error_ms(self._h, out))
        return tuple(out)


def error_tile_rel(tiles):
    """The per-tile relative error of rl_error_unit_estimate's host statistics, from (tiles_y, tiles_x, 2) {t_se, t_y} pairs:
    t_se / max(t_y, mean t_y), the sums sequential in f64 in tile raster order."""
    pairs = np.asarray(tiles, dtype=np.float64).reshape(-1, 2)
    sum_y = np.float64(0)
    for t_y in pairs[:, 1]:
        sum_y = sum_y + t_y
    m = sum_y / np.float64(len(pairs))
    with np.errstate(all="ignore"):
        return (pairs[:, 0] / np.where(pairs[:, 1] > m, pairs[:, 1], m)).reshape(np.asarray(tiles).shape[:-1])


class RobustUnit(_Handle):
    """The robust film (rl_robust_unit_*): n_buckets sub-films of f64 XYZ sums over the plot buffers shown to the unit just before
    they are gathered, combined per pixel by a median of means whose trim follows the Gini coefficient of the bucket means."""
    _destroy = lib.rl_robust_unit_destroy

    def __init__(self, width, height, n_buckets=15, device=0):
        super().__init__()
        check(lib.rl_robust_unit_create(device, width, height, n_buckets, C.byref(self._h)))
        self.width, self.height, self.n_buckets, self.device = width, height, n_buckets, device

    def clear(self):
        check(lib.rl_robust_unit_clear(self._h))

    def observe(self, plot_unit, n_paths, bucket=None):
        """rl_robust_unit_observe: the plot unit's buffer, the sum over n_paths paths no other bucket has seen, is added to `bucket`
        (None: RL_ROBUST_NEXT, the buckets in turn).  The buffer is left as it was: gather it afterwards.  Does not wait on the host."""
        check(lib.rl_robust_unit_observe(self._h, plot_unit.handle, n_paths, RL_ROBUST_NEXT if bucket is None else bucket))

    def resolve(self, dst, gain=1.0, max_trim=0xFFFFFFFF, trim=False):
        """rl_robust_unit_resolve into the gather unit `dst`: the stats as a dict, or (stats, trim as (height, width) uint8) with
        trim=True."""
        params, stats = RlRobustParams(gain, max_trim, 0), RlRobustStats()
        trim_out = np.zeros((self.height, self.width), dtype=np.uint8) if trim else None
        check(lib.rl_robust_unit_resolve(self._h, C.byref(params), dst.handle, C.byref(stats), _host_ptr(trim_out)))
        out = {name: getattr(stats, name) for name, _ in RlRobustStats._fields_}
        return (out, trim_out) if trim else out

    def estimate(self, gain=1.0, max_trim=0xFFFFFFFF, se=True, trim=False):
        """rl_robust_unit_estimate, the standard error of the film that resolve() writes with the same gain and max_trim, in
        ErrorUnit.estimate's shapes: (stats dict, se as (height, width) float32 or None, tiles as (tiles_y, tiles_x, 2) float64
        {t_se, t_y}), and with trim=True a fourth element, (height, width) uint8: c, bit 7 set for an untrimmable pixel."""
        params, stats = RlRobustParams(gain, max_trim, 0), RlErrorStats()
        se_out = np.zeros((self.height, self.width), dtype=np.float32) if se else None
        tiles_out = np.zeros((-(-self.height // RL_ERROR_TILE), -(-self.width // RL_ERROR_TILE), 2), dtype=np.float64)
        trim_out = np.zeros((self.height, self.width), dtype=np.uint8) if trim else None
        check(lib.rl_robust_unit_estimate(self._h, C.byref(params), C.byref(stats), _host_ptr(se_out), _host_ptr(tiles_out), _host_ptr(trim_out)))
        out = (_error_stats(stats), se_out, tiles_out)
        return out + (trim_out,) if trim else out

    def estimate_ms(self):
        """Device milliseconds of the last estimate launch of this unit (rl_debug_robust_estimate_ms)."""
        out = C.c_float(0)
        check(lib.rl_debug_robust_estimate_ms(self._h, C.byref(out)))
        return out.value

    def download(self):
        """(sums as (n_buckets, 3, height, width) float64, bucket_paths as (n_buckets,) uint64, k)."""
        sums = np.zeros((self.n_buckets, 3, self.height, self.width), dtype=np.float64)
        paths, k = np.zeros(self.n_buckets, dtype=np.uint64), C.c_uint64(0)
        check(lib.rl_robust_unit_download(self._h, _host_ptr(sums), _host_ptr(paths), C.byref(k)))
        return sums, paths, k.value

    def upload(self, sums, bucket_paths, observations):
        s = np.ascontiguousarray(sums, dtype=np.float64).reshape(self.n_buckets, 3, self.height, self.width)
        n = np.ascontiguousarray(bucket_paths, dtype=np.uint64).reshape(self.n_buckets)
        check(lib.rl_robust_unit_upload(self._h, _host_ptr(s), _host_ptr(n), observations))

    def launch_ms(self):
        """Device milliseconds of (the last observe launch, the last resolve launch) of this unit (rl_debug_robust_ms)."""
        out = (C.c_float * 2)()
        check(lib.rl_debug_robust_ms(self._h, out))
        return tuple(out)


class AdaptiveUnit(_Handle):
    """Adaptive sampling (rl_adaptive_unit_*): a plan of how many of a batch's camera paths start in each 16 x 16 tile of the film
    and the weight their splats carry, so that the film's expectation is the uniform sampler's."""
    _destroy = lib.rl_adaptive_unit_destroy

    def __init__(self, width, height, device=0):
        super().__init__()
        check(lib.rl_adaptive_unit_create(device, width, height, C.byref(self._h)))
        self.width, self.height, self.device = width, height, device
        self.tiles_x, self.tiles_y = -(-width // RL_ERROR_TILE), -(-height // RL_ERROR_TILE)

    def plan(self, importance, uniform_share, n_paths):
        """rl_adaptive_unit_plan: importance is None (the uniform plan) or tiles_y * tiles_x values in raster order.  Returns the
        plan's stats as a dict.  A plan that would leave a tile without a sample raises RlError and the previous plan stays."""
        g = None
        if importance is not None:
            g = np.ascontiguousarray(importance, dtype=np.float64).reshape(-1)
            if len(g) != self.tiles_x * self.tiles_y:
                raise ValueError("importance must hold tiles_y * tiles_x values")
        stats = RlAdaptiveStats()
        check(lib.rl_adaptive_unit_plan(self._h, _host_ptr(g), uniform_share, n_paths, C.byref(stats)))
        return {name: getattr(stats, name) for name, _ in RlAdaptiveStats._fields_}

    def plan_from_error_tiles(self, tiles, uniform_share, n_paths):
        """plan() with a tile's t_se as its importance: `tiles` is rl_error_unit_estimate's (tiles_y, tiles_x, 2) {t_se, t_y} array."""
        return self.plan(np.asarray(tiles, dtype=np.float64).reshape(self.tiles_y, self.tiles_x, 2)[:, :, 0], uniform_share, n_paths)

    def download_plan(self):
        """(counts uint32, weights float32), each (tiles_y, tiles_x), read back from the device."""
        counts = np.zeros((self.tiles_y, self.tiles_x), dtype=np.uint32)
        weights = np.zeros((self.tiles_y, self.tiles_x), dtype=np.float32)
        check(lib.rl_adaptive_unit_download_plan(self._h, _host_ptr(counts), _host_ptr(weights)))
        return counts, weights

    def samples(self, scene, seed, stream, first_path_index, first_sample, n):
        """rl_adaptive_unit_samples: samples first_sample .. first_sample + n - 1 of the plan as an (n,) CAMERA_SAMPLE_DTYPE array;
        reserved0 is the sample's tile, reserved1 the bits of its weight."""
        out = np.empty(n, dtype=CAMERA_SAMPLE_DTYPE)
        check(lib.rl_adaptive_unit_samples(self._h, scene.handle, seed, stream, first_path_index, first_sample, n, _host_ptr(out)))
        return out

    def samples_device(self, scene, seed, stream, first_path_index, first_sample, samples, n=None):
        """rl_adaptive_unit_samples_device: fills a device buffer with data_ptr() (e.g. a torch tensor) with n records, by default
        as many as it holds whole."""
        room = _n_bytes(samples) // CAMERA_SAMPLE_DTYPE.itemsize
        n = room if n is None else n
        if n > room:
            raise ValueError("samples must have room for n 48-byte records")
        check(lib.rl_adaptive_unit_samples_device(self._h, scene.handle, seed, stream, first_path_index, first_sample, n, _device_ptr(samples)))

    def launch_ms(self):
        """Device milliseconds of the (sample, path, splat) launches of the last chunk of this unit's last render (rl_debug_adaptive_ms)."""
        out = (C.c_float * 3)()
        check(lib.rl_debug_adaptive_ms(self._h, out))
        return tuple(out)


def render_adaptive_to_error(scene, plot, gather, error, adaptive, n_paths_per_batch, max_batches, target_error, uniform_share=0.25,
                             min_observations=4, seed=1, stream=0, first_path_index=0, fetch=FETCH_LDS, max_segments=0, adaptive_sampling=True):
    """Renders batches of n_paths_per_batch paths into `plot`, shows each to `error` and accumulates it into `gather` (the plot unit is
    cleared by the accumulation), until rl_error_unit_estimate's relative_error is at most target_error or max_batches are made.  The plans
    are uniform until the error unit has min_observations (at least 2); from then on every batch is planned from the running tile
    map (a tile's t_se), with uniform_share of the paths spread by area.  adaptive_sampling=False keeps the uniform plan throughout:
    the same driver as the yardstick.  `error` must be empty (ErrorUnit.clear): the driver counts its own batches as the unit's
    observations.  Returns (batches made, the last estimate's stats or None, its tiles or None)."""
    if max(2, min_observations) > max_batches:
        raise ValueError("max_batches leaves no room for min_observations")
    stats = tiles = None
    adaptive.plan(None, uniform_share, n_paths_per_batch)
    for batch in range(max_batches):
        plot.render_adaptive(adaptive, scene, seed, stream, first_path_index + batch * n_paths_per_batch, fetch=fetch, max_segments=max_segments)
        error.observe(plot, n_paths_per_batch)
        gather.accumulate(plot)       # (and clears the plot unit)
        if batch + 1 < max(2, min_observations):
            continue
        stats, _, tiles = error.estimate(se=False)
        if stats["relative_error"] <= target_error:
            return batch + 1, stats, tiles
        if adaptive_sampling and batch + 1 < max_batches:
            adaptive.plan_from_error_tiles(tiles, uniform_share, n_paths_per_batch)
    return max_batches, stats, tiles


def render_robust_to_error(scene, plot, gather, robust, adaptive, n_paths_per_batch, max_batches, target_error, gain=1.0,
                           max_trim=0xFFFFFFFF, uniform_share=0.25, min_observations=0, seed=1, stream=0, first_path_index=0,
                           fetch=FETCH_LDS, max_segments=0, adaptive_sampling=True):
    """render_adaptive_to_error's loop on the robust film: each batch is shown to `robust` (the buckets in turn) and accumulated into
    `gather`, until rl_robust_unit_estimate's relative_error -- the noise of the film that robust.resolve writes with this gain and
    max_trim -- is at most target_error or max_batches are made.  The first estimate comes after max(M, min_observations)
    batches, M = robust.n_buckets: every bucket needs one.  Until then the plans are uniform; from then on every batch is planned
    from the estimate's tile map, which a trimmed firefly no longer inflates.  adaptive_sampling=False keeps the uniform plan
    throughout.  `robust` must be empty (RobustUnit.clear).  Returns (batches made, the last estimate's stats, its tiles)."""
    first = max(robust.n_buckets, min_observations)
    if max_batches < first:
        raise ValueError("max_batches leaves no room for one batch per bucket and min_observations")
    stats = tiles = None
    adaptive.plan(None, uniform_share, n_paths_per_batch)
    for batch in range(max_batches):
        plot.render_adaptive(adaptive, scene, seed, stream, first_path_index + batch * n_paths_per_batch, fetch=fetch, max_segments=max_segments)
        robust.observe(plot, n_paths_per_batch)
        gather.accumulate(plot)       # (and clears the plot unit)
        if batch + 1 < first:
            continue
        stats, _, tiles = robust.estimate(gain, max_trim, se=False)
        if stats["relative_error"] <= target_error:
            return batch + 1, stats, tiles
        if adaptive_sampling and batch + 1 < max_batches:
            adaptive.plan_from_error_tiles(tiles, uniform_share, n_paths_per_batch)
    return max_batches, stats, tiles


class Task:
    """enum Task (task_scheduler.rs:26-41) by unit ids."""

    def __init__(self, kind=TASK_SLEEP, unit=0, units=()):
        self.kind, self.unit, self.units = kind, unit, list(units)

    def _to_c(self):
        t = RlTask()
        t.kind, t.unit, t.n_units = self.kind, self.unit, len(self.units)
        for i, u in enumerate(self.units):
            t.units[i] = u
        return t

    @classmethod
    def _from_c(cls, t):
        return cls(t.kind, t.unit, [t.units[i] for i in range(t.n_units)])

    def __repr__(self):
        names = ["Sleep", "Trace", "Plot", "Gather", "Tonemap"]
        if self.kind == TASK_TRACE:
            return "Trace(%d)" % self.unit
        if self.kind == TASK_PLOT:
            return "Plot(%d, %r)" % (self.unit, self.units)
        if self.kind == TASK_GATHER:
            return "Gather(%r)" % (self.units,)
        return names[self.kind]

    def __eq__(self, other):
        return (self.kind, self.unit, self.units) == (other.kind, other.unit, other.units)


class TaskScheduler(_Handle):
    """task_scheduler.rs:48-325."""
    _destroy = lib.rl_scheduler_destroy

    def __init__(self, concurrency, tonemap_interval_ms=30000):
        super().__init__()
        check(lib.rl_scheduler_create(concurrency, tonemap_interval_ms, C.byref(self._h)))

    def get_new_task(self, completed_task, now_ms=0):
        c, n = completed_task._to_c(), RlTask()
        check(lib.rl_scheduler_get_new_task(self._h, C.byref(c), now_ms, C.byref(n)))
        return Task._from_c(n)

    def performance(self):
        m, s = C.c_float(0), C.c_float(0)
        check(lib.rl_scheduler_performance(self._h, C.byref(m), C.byref(s)))
        return m.value, s.value


def app_run(width, height, max_batches, concurrency=1, device=0, photons_per_batch=NUMBER_OF_PHOTONS, seed=1, stream=0,
            scene=SCENE_DEMO, scene_param=0, tonemap_interval_ms=30000, fused=False, output_ppm=None, checkpoint=None,
            resume=False, verbose=False, sleep_us=0, first_batch=0, devices=None, blocking_trace=False, threads=0,
            wavelength_importance=None, wavelength_uniform_share=0.1):
    """App::new + worker loops (app.rs:54-111) until `max_batches` trace tasks are done, on one GPU or, with
    `devices` = a list of device indices (repeats allowed), on one rank per entry with the plot buffers summed
    onto rank 0 at every gather.  `concurrency` sizes the scheduler's pools, `threads` (0 = concurrency) the host worker pool.
    wavelength_importance ("cie" or values from 380 to 780 nm) makes the trace units draw their wavelengths by importance
    (rl_app_run_sampled), wavelength_uniform_share of the density staying uniform.
    Returns (rgb image as (H, W, 3) uint8, stats dict)."""
    if wavelength_importance is not None:
        rgb, stats, _ = app_run_to_error(width, height, max_batches, None, concurrency=concurrency, device=device, photons_per_batch=photons_per_batch,
                                         seed=seed, stream=stream, scene=scene, scene_param=scene_param, tonemap_interval_ms=tonemap_interval_ms,
                                         fused=fused, output_ppm=output_ppm, checkpoint=checkpoint, resume=resume, verbose=verbose,
                                         sleep_us=sleep_us, first_batch=first_batch, devices=devices, blocking_trace=blocking_trace,
                                         threads=threads, wavelength_importance=wavelength_importance,
                                         wavelength_uniform_share=wavelength_uniform_share)
        return rgb, stats
    dev_arr = (C.c_int * len(devices))(*devices) if devices else None
    cfg = RlAppConfig(width, height, device, concurrency, photons_per_batch, seed, stream, scene, scene_param, max_batches,
                      tonemap_interval_ms, int(fused), output_ppm.encode() if output_ppm else None,
                      checkpoint.encode() if checkpoint else None, int(resume), int(verbose), sleep_us, first_batch,
                      len(devices) if devices else 0, int(blocking_trace), dev_arr, int(threads))
    stats = RlAppStats()
    rgb = np.zeros((height, width, 3), dtype=np.uint8)
    check(lib.rl_app_run(C.byref(cfg), C.byref(stats), rgb.ctypes.data_as(C.c_void_p)))
    return rgb, _app_stats(stats)


def _app_stats(stats):
    out = {name: getattr(stats, name) for name, _ in RlAppStats._fields_ if name != "tasks"}
    out["tasks"] = dict(zip(["sleep", "trace", "plot", "gather", "tonemap"], list(stats.tasks)))
    return out


def app_run_to_error(width, height, max_batches, target_error=None, worst_tile_error=0.0, min_observations=0, concurrency=1, device=0,
                     photons_per_batch=NUMBER_OF_PHOTONS, seed=1, stream=0, scene=SCENE_DEMO, scene_param=0, tonemap_interval_ms=30000,
                     fused=False, output_ppm=None, checkpoint=None, resume=False, verbose=False, sleep_us=0, first_batch=0, devices=None,
                     blocking_trace=False, threads=0, reserved=0, wavelength_importance=None, wavelength_uniform_share=0.1):
    """rl_app_run_to_error: app_run that ends the hand-out of batches once an estimate made at a tonemap (every tonemap_interval_ms)
    has at least min_observations (0 = 16) observations and a relative error <= target_error (and, with a non-zero worst_tile_error,
    a worst tile <= it); max_batches stays the cap.  target_error=None passes no target: app_run.  wavelength_importance ("cie" or
    values from 380 to 780 nm) makes the trace units draw their wavelengths by importance (rl_app_run_sampled).  Returns (rgb, stats dict, error
    dict {at_stop, at_end: rl_error_unit_estimate's stats, reached, estimates, tiles: at_end's (tiles_y, tiles_x, 2) pairs or None})."""
    dev_arr = (C.c_int * len(devices))(*devices) if devices else None
    cfg = RlAppConfig(width, height, device, concurrency, photons_per_batch, seed, stream, scene, scene_param, max_batches,
                      tonemap_interval_ms, int(fused), output_ppm.encode() if output_ppm else None,
                      checkpoint.encode() if checkpoint else None, int(resume), int(verbose), sleep_us, first_batch,
                      len(devices) if devices else 0, int(blocking_trace), dev_arr, int(threads))
    target = None if target_error is None else C.byref(RlErrorTarget(target_error, worst_tile_error, min_observations, reserved))
    stats, es = RlAppStats(), RlAppErrorStats()
    rgb = np.zeros((height, width, 3), dtype=np.uint8)
    g = _wavelength_importance(wavelength_importance)
    if g is None:
        check(lib.rl_app_run_to_error(C.byref(cfg), target, C.byref(stats), C.byref(es), rgb.ctypes.data_as(C.c_void_p)))
    else:
        sampling = RlWavelengthSampling(g.ctypes.data, len(g), 0, wavelength_uniform_share)
        check(lib.rl_app_run_sampled(C.byref(cfg), target, C.byref(sampling), C.byref(stats), C.byref(es), rgb.ctypes.data_as(C.c_void_p)))
    n = C.c_uint32(0)
    lib.rl_app_error_tiles(None, 0, C.byref(n))     # (RL_E_INVALID when there are tiles: the count is what is asked for)
    tiles = None
    if n.value:
        tiles = np.zeros((-(-height // RL_ERROR_TILE), -(-width // RL_ERROR_TILE), 2), dtype=np.float64)
        check(lib.rl_app_error_tiles(tiles.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    error = {"at_stop": _error_stats(es.at_stop), "at_end": _error_stats(es.at_end), "reached": es.reached, "estimates": es.estimates,
             "tiles": tiles}
    return rgb, _app_stats(stats), error


def app_error_state():
    """rl_app_error_state: (S, Q as flat float64 arrays of width * height, k, N) of the error unit at the end of this thread's last
    app_run_to_error; empty arrays and zeros after a run without a target or without an observation.  Reshape to (height, width)
    and ErrorUnit.upload them to estimate again or to DenoiseUnit.denoise_variance the run's image."""
    n, k, paths = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lib.rl_app_error_state(None, None, 0, C.byref(n), C.byref(k), C.byref(paths))   # (RL_E_INVALID when there is a state: the size is what is asked for)
    s, q = np.zeros(n.value, dtype=np.float64), np.zeros(n.value, dtype=np.float64)
    if n.value:
        check(lib.rl_app_error_state(s.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(k), C.byref(paths)))
    return s, q, k.value, paths.value


def batch_histogram(device=0):
    """{k: open launches that carried k blocking render calls} since the library was loaded (waits for running ones)."""
    out = (C.c_uint64 * 257)()
    check(lib.rl_debug_batch_histogram(device, out))
    return {k: int(out[k]) for k in range(1, 257) if out[k]}


def _launch_counters(symbol, n, kind):
    """The n launch counters that `symbol` fills, as a list (a kernel family's instantiations) or a tuple (a unit's two kernels)."""
    out = (C.c_uint64 * n)()
    check(symbol(out))
    return kind(int(x) for x in out)


def variant_launches():
    """rl_debug_variant_launches: launches per instantiation of the trace kernel since the library was loaded;
    index = 8 * whole scene staged in LDS + 4 * fused + 2 * open launch + 1 * prisms with a second bound; 16 + the low three
    bits for the variants that stage the scene's tables only."""
    return _launch_counters(lib.rl_debug_variant_launches, 24, list)


def wavelength_variant_launches():
    """rl_debug_wavelength_variant_launches: the same for the instantiations that draw the wavelength from a table (a TraceUnit after
    set_wavelengths), indexed as variant_launches is, which does not count them."""
    return _launch_counters(lib.rl_debug_wavelength_variant_launches, 24, list)


def query_launches():
    """rl_debug_query_launches: launches per instantiation of the query kernel (Scene.intersect*) since the library was loaded;
    index = 2 * stage + 1 * prisms with a second bound, stage 0: nothing staged in LDS, 1: the scene's tables, 2: the whole scene."""
    return _launch_counters(lib.rl_debug_query_launches, 6, list)


def occlusion_launches():
    """rl_debug_occlusion_launches: launches per instantiation of the occlusion kernel (Scene.occluded*) since the library was
    loaded, indexed as query_launches()."""
    return _launch_counters(lib.rl_debug_occlusion_launches, 6, list)


def path_launches():
    """rl_debug_path_launches: launches per instantiation of the path kernel (Scene.render_rays*) since the library was loaded,
    indexed as query_launches()."""
    return _launch_counters(lib.rl_debug_path_launches, 6, list)


def film_launches():
    """rl_debug_film_launches: launches per instantiation of the film path kernel (PlotUnit.render_samples*) since the library was
    loaded, indexed as query_launches()."""
    return _launch_counters(lib.rl_debug_film_launches, 6, list)


def step_launches():
    """rl_debug_step_launches: launches per instantiation of the step kernel (Scene.step_paths*) since the library was loaded,
    indexed as query_launches()."""
    return _launch_counters(lib.rl_debug_step_launches, 6, list)


def path_list_launches():
    """rl_debug_path_list_launches: launches per instantiation of the list-step kernel (Scene.step_path_list*) since the library
    was loaded, indexed as query_launches()."""
    return _launch_counters(lib.rl_debug_path_list_launches, 6, list)


def light_launches():
    """Launches per light-kernel instantiation since the library was loaded (rl_debug_light_launches); index = 2 * stage +
    (prisms carry a second bound), as query_launches()."""
    return _launch_counters(lib.rl_debug_light_launches, 6, list)


def light_film_launches():
    """Launches per instantiation of the light kernel with a film (PlotUnit.light_paths*, PlotUnit.render_samples_direct*) since the
    library was loaded (rl_debug_light_film_launches); index = 2 * stage + cylinders, as light_launches()."""
    return _launch_counters(lib.rl_debug_light_film_launches, 6, list)


def direct_launches():
    """Launches per instantiation of the direct path kernel (PlotUnit.render_direct) since the library was loaded
    (rl_debug_direct_launches); index = 2 * stage + cylinders, as light_launches()."""
    return _launch_counters(lib.rl_debug_direct_launches, 6, list)


def feature_launches():
    """Launches per instantiation of the feature path kernel (Scene.render_features) since the library was loaded
    (rl_debug_feature_launches); index = 2 * stage + cylinders, as light_launches()."""
    return _launch_counters(lib.rl_debug_feature_launches, 6, list)


def denoise_launches():
    """(launches of the denoiser's guide kernel, launches of its pass kernel) since the library was loaded
    (rl_debug_denoise_launches): one and `iterations` per DenoiseUnit.denoise."""
    return _launch_counters(lib.rl_debug_denoise_launches, 2, tuple)


def denoise_variance_launches():
    """(launches of the V_0 kernel, launches of the variance form of the pass kernel) since the library was loaded
    (rl_debug_denoise_variance_launches): one and `iterations` per DenoiseUnit.denoise_variance, whose guide launch counts in
    denoise_launches()."""
    return _launch_counters(lib.rl_debug_denoise_variance_launches, 2, tuple)


def spectral_launches():
    """(launches of the spectral film's splat kernel, launches of its projection kernel) since the library was loaded
    (rl_debug_spectral_launches)."""
    return _launch_counters(lib.rl_debug_spectral_launches, 2, tuple)


def glare_launches():
    """Launches of the glare kernel (GlareUnit.apply) since the library was loaded (rl_debug_glare_launches)."""
    out = C.c_uint64(0)
    check(lib.rl_debug_glare_launches(C.byref(out)))
    return out.value


def relight_launches():
    """(launches of the relight film's routed splat kernel, path kernel launches of RelightUnit.render, launches of its mix) since
    the library was loaded (rl_debug_relight_launches)."""
    return _launch_counters(lib.rl_debug_relight_launches, 3, tuple)


def gather_accumulate_ms(gather, plot_unit):
    """rl_debug_gather_accumulate_ms: gather.accumulate(plot_unit), returning the device milliseconds of its kernel launch."""
    ms = C.c_float(0)
    check(lib.rl_debug_gather_accumulate_ms(gather.handle, plot_unit.handle, C.byref(ms)))
    return ms.value


def error_launches():
    """(launches of the error unit's observe kernel, launches of its estimate kernel) since the library was loaded
    (rl_debug_error_launches)."""
    return _launch_counters(lib.rl_debug_error_launches, 2, tuple)


def robust_launches():
    """(launches of the robust unit's observe kernel, launches of its resolve kernel) since the library was loaded
    (rl_debug_robust_launches)."""
    return _launch_counters(lib.rl_debug_robust_launches, 2, tuple)


def robust_estimate_launches():
    """Launches of the robust unit's estimate kernel since the library was loaded (rl_debug_robust_estimate_launches)."""
    out = C.c_uint64(0)
    check(lib.rl_debug_robust_estimate_launches(C.byref(out)))
    return out.value


def adaptive_launches():
    """(sample kernel launches, path kernel launches made by render_adaptive, splat kernel launches) since the library was loaded
    (rl_debug_adaptive_launches)."""
    return _launch_counters(lib.rl_debug_adaptive_launches, 3, tuple)


def live_resources():
    """rl_debug_live_resources: (device allocations, streams, plain events, timed event pairs) that the live handles of this
    process hold, all devices together."""
    out = (C.c_uint64 * 4)()
    check(lib.rl_debug_live_resources(out))
    return tuple(int(x) for x in out)


def description_emitters(objects):
    """rl_debug_scene_emitters: the object indices of the sampleable emitters of an OBJECT_DTYPE description, without a device."""
    objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
    n = C.c_uint32(0)
    lib.rl_debug_scene_emitters(objects.ctypes.data_as(C.c_void_p), len(objects), None, 0, C.byref(n))
    out = np.zeros(n.value, dtype=np.uint32)
    check(lib.rl_debug_scene_emitters(objects.ctypes.data_as(C.c_void_p), len(objects), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return out


def light_sample_host(objects, states, hits, seed, stream):
    """rl_debug_light_sample: the host compile of the light sampling function for (n,) PATH_STATE_DTYPE states and HIT_DTYPE hits
    against the emitters of an OBJECT_DTYPE description; no device.  Returns (samples, rays): LIGHT_SAMPLE_DTYPE records as the
    call writes them for an unblocked ray, and the RAY_DTYPE shadow rays (all zero where none is cast)."""
    objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
    states = np.ascontiguousarray(states, dtype=PATH_STATE_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if len(hits) != len(states):
        raise ValueError("states and hits differ in length")
    samples = np.zeros(len(states), dtype=LIGHT_SAMPLE_DTYPE)
    rays = np.zeros(len(states), dtype=RAY_DTYPE)
    check(lib.rl_debug_light_sample(objects.ctypes.data_as(C.c_void_p), len(objects), seed, stream, states.ctypes.data_as(C.c_void_p),
                                    hits.ctypes.data_as(C.c_void_p), len(states), samples.ctypes.data_as(C.c_void_p), rays.ctypes.data_as(C.c_void_p)))
    return samples, rays


def math_probe(fn, x, device=0):
    """Evaluates csrc/rl_math.h function `fn` on the GPU (diagnostics for the parity tests)."""
    names = {"sin": 0, "cos": 1, "tan": 2, "exp": 3, "log": 4, "acos": 5, "sf10": 6, "sqrt": 7, "div": 8, "gamma": 9, "roulette": 10, "normalise": 11, "sin_d": 12, "cos_d": 13, "exp_d": 14, "acos_d": 15, "sqrt_short": 16, "recip_short": 17, "div200_short": 18}
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros_like(x)
    check(lib.rl_debug_math_probe(device, names[fn], x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size))
    return y


def math_sweep(fn, lo_bits, hi_bits, both_signs=False, device=0):
    """rl_debug_math_sweep: the short form `fn` ("sqrt_short", "recip_short", "div200_short") against the compiler's IEEE expansion
    on the device for every float with bits in [lo_bits, hi_bits) (and its negative): (mismatches, compared, example bits)."""
    counts = (C.c_uint64 * 2)()
    example = C.c_uint32(0)
    check(lib.rl_debug_math_sweep(device, {"sqrt_short": 16, "recip_short": 17, "div200_short": 18}[fn], int(lo_bits), int(hi_bits),
                                  1 if both_signs else 0, counts, C.byref(example)))
    return int(counts[0]), int(counts[1]), int(example.value)


def app_rank_plan(devices=None, device=0):
    """rl_debug_app_rank_plan: (rank_device, leader, comm_rank, communicator size) of rl_app_run for `devices` (no GPU needed)."""
    n = len(devices) if devices else 0
    m = max(n, 1)
    dev = (C.c_int * n)(*devices) if n else None
    rd, ld, cr, size = (C.c_int * m)(), (C.c_int * m)(), (C.c_int * m)(), C.c_uint32(0)
    check(lib.rl_debug_app_rank_plan(device, dev, n, rd, ld, cr, C.byref(size)))
    return list(rd), list(ld), list(cr), int(size.value)


def prism_probe(scene, prism, rays):
    """rl_debug_prism_probe: the prism shortcut (rl_hex_prism_fast) and the Compound tree, both on the GPU, for `rays`
    (n x 6: origin, direction) against prism number `prism` of the scene's flattened order.  Returns an (n, 5) uint32
    array: status (0 miss, 1 hit, 2 undecided), shortcut {t bits, half-space}, tree {t bits or 0xffffffff, half-space}."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros((len(rays), 5), dtype=np.uint32)
    check(lib.rl_debug_prism_probe(scene.handle, int(prism), rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.c_void_p)))
    return out


def prism_count(scene):
    n = C.c_uint32(0)
    check(lib.rl_debug_prism_count(scene.handle, C.byref(n)))
    return n.value
