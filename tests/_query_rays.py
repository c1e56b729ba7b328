"""Ray sets for Scene.intersect (tests/_cases.py, tools/query_bench.py): camera-like rays through a jittered pixel grid
and bounce-like rays that leave the camera rays' hits in uniform directions.  Host arithmetic (numpy), and DeviceBuffer for the device path."""
import ctypes as C

import numpy as np


def camera_frame(cam, t=0.0):
    """Position of the camera of an RlCameraDesc at time t (include/robigo_luculenta.h: make_camera, app.rs:327-357), and a
    pinhole frame looking at the scene's origin with its field of view."""
    phi = np.pi * (cam.phi0 + cam.phi1 * t)
    alpha = np.pi * (cam.alpha0 + cam.alpha1 * t)
    dist = cam.dist0 + cam.dist1 * t
    pos = np.array([np.cos(alpha) * np.sin(phi), np.cos(alpha) * np.cos(phi), np.sin(alpha)]) * dist
    fwd = -pos / np.linalg.norm(pos)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return pos, fwd, right, up, np.pi * cam.fov_over_pi


def camera_rays(cam, width, height, rng, n=None):
    """(origins, directions) float32 of n rays through a width x height grid, each jittered inside its pixel (all pixels in row
    order when n is None, else n random pixels).  Directions are unit vectors."""
    pos, fwd, right, up, fov = camera_frame(cam)
    pix = np.arange(width * height, dtype=np.int64) if n is None else rng.integers(0, width * height, n)
    sx = ((pix % width) + rng.random(len(pix))) / width * 2.0 - 1.0
    sy = ((pix // width) + rng.random(len(pix))) / height * 2.0 - 1.0
    half = np.tan(fov * 0.5)
    d = fwd[None, :] + (sx * half)[:, None] * right[None, :] + (-sy * half * height / width)[:, None] * up[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(pos, d.shape)
    return np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)


def uniform_directions(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def bounce_rays(origins, directions, hits, rng):
    """Rays from the hits of (origins, directions) -- HIT_DTYPE records -- offset by 1e-5 * direction (so they start just behind
    the surface: inside glass, just inside or outside a sphere), in uniform directions.  Misses are dropped."""
    m = hits["object"] != 0xffffffff
    o = (hits["position"][m] + np.float32(1e-5) * directions[m]).astype(np.float32)
    return np.ascontiguousarray(o), uniform_directions(rng, int(m.sum()))


class DeviceBuffer:
    """Device memory through the HIP runtime the library uses, with the data_ptr() / numel() / element_size() that
    Scene.intersect_device reads (the interface of a torch tensor)."""
    _hip = None

    def __init__(self, nbytes):
        if DeviceBuffer._hip is None:
            DeviceBuffer._hip = C.CDLL("libamdhip64.so.7")
        self.ptr, self.nbytes = C.c_void_p(), nbytes
        assert self._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(nbytes, 1))) == 0

    def data_ptr(self):
        return self.ptr.value

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def upload(self, a):
        assert self._hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0   # hipMemcpyHostToDevice

    def download(self, a):
        assert self._hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(a.nbytes), 2) == 0   # hipMemcpyDeviceToHost

    def __del__(self):
        self._hip.hipFree(self.ptr)
