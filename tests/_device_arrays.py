"""Arrays in device memory for the _device forms of the C ABI, and the prefilled host arrays that show what a call wrote: record
arrays and uint32 words with their host copies, begun path states, hits and light samples that hold a poison pattern."""
import ctypes as C

import numpy as np

import robigo_luculenta_amd as R
import _guarded as G
import _lds_poison as LP
import _query_rays as QR


class _Device:
    """An (n,) record array in device memory."""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a).copy()
        self.buf = QR.DeviceBuffer(max(self.host.nbytes, 64))
        if self.host.nbytes:
            self.buf.upload(self.host)

    def get(self):
        if self.host.nbytes:
            self.buf.download(self.host)
        return self.host


class _Words:
    """n uint32 in device memory."""

    def __init__(self, a):
        self.host = np.ascontiguousarray(a, dtype=np.uint32).copy()
        self.buf = QR.DeviceBuffer(max(self.host.nbytes, 64))
        if self.host.nbytes:
            self.buf.upload(self.host)

    def get(self):
        if self.host.nbytes:
            self.buf.download(self.host)
        return self.host


def _upload(a):
    """A device buffer of exactly a's bytes, without a host copy."""
    b = QR.DeviceBuffer(a.nbytes)
    b.upload(np.ascontiguousarray(a))
    return b


def _begin_device(scene, rays, first):
    rb = _Device(np.ascontiguousarray(rays))
    poison = np.zeros(len(rays), R.PATH_STATE_DTYPE)
    poison["end"] = 12345   # every record must be written
    sb = _Device(poison)
    R.check(R.lib.rl_scene_begin_paths_device(scene.handle, first, C.c_void_p(rb.buf.data_ptr()), len(rays), C.c_void_p(sb.buf.data_ptr())))
    return sb


def _poison_hits(n):
    return np.frombuffer(bytes([0xa5]) * (48 * n), dtype=R.HIT_DTYPE).copy()


def _prefilled(n):
    """n light samples that hold the guard's fill."""
    return np.frombuffer(bytes([G.FILL]) * (32 * n), dtype=R.LIGHT_SAMPLE_DTYPE).copy()


def _slice_crossing_size():
    """A list longer than the slice rule's threshold whatever the residency (16 states per lane of a grid of at most two
    workgroups of 1,024 threads per CU), and not a multiple of 64 or of the slice."""
    return LP.cu_count() * 2 * 1024 * 16 + 4097
