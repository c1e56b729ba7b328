"""Guarded, prefilled output buffers for the _device forms of the C ABI (tests/test_gpu_dirty_state.py): the payload a kernel is
to write lies between two guards of 64 bytes, the whole allocation is filled with 0xAA first, and after the call the guards must
be intact and the payload must hold, byte for byte, what the host form returned -- so a tail wave that writes one record too many
and a slot, padding or reserved field that is left unwritten (and would pass on a zeroed buffer) both fail.  The allocator is a
parameter: tests/_query_rays.DeviceBuffer on the GPU, HostBuffer (numpy) in the helper's own CPU test."""
import ctypes as C

import numpy as np

import _query_rays as QR

GUARD = 64    # bytes in front of and behind the payload; a multiple of every alignment the ABI asks for (16 bytes: RlPathState)
FILL = 0xAA   # 0xAAAAAAAA is no value a kernel writes: a finite, tiny negative float (-3.0e-13), an object index beyond any scene


class HostBuffer:
    """The interface of tests/_query_rays.DeviceBuffer over host memory: the stand-in for the helper's CPU test."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.mem = np.zeros(max(nbytes, 1), np.uint8)

    def data_ptr(self):
        return self.mem.ctypes.data

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def upload(self, a):
        C.memmove(self.mem.ctypes.data, a.ctypes.data, a.nbytes)

    def download(self, a):
        C.memmove(a.ctypes.data, self.mem.ctypes.data, a.nbytes)


class Guarded:
    """`nbytes` of payload with a guard behind it and (front=True) one in front, all of it FILL; or, with `initial`, that array's
    bytes as the payload (a state array stepped in place).  Has the data_ptr() / numel() / element_size() the package's _device
    wrappers read, for the payload alone."""

    def __init__(self, alloc, nbytes=None, initial=None, front=True):
        if initial is not None:
            initial = np.ascontiguousarray(initial)
            nbytes = initial.nbytes
        self.nbytes, self.front = int(nbytes), GUARD if front else 0
        self.whole = self.front + self.nbytes + GUARD
        self.buf = alloc(self.whole)
        image = np.full(self.whole, FILL, np.uint8)
        if initial is not None:
            image[self.front:self.front + self.nbytes] = initial.view(np.uint8).reshape(-1)
        self.buf.upload(image)

    def data_ptr(self):
        return self.buf.data_ptr() + self.front

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def payload(self, what, dtype=np.uint8):
        """Downloads everything, asserts that both guards still hold FILL and returns the payload as `dtype` records."""
        image = np.zeros(self.whole, np.uint8)
        self.buf.download(image)
        lo, hi = image[:self.front], image[self.front + self.nbytes:]
        assert (hi == FILL).all(), "%s: %d guard bytes BEHIND the %d-byte output were written, first at +%d: %r" % (
            what, int((hi != FILL).sum()), self.nbytes, int(np.flatnonzero(hi != FILL)[0]), hi[:16])
        assert (lo == FILL).all(), "%s: %d guard bytes IN FRONT of the output were written, first at -%d" % (
            what, int((lo != FILL).sum()), self.front - int(np.flatnonzero(lo != FILL)[-1]))
        return image[self.front:self.front + self.nbytes].copy().view(dtype)


def device_guarded(nbytes=None, initial=None):
    """A Guarded buffer in device memory."""
    return Guarded(QR.DeviceBuffer, nbytes=nbytes, initial=initial)


def assert_written_as(got, want, what):
    """`got` (a payload) equals `want` (the host form's records) byte for byte; the message names the first differing record and
    says whether it still holds the prefill, i.e. was never written."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert g.size == w.size, (what, g.size, w.size)
    if g.tobytes() == w.tobytes():
        return
    size = max(1, want.dtype.itemsize)
    bad = np.flatnonzero(g != w)
    rec = int(bad[0]) // size
    left = bad[g[bad] == FILL]
    raise AssertionError("%s: %d of %d bytes differ from the host form, first in record %d at byte %d; %d of them still hold the 0x%02X "
                         "prefill (never written): got %r want %r" % (what, len(bad), g.size, rec, int(bad[0]) % size, len(left), FILL,
                                                                      g[rec * size:(rec + 1) * size].tobytes(), w[rec * size:(rec + 1) * size].tobytes()))
