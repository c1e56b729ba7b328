"""What the tests of the C ABI's boundary share: the last error's text, a stand-in handle, the oracle's camera record and the
kernel variant a call ran on."""
import ctypes as C

from robigo_luculenta_amd import _lib


def _err():
    return _lib.lib.rl_last_error()


class _Fake:
    """A handle for the checks that come before the handle is read or a device is touched: every one of them must refuse first
    (the pointer is never dereferenced when an argument is bad)."""

    def __init__(self):
        self.buf = (C.c_uint8 * 256)()
        self.ptr = C.cast(self.buf, C.c_void_p)


_FakeScene = _Fake


def _ocam(cam):
    """The package's camera record as the oracle's."""
    import _oracle as O
    return O.RlCameraDesc.from_buffer_copy(bytes(cam))


def _variant_of(launches, before):
    """The index of the one kernel variant that ran since `before` = launches() was read (R.query_launches and its like)."""
    ran = [a - b for a, b in zip(launches(), before)]
    assert sum(1 for r in ran if r) == 1, ran
    return next(i for i, r in enumerate(ran) if r)
