"""tests/_guarded.py on the CPU, with host memory standing in for the device buffer: the helper must FAIL for a writer that goes one
record beyond its output (a buffer that is one record short for it), one that starts a record early and one that leaves a record,
or a reserved field, unwritten -- and pass for a writer that writes exactly its records.  Without this the GPU tests that use the
helper (tests/test_gpu_dirty_state.py) could pass vacuously.  The poison helper must import without a GPU."""
import ctypes as C

import numpy as np
import pytest

import _guarded as G

REC = np.dtype([("value", "<f4"), ("object", "<u4"), ("reserved", "<u4")])


def _records(n):
    r = np.zeros(n, REC)
    r["value"], r["object"] = np.arange(n) + 0.5, np.arange(n)
    return r


def _write(buf, records, offset=0):
    """The stand-in kernel: `records` at `offset` bytes from the payload's start, as a device kernel would through data_ptr()."""
    C.memmove(buf.data_ptr() + offset, records.ctypes.data, records.nbytes)


@pytest.mark.parametrize("front", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4033])
def test_exact_writer_passes(n, front):
    want = _records(n)
    g = G.Guarded(G.HostBuffer, want.nbytes, front=front)
    assert g.numel() * g.element_size() == want.nbytes and g.data_ptr() % 16 == g.buf.data_ptr() % 16
    assert (g.payload("prefill") == G.FILL).all()
    _write(g, want)
    G.assert_written_as(g.payload("exact", REC), want, "exact")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4033])
def test_a_buffer_one_record_short_fails(n):
    """The writer writes n records into an output that has room for n - 1: the last one lands in the guard."""
    g = G.Guarded(G.HostBuffer, (n - 1) * REC.itemsize)
    _write(g, _records(n))
    with pytest.raises(AssertionError, match="BEHIND"):
        g.payload("short")


def test_a_single_byte_behind_the_output_fails():
    g = G.Guarded(G.HostBuffer, 65)
    _write(g, np.zeros(66, np.uint8))
    with pytest.raises(AssertionError, match="BEHIND"):
        g.payload("one byte")


def test_a_write_in_front_of_the_output_fails():
    g = G.Guarded(G.HostBuffer, 64 * REC.itemsize)
    _write(g, _records(1), offset=-REC.itemsize)
    with pytest.raises(AssertionError, match="IN FRONT"):
        g.payload("early")


def test_an_unwritten_record_or_reserved_field_fails():
    want = _records(65)
    g = G.Guarded(G.HostBuffer, want.nbytes)
    _write(g, want[:64])                                  # the tail wave's record is missing
    with pytest.raises(AssertionError, match="record 64 .*never written"):
        G.assert_written_as(g.payload("tail", REC), want, "tail")
    g = G.Guarded(G.HostBuffer, want.nbytes)
    _write(g, want)
    _write(g, np.full(4, G.FILL, np.uint8), offset=7 * REC.itemsize + 8)   # as if record 7's reserved word had been skipped
    with pytest.raises(AssertionError, match="record 7 at byte 8"):
        G.assert_written_as(g.payload("reserved", REC), want, "reserved")


def test_initial_payload_is_kept_and_compared():
    st = _records(10)
    g = G.Guarded(G.HostBuffer, initial=st)
    G.assert_written_as(g.payload("initial", REC), st, "initial")
    with pytest.raises(AssertionError):
        G.assert_written_as(g.payload("initial", REC), _records(10)[::-1].copy(), "initial")


def test_poison_helper_imports_without_a_gpu():
    import _lds_poison as LP
    assert LP.PATTERNS == (0xFFFFFFFF, 0x7FC00000, 0x00ABCDEF) and LP._poison_lds is LP.poison_lds
