"""The comparison helpers the GPU tests share (tests/_compare.py, tests/_boundary.py: _variant_of, tests/_scenes.py: _scene) on small
arrays made by hand, without a GPU: they pass on equal bytes, and they fail -- naming the place -- on one byte's difference, a
reserved byte's included."""
import numpy as np
import pytest

import robigo_luculenta_amd as R
from _boundary import _variant_of
from _compare import assert_same, assert_same_bytes
from _scenes import _scene

N = 8


def _records(dtype):
    """N records of `dtype` whose every byte is set and differs from its neighbours'."""
    return ((np.arange(N * dtype.itemsize) * 7 + 1) % 251).astype(np.uint8).view(dtype).copy()


def _with_byte_flipped(a, row, offset):
    b = a.copy()
    b.view(np.uint8).reshape(N, a.dtype.itemsize)[row, offset] ^= 0x01
    return b


@pytest.mark.parametrize("dtype", [R.HIT_DTYPE, R.PATH_RESULT_DTYPE], ids=["hit", "path_result"])
def test_assert_same_passes_on_equal_bytes(dtype):
    a = _records(dtype)
    assert_same(a, a.copy(), "equal")
    assert_same(a[:0], a[:0].copy(), "empty")


@pytest.mark.parametrize("dtype, field", [(R.HIT_DTYPE, "distance"), (R.HIT_DTYPE, "object"), (R.PATH_RESULT_DTYPE, "value"),
                                          (R.PATH_RESULT_DTYPE, "end")])
def test_assert_same_names_the_first_row_that_differs_in_a_field(dtype, field):
    a = _records(dtype)
    b = _with_byte_flipped(_with_byte_flipped(a, 5, dtype.fields[field][1]), 6, 0)
    assert a[field][5] != b[field][5] or np.isnan(a[field][5])
    with pytest.raises(AssertionError, match=r"a field: 2 of 8 records differ, first 5: got "):
        assert_same(b, a, "a field")


def test_assert_same_sees_a_reserved_byte():
    a = _records(R.HIT_DTYPE)
    offset = R.HIT_DTYPE.fields["reserved"][1] + 3
    assert offset == R.HIT_DTYPE.itemsize - 1      # the record's last byte: nothing but the whole record's bytes covers it
    b = _with_byte_flipped(a, 3, offset)
    for f in R.HIT_DTYPE.names:
        if f != "reserved":
            assert a[f].tobytes() == b[f].tobytes(), f
    with pytest.raises(AssertionError, match=r"reserved: 1 of 8 records differ, first 3: got "):
        assert_same(b, a, "reserved")


def test_assert_same_bytes():
    a = (np.arange(N) % 2).astype(np.uint8)
    assert_same_bytes(a, a.copy(), "equal")
    b = a.copy()
    b[4] ^= 1
    b[7] ^= 1
    with pytest.raises(AssertionError, match=r"bytes: 2 of 8 rays differ, first 4: got 1 want 0"):
        assert_same_bytes(b, a, "bytes")
    with pytest.raises(AssertionError):
        assert_same_bytes(a.astype(np.int8), a, "another type")
    with pytest.raises(AssertionError):
        assert_same_bytes(a[:7], a, "another length")


def _counters(moved):
    """(launches, before): six counters of which those in `moved` went up since `before` was read."""
    before = [3, 0, 9, 1, 0, 4]
    return (lambda: [b + (2 if i in moved else 0) for i, b in enumerate(before)]), before


@pytest.mark.parametrize("index", range(6))
def test_variant_of_returns_the_one_counter_that_moved(index):
    assert _variant_of(*_counters({index})) == index


@pytest.mark.parametrize("moved", [set(), {1, 4}], ids=["none", "two"])
def test_variant_of_refuses_none_and_two(moved):
    with pytest.raises(AssertionError):
        _variant_of(*_counters(moved))


def test_scene_raises_key_error_on_an_unknown_name():
    for name in ("no-such-scene", "degenerate-no-such-layout", ""):
        with pytest.raises(KeyError):
            _scene(name)
