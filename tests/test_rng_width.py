"""The full-width RNG cases of tests/_rng_width.py, without a GPU: each case has the property it is there for; the CPU oracle's
words and the x, y and wavelength of its photons equal tools/independent_paths.py's numpy Philox at every path of every case
(from here on the oracle is a reference that does not rest on rl_rng.h's text at these coordinates, and
tests/test_gpu_rng_width.py holds the kernels to it); and the Python step and light oracles form their blocks as the 32-bit
sums the C forms."""
import ctypes as C

import numpy as np
import pytest

import _light_oracle as LO
import _oracle as O
import _rng_width as RW
import _step_oracle as S
from _cases import vertex_states
from _scenes import closed_scene

M32 = RW.M32


@pytest.fixture(scope="module")
def demo():
    objs, cam = O.demo_scene_desc()
    return O.Scene(objs, cam)


@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_each_case_has_the_property_its_row_names(case):
    for n in (RW.N_TRACE, RW.N_QUERY):
        assert 0 <= case.first and case.first + n < RW.LAST, "the range is legal"        # (first + n must stay below 2^64 - 1)
        assert 0 <= case.seed < 1 << 64 and 0 <= case.stream < 1 << 32
        if case.id in RW.CARRY_LANE:
            assert RW.carry_position(case.first, n) == RW.CARRY_LANE[case.id], "the carry falls inside the launch, where the row says"
            paths = RW.paths_of(case.first, n)
            at = 64 * RW.CARRY_LANE[case.id][0] + RW.CARRY_LANE[case.id][1]
            assert int(paths[at]) & M32 == 0 and int(paths[at - 1]) & M32 == M32 and int(paths[at] >> np.uint64(32)) == int(paths[at - 1] >> np.uint64(32)) + 1
    assert RW.N_TRACE % 64 == 0 and RW.N_QUERY % 64 == 1
    if case.id == "carry-mid-wave":
        assert (case.seed, case.stream) == (7, 1)
    if case.id == "carry-wave-edge":
        assert (case.first + 2048) >> 32 >= 2 and (case.first + 2048) % 64 == 0
    if case.id == "seed-high":
        assert case.seed >> 32 != 0 and (case.seed & M32, case.stream, case.first) == (7, 1, 0)
    if case.id in ("stream-high", "stream-msb"):
        assert case.stream >> 31 == 1 and (case.seed, case.first) == (7, 0)
    if case.id == "sign-carry":
        assert case.first < 1 << 63 <= case.first + RW.N_QUERY - 1 and case.seed >> 63 == 1 and case.stream >> 31 == 1
    if case.id == "top":
        assert case.first + RW.N_TRACE == RW.LAST - 1 and case.seed == (1 << 64) - 1 and case.stream == M32
    assert {c.stream for c in RW.CASES} >= {0xFFFFFFFF, 0x80000001}


@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_oracle_words_are_the_numpy_philox_at_every_path_of_the_case(case):
    paths = RW.paths_of(case.first, RW.N_TRACE)
    for block in RW.ORACLE_BLOCKS:
        got = np.zeros((len(paths), 4), np.uint32)
        blocks = np.full(len(paths), block, np.uint32)
        O.lib().oracle_rng_blocks(case.seed, case.stream, O.ptr(paths), O.ptr(blocks), O.ptr(got), len(paths))
        want = RW.numpy_words(case.seed, case.stream, paths, block)
        assert np.array_equal(got, want), (case.id, block, np.flatnonzero((got != want).any(axis=1))[:4])
        one = np.zeros(4, np.uint32)      # the single-block entry point the step and path oracles use
        O.lib().oracle_rng_block(case.seed, case.stream, int(paths[-1]), block, O.ptr(one))
        assert one.tolist() == want[-1].tolist(), (case.id, block)


@pytest.mark.parametrize("case", RW.CASES, ids=RW.IDS)
def test_oracle_photons_are_drawn_from_the_numpy_words(demo, case):
    """x, y and wavelength of oracle.render's photons, bit for bit: pins the oracle's own first + i."""
    n = RW.N_TRACE
    got, _ = demo.render(RW.W, RW.H, case.seed, case.stream, case.first, n, threads=4)
    x, y, wavelength = RW.numpy_camera(case.seed, case.stream, case.first, n)
    for name, want in (("x", x), ("y", y), ("wavelength", wavelength)):
        bad = np.flatnonzero(got[name].view(np.uint32) != want.view(np.uint32))
        assert not len(bad), (case.id, name, len(bad), bad[:4], got[name][bad[:4]], want[bad[:4]])
    one, _ = demo.render(RW.W, RW.H, case.seed, case.stream, case.first, n)
    assert one.tobytes() == got.tobytes()
    if case.id == "seed-high":
        low, _ = demo.render(RW.W, RW.H, 7, 1, 0, n, threads=4)
        assert (low["x"] == got["x"]).mean() < 0.01 and (low["wavelength"] == got["wavelength"]).mean() < 0.01


class _Spy:
    """The oracle library with the RNG coordinates of every call kept."""

    def __init__(self, lib):
        self._lib, self.blocks = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        at = {"oracle_material_bounce": 9, "oracle_rng_block": 3}.get(name)
        if at is None and name != "oracle_rng_blocks":
            return fn

        def call(*a):
            if at is not None:
                self.blocks.append(int(a[at]))
            else:
                self.blocks += C.cast(a[3], C.POINTER(C.c_uint32))[:int(a[5])]
            return fn(*a)
        return call


def test_step_and_light_oracles_form_their_blocks_as_32_bit_sums(monkeypatch):
    """`segments` at the edges of 32 bits: StepOracle.step_one draws block (2 + segments) mod 2^32 and stores segments + 1
    mod 2^32; _light_oracle.draw draws block (2^31 + segments) mod 2^32.  Neither raises."""
    objs, cam = closed_scene(False)
    so = S.StepOracle(objs, cam)
    spy = _Spy(O.lib())
    monkeypatch.setattr(O, "_lib", spy)
    seed, stream = 0xA5A5A5A500000007, 0xFFFFFFFF
    for segments in RW.SEGMENT_EDGES:
        st, _ = vertex_states(1, first=(1 << 63) + 5)
        st = st.view(S.STATE_DTYPE)
        st["origin"], st["direction"], st["segments"] = (0, 0, 1), (0, 0, -1), segments       # down onto the diffuse floor
        hit = np.zeros(1, S.HIT_DTYPE)
        spy.blocks.clear()
        so.step_one(st[0:1].reshape(()), hit[0:1].reshape(()), seed, stream)
        assert int(hit["object"][0]) == 0 and int(st["segments"][0]) == (segments + 1) & M32, segments
        assert spy.blocks and set(spy.blocks) == {(2 + segments) & M32}, (segments, spy.blocks)
    assert (0xFFFFFFFF + 1) & M32 == 0
    edges = np.array([s for s in RW.SEGMENT_EDGES if s >= 1], np.uint32)
    st, ht = vertex_states(len(edges), first=(1 << 64) - 2 - len(edges))
    st["segments"] = edges
    spy.blocks.clear()
    out, _ = LO.draw(objs, st.view(S.STATE_DTYPE), ht, seed, stream)
    assert (out["status"] != LO.SKIPPED).all()
    assert spy.blocks == [((1 << 31) + int(s)) & M32 for s in edges], spy.blocks
    # the draw is that block's: the emitter it picks is word 2 of the numpy Philox at it
    words = np.concatenate([RW.numpy_words(seed, stream, st["path_index"][i:i + 1], ((1 << 31) + int(s)) & M32) for i, s in enumerate(edges)])
    em = LO.emitters(objs.view(O.OBJECT_DTYPE))
    assert out["emitter"].tolist() == em[(words[:, 2].astype(np.uint64) * np.uint64(len(em))) >> np.uint64(32)].tolist()
