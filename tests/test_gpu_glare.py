"""The glare unit on the GPU: rl_glare_unit_apply against the numpy restatement (tests/_glare_oracle.py) bit for bit at the
smallest shapes that can break a tiled kernel, on clean and on poisoned LDS, into a prefilled dst; impulses at every corner and
edge; K = 1 against the projection; ordering; the argument checks; the resources; and the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import _glare_cases as GC
import _glare_oracle as GO
import _guarded as G
import _lds_poison as LP
from _glare_cases import same_bits

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402
from robigo_luculenta_amd import __main__ as CLI  # noqa: E402

RL_E_INVALID, RL_E_STATE = -1, -5


def _err():
    return _lib.lib.rl_last_error()


def _prefill(dst, tmp_path):
    """dst's tristimulus and compensation buffers all 0xAA: a pixel the kernel leaves out, and a compensation the call does not
    zero, both show.  (A gather unit owns its buffers: the guards of _guarded.py cannot be put round them, so its FILL is put in
    them, and the neighbours of every output are outputs that are compared as well.)"""
    path = str(tmp_path / "aa.raw")
    n = dst.width * dst.height
    with open(path, "wb") as f:
        f.write(bytes([G.FILL]) * (n * 24))
    dst.load(path)
    assert dst._download()[0].tobytes() == bytes([G.FILL]) * (n * 12)


def _apply_checked(unit, spectral, film, tables, matrix, dst, what):
    before = R.glare_launches()
    assert unit.apply(spectral, matrix, dst) is dst
    assert R.glare_launches() == before + 1
    got, comp = dst._download()
    want = GO.apply(film, tables, matrix).reshape(-1, 3)
    G.assert_written_as(np.ascontiguousarray(got).reshape(-1, 3), want, what)
    assert comp.tobytes() == bytes(comp.nbytes), what
    return got


@pytest.mark.parametrize("shape", GC.SHAPES, ids=GC.shape_id)
def test_apply_matches_the_oracle_bit_for_bit_into_a_prefilled_dst(shape, tmp_path):
    w, h, n_nodes, taps = shape
    spectral, unit, dst = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps), R.GatherUnit(w, h)
    film, tables, matrix = GC.film(w, h, n_nodes), GC.tables(n_nodes, taps), GC.matrix(n_nodes)
    spectral.upload(film)
    unit.set_kernels(tables)
    _prefill(dst, tmp_path)
    _apply_checked(unit, spectral, film, tables, matrix, dst, "apply %s" % GC.shape_id(shape))
    assert unit.launch_ms() > 0.0
    assert same_bits(spectral.download(), film)       # the film is left as it was
    # the same bits on a second run
    first = dst._download()[0].copy()
    unit.apply(spectral, matrix, dst)
    assert dst._download()[0].tobytes() == first.tobytes()


@pytest.mark.parametrize("pattern", LP.PATTERNS[:2], ids=lambda p: "%08x" % p)
@pytest.mark.parametrize("shape", GC.SHAPES, ids=GC.shape_id)
def test_apply_on_poisoned_lds(shape, pattern, tmp_path):
    w, h, n_nodes, taps = shape
    spectral, unit, dst = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps), R.GatherUnit(w, h)
    film, tables, matrix = GC.film(w, h, n_nodes, salt=1), GC.tables(n_nodes, taps, salt=1), GC.matrix(n_nodes, salt=1)
    spectral.upload(film)
    unit.set_kernels(tables)
    _prefill(dst, tmp_path)
    LP.poison_lds(pattern)
    _apply_checked(unit, spectral, film, tables, matrix, dst, "apply %s on LDS full of %08x" % (GC.shape_id(shape), pattern))


@pytest.mark.parametrize("shape", [(5, 3, 2, 9), (67, 19, 3, 9), (40, 1, 3, 3), (40, 40, 2, 65)], ids=GC.shape_id)
def test_a_table_that_is_not_finite_takes_the_exact_skip_and_matches_the_oracle(shape, tmp_path):
    """A NaN or an infinity in a table times a +0 staged outside the film is a NaN the contract never makes: the library then
    launches the form of the kernel that skips the tap.  Pixels the entry reaches inside the film are NaN or infinite in the
    oracle too; every other pixel holds the oracle's bits."""
    w, h, n_nodes, taps = shape
    spectral, unit, dst = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps), R.GatherUnit(w, h)
    film, tables, matrix = np.abs(GC.film(w, h, n_nodes, salt=2)) + np.float32(1.0), GC.tables(n_nodes, taps, salt=2), GC.matrix(n_nodes, salt=2)
    tables[0, 0, 0], tables[n_nodes - 1, taps - 1, taps - 1] = np.nan, -np.inf      # reach (x >= R, y >= R) and (x < w - R, y < h - R)
    spectral.upload(film)
    unit.set_kernels(tables)
    _prefill(dst, tmp_path)
    unit.apply(spectral, matrix, dst)
    got, comp = dst._download()
    got, want = np.ascontiguousarray(got).reshape(h, w, 3), GO.apply(film, tables, matrix)
    finite = np.isfinite(want)
    assert finite.any(), (finite.sum(), finite.size)       # the skip shows: with t * 0 for a tap outside the film no pixel would be finite
    assert same_bits(got[finite], want[finite]) and (np.isnan(got) == np.isnan(want)).all() and (got[np.isinf(want)] == want[np.isinf(want)]).all()
    assert not comp.any()
    # finite tables again: the fast form, the oracle's bits everywhere
    tables = GC.tables(n_nodes, taps, salt=3)
    unit.set_kernels(tables)
    _apply_checked(unit, spectral, film, tables, matrix, dst, "finite tables after the others")


def test_an_impulse_in_each_corner_on_each_edge_and_in_the_interior(tmp_path):
    w, h, n_nodes, taps = 20, 12, 2, 9
    spectral, unit, dst = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps), R.GatherUnit(w, h)
    tables = np.stack([GC.asymmetric_psf(taps), GC.asymmetric_psf(taps).T * np.float32(-0.5)])
    matrix = GC.matrix(n_nodes)
    unit.set_kernels(tables)
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2), (w // 2, h // 2), (3, 2)):
        film = np.zeros((n_nodes, h, w), np.float32)
        film[0, y, x], film[1, y, x] = 1.0, 3.0
        spectral.upload(film)
        _prefill(dst, tmp_path)
        got = _apply_checked(unit, spectral, film, tables, matrix, dst, "impulse at (%d, %d)" % (x, y)).reshape(h, w, 3)
        # the response is the table point-flipped about the impulse, cut by the frame: pixel p gathers the impulse through entry q - p + R
        py, px = np.nonzero(got[:, :, 0])
        assert px.min() == max(0, x - 4) and px.max() == min(w - 1, x + 4) and py.min() == max(0, y - 4) and py.max() == min(h - 1, y + 4)


def test_one_tap_of_one_is_the_projection_on_a_rendered_film():
    w, h, n_nodes, n = 64, 36, 16, 1 << 16
    scene = R.Scene.builtin(R.SCENE_DEMO)
    trace = R.TraceUnit(0, w, h, n_photons=n)
    trace.render(scene, seed=1, stream=0, first_path_index=0)
    spectral, unit, a, b = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, 1), R.GatherUnit(w, h), R.GatherUnit(w, h)
    spectral.plot([trace])
    unit.set_kernels(np.ones((n_nodes, 1, 1), np.float32))
    observer = R.spectral_observer_cie1931(n_nodes)
    glared, projected = unit.apply(spectral, observer, a)._download()[0], spectral.project(observer, b)._download()[0]
    assert projected.any() and glared.tobytes() == projected.tobytes()


def test_apply_sees_what_is_queued_before_it_and_overwrites_what_is_queued_on_dst():
    w, h, n_nodes, taps = 64, 36, 5, 9
    spectral, unit, dst = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps), R.GatherUnit(w, h)
    matrix = GC.matrix(n_nodes)
    photons = np.zeros(4096, R.PHOTON_DTYPE)
    g = np.random.default_rng(5)
    photons["x"], photons["y"] = g.uniform(-1, 1, 4096), g.uniform(-1, 1, 4096) * h / w
    photons["probability"], photons["wavelength"] = g.uniform(0, 1, 4096), g.uniform(380, 780, 4096)
    plot = R.PlotUnit(0, w, h)
    plot.upload(np.full((h, w, 3), 7.0, np.float32))
    first, second = GC.tables(n_nodes, taps, salt=4), GC.tables(n_nodes, taps, salt=5)
    unit.set_kernels(first)
    unit.set_kernels(second)                       # set twice: the second holds
    spectral.clear()                               # (queued on the film)
    spectral.plot_photons(photons)
    dst.accumulate(plot)                           # queued on dst's stream immediately before: a film of 7s, which apply must come after
    unit.apply(spectral, matrix, dst)
    got, comp = dst._download()
    film = spectral.download()
    assert film.any() and same_bits(got.reshape(-1, 3), GO.apply(film, second, matrix).reshape(-1, 3)) and not comp.any()
    assert not same_bits(got.reshape(-1, 3), GO.apply(film, first, matrix).reshape(-1, 3))
    # a clear queued on the film immediately before the apply is seen too
    spectral.clear()
    unit.apply(spectral, matrix, dst)
    assert dst._download()[0].tobytes() == bytes(w * h * 12)


def test_every_argument_failure_in_the_documented_order():
    w, h, n_nodes, taps = 9, 8, 5, 3
    L = _lib.lib
    spectral, unit = R.SpectralUnit(w, h, n_nodes), R.GlareUnit(w, h, n_nodes, taps)
    film = GC.film(w, h, n_nodes)
    spectral.upload(film)
    matrix, tables = GC.matrix(n_nodes), GC.tables(n_nodes, taps)
    M, T = matrix.ctypes.data_as(C.c_void_p), tables.ctypes.data_as(C.c_void_p)

    def marked(w_, h_):
        plot, gather = R.PlotUnit(0, w_, h_), R.GatherUnit(w_, h_)
        plot.upload(np.full((h_, w_, 3), 3.5, np.float32))
        gather.accumulate(plot)
        return gather

    def untouched(gather):
        t, c = gather._download()
        return (t == 3.5).all() and not c.any()
    dst = marked(w, h)
    launches = R.glare_launches()
    for args in ((None, None, None, None), (None, spectral.handle, M, dst.handle), (unit.handle, None, M, dst.handle),
                 (unit.handle, spectral.handle, None, dst.handle), (unit.handle, spectral.handle, M, None)):
        assert L.rl_glare_unit_apply(*args) == RL_E_INVALID and b"null" in _err()
    # no tables yet: RL_E_STATE, after the nulls and before the film and the dst
    wrong_film, wrong_dst = R.SpectralUnit(w + 1, h, n_nodes), marked(w, h + 1)
    assert L.rl_glare_unit_apply(unit.handle, wrong_film.handle, None, wrong_dst.handle) == RL_E_INVALID
    assert L.rl_glare_unit_apply(unit.handle, wrong_film.handle, M, wrong_dst.handle) == RL_E_STATE and b"has no tables" in _err()
    assert L.rl_glare_unit_apply(unit.handle, spectral.handle, M, dst.handle) == RL_E_STATE and b"has no tables" in _err()
    assert L.rl_glare_unit_set_kernels(unit.handle, None) == RL_E_INVALID and L.rl_glare_unit_set_kernels(None, T) == RL_E_INVALID
    assert L.rl_glare_unit_apply(unit.handle, spectral.handle, M, dst.handle) == RL_E_STATE                  # a refused set gives no tables
    unit.set_kernels(tables)
    # a film of another size or node count: RL_E_STATE before the dst is looked at
    for other in (wrong_film, R.SpectralUnit(w, h + 1, n_nodes), R.SpectralUnit(h, w, n_nodes), R.SpectralUnit(w, h, n_nodes + 1)):
        for d in (dst, wrong_dst):
            assert L.rl_glare_unit_apply(unit.handle, other.handle, M, d.handle) == RL_E_STATE and b"spectral unit does not match" in _err()
    for other in (wrong_dst, marked(w + 1, h), marked(h, w)):
        assert L.rl_glare_unit_apply(unit.handle, spectral.handle, M, other.handle) == RL_E_STATE and b"gather unit does not match" in _err()
        assert untouched(other)
    if R.device_count() > 1:
        assert L.rl_glare_unit_apply(unit.handle, R.SpectralUnit(w, h, n_nodes, device=1).handle, M, dst.handle) == RL_E_STATE
        assert L.rl_glare_unit_apply(unit.handle, spectral.handle, M, R.GatherUnit(w, h, device=1).handle) == RL_E_STATE
    assert untouched(dst) and untouched(wrong_dst) and R.glare_launches() == launches
    assert same_bits(spectral.download(), film)
    # create: the order of its checks, and the limits themselves
    for args, word in (((0, 4, 81, 9), "zero"), ((4, 0, 1, 2), "zero"), ((4, 4, 1, 2), "n_nodes"), ((65536, 65536, 402, 9), "n_nodes"),
                       ((65536, 65536, 2, 2), "taps"), ((4, 4, 2, 67), "taps"), ((4, 4, 2, 0), "taps"), ((65536, 65536, 2, 9), "RL_MAX_PIXELS")):
        with pytest.raises(R.RlError) as e:
            R.GlareUnit(*args)
        assert e.value.code == RL_E_INVALID and word in str(e.value), (args, str(e.value))
    with pytest.raises(R.RlError) as e:
        R.GlareUnit(4, 4, 3, 3, device=R.device_count())
    assert e.value.code == RL_E_INVALID
    # ... and after all that the unit works
    unit.apply(spectral, matrix, dst)
    assert same_bits(dst._download()[0].reshape(-1, 3), GO.apply(film, tables, matrix).reshape(-1, 3))


def test_a_unit_gives_back_what_it_took():
    R.GatherUnit(4, 4).close()
    before = R.live_resources()
    unit = R.GlareUnit(16, 9, 5, 9)
    assert R.live_resources() != before
    unit.set_kernels(GC.tables(5, 9))
    spectral, dst = R.SpectralUnit(16, 9, 5), R.GatherUnit(16, 9)
    unit.apply(spectral, GC.matrix(5), dst)
    unit.set_kernels(GC.tables(5, 9, salt=1))
    for u in (unit, spectral, dst):
        u.close()
    assert R.live_resources() == before


def test_the_command_line_writes_an_image_and_the_glare_keeps_the_light_it_moves(tmp_path):
    """Every table sums to 1, so a pixel's light is moved, not made: what leaves the output is exactly what the tables carry across
    the frame's edge.  The XYZ totals of the glared image are therefore those of the film weighted, pixel by pixel, by the share of
    its table that stays inside the frame -- the un-glared projection's total wherever the table fits, and never more than it --
    within the sum over the pixels of the rounding bound of apply (tests/_glare_oracle.py) plus the tables' own K^2 2^-24."""
    out, glared = str(tmp_path / "image.png"), str(tmp_path / "glare.png")
    argv = ["--glare", glared, "--glare-strength", "0.3", "--glare-taps", "9", "--spectral-nodes", "16", "--output", out, "--width", "64",
            "--height", "36", "--batches", "1", "--photons-per-batch", "65536", "--quiet"]
    CLI.main(argv)
    assert os.path.getsize(glared) > 100 and open(glared, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    # the same steps once more with the film in hand
    a = CLI.parse_args(argv)
    spectral = CLI.spectral_film(a)
    got = CLI.render_glare(a, spectral).tristimulus_buffer.astype(np.float64).reshape(36, 64, 3)
    film, observer = spectral.download().astype(np.float64), R.spectral_observer_cie1931(16).astype(np.float64)
    plain = spectral.project(R.spectral_observer_cie1931(16), R.GatherUnit(64, 36)).tristimulus_buffer.astype(np.float64).reshape(36, 64, 3)
    side = 2 * 9 - 1
    tables = R.glare_kernels_scaled(R.glare_psf_veil(side, 2.0), 550.0, 16, 0.3, 9).astype(np.float64)
    kept = np.zeros_like(film)          # per node and source pixel q: the sum of the entries through which a pixel inside the frame gathers q
    ones = np.ones((36, 64))
    for b in range(16):
        kept[b] = GO._correlate_f64(ones, tables[b][::-1, ::-1])
    want = np.einsum("bhw,bc->c", film * kept, observer)
    scale = np.einsum("bhw,bc->c", np.abs(film) * kept, np.abs(observer))
    bound = GO.bound(scale, 9, 16) + 81 * GO.U * scale
    total, plain_total = got.sum(axis=(0, 1)), plain.sum(axis=(0, 1))
    print("XYZ totals: glared %s, expected %s, un-glared %s; difference %s of the bound" % (total, want, plain_total, np.abs(total - want) / bound))
    assert (plain_total > 0).all() and (np.abs(total - want) <= bound).all()
    assert (total <= plain_total * (1 + 1e-5)).all() and (total >= 0.9 * plain_total).all()
    inner = kept[:, 4:-4, 4:-4]
    assert (np.abs(inner - 1.0) <= 81 * GO.U).all()                      # where the table fits, all of a pixel's light stays
