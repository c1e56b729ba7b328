"""The glare unit without a GPU: the numpy restatement (tests/_glare_oracle.py) against an f64 evaluation within the derived
rounding bound; the two host helpers against the restatement bit for bit; what the tables mean (they sum to 1, a base function is
point-flipped, the fringe of a white impulse is red outside); every argument check that comes before the device, in the header's
order; the mirrors of the ABI; the command line's options; and the compiled kernel's resources and instructions (hipcc
cross-compiles here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _device_build
import _glare_cases as GC
import _glare_oracle as GO
import _spectral_oracle as SO
from _device_build import kernels  # noqa: F401  (kernels is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import robigo_luculenta_amd as R  # noqa: E402  (a missing HIP library is a failure, never a skip)
from robigo_luculenta_amd import _lib  # noqa: E402
from robigo_luculenta_amd import __main__ as CLI  # noqa: E402

lib = _lib.lib
RL_E_INVALID, RL_E_NO_DEVICE, RL_E_STATE = -1, -2, -5
POISON = 0xDEAD0
TAPS, NODES, LAMBDA0S, STRENGTHS = (1, 3, 9, 65), (2, 16, 81), (380.0, 550.0, 780.0), (0.0, 0.25, 1.0)


def last():
    return lib.rl_last_error().decode()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 2, 1), (5, 3, 2, 9), (23, 17, 5, 9), (40, 7, 16, 3), (9, 9, 2, 65)], ids=GC.shape_id)
def test_the_oracle_is_the_f64_sum_within_the_rounding_bound_of_the_two_level_sum(shape):
    w, h, n_nodes, taps = shape
    film, tables, matrix = GC.random_film(w, h, n_nodes), GC.tables(n_nodes, taps), GC.matrix(n_nodes)
    got = GO.apply(film, tables, matrix).astype(np.float64)
    want, scale = GO.apply_f64(film, tables, matrix)
    bound = GO.bound(scale, taps, n_nodes)
    d = np.abs(got - want)
    on = scale > 0
    print("largest error %.3f of the bound (2 K + n_nodes + 3 = %d roundings of 2^-24)" % ((d[on] / bound[on]).max(), 2 * taps + n_nodes + 3))
    assert on.all() and (d <= bound).all()


def test_the_oracle_skips_a_tap_outside_the_film_and_with_a_delta_it_is_the_projection():
    # a NaN in the table reaches exactly the pixels whose tap lies inside the film: skipping is not adding t * 0
    film, matrix = np.ones((2, 3, 4), np.float32), np.ones((2, 3), np.float32)
    tables = np.zeros((2, 3, 3), np.float32)
    tables[:, 1, 1] = 1.0
    tables[0, 0, 0] = np.nan                               # weighs (x - 1, y - 1)
    got = GO.apply(film, tables, matrix)
    assert np.isnan(got[1:, 1:]).all() and (got[0] == 2.0).all() and (got[:, 0] == 2.0).all()
    # K = 1, every entry 1.0f: the bits of the projection
    for w, h, n_nodes in ((7, 5, 3), (1, 1, 2), (16, 4, 16)):
        film, matrix = GC.film(w, h, n_nodes), GC.matrix(n_nodes)
        assert GC.same_bits(GO.apply(film, np.ones((n_nodes, 1, 1), np.float32), matrix).reshape(-1, 3), SO.project(film, matrix).reshape(-1, 3))


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("taps", TAPS)
def test_the_veil_is_the_restatement_bit_for_bit(taps):
    for r0 in (0.5, 1.0, 2.0, 3.7, 1e-3, 1e6):
        got = R.glare_psf_veil(taps, r0)
        assert got.shape == (taps, taps) and GC.same_bits(got, GO.psf_veil(taps, r0)), (taps, r0)
        assert got[taps // 2, taps // 2] == 1.0 and (got > 0).all() and GC.same_bits(got, got.T) and GC.same_bits(got, got[::-1, ::-1])


@pytest.mark.parametrize("n_nodes", NODES)
@pytest.mark.parametrize("taps", TAPS)
def test_the_scaled_tables_are_the_restatement_bit_for_bit_and_each_sums_to_one(taps, n_nodes):
    """Two base functions: the library's veil on as many samples as the tables have, and an asymmetric one twice as wide."""
    bases = [R.glare_psf_veil(taps, 2.0), GC.asymmetric_psf(min(2 * taps - 1, 257))]
    for psf in bases:
        for lambda0 in LAMBDA0S:
            for strength in STRENGTHS:
                got = R.glare_kernels_scaled(psf, lambda0, n_nodes, strength, taps)
                want = GO.kernels_scaled(psf, lambda0, n_nodes, strength, taps)
                assert got.shape == (n_nodes, taps, taps) and GC.same_bits(got, want), (len(psf), lambda0, strength)
                sums = got.astype(np.float64).reshape(n_nodes, -1).sum(axis=1)
                assert (np.abs(sums - 1.0) <= taps * taps * GO.U).all(), (len(psf), lambda0, strength, np.abs(sums - 1.0).max())
                if strength == 0.0:        # a delta: apply is then the projection
                    delta = np.zeros((taps, taps), np.float32)
                    delta[taps // 2, taps // 2] = 1.0
                    assert all(GC.same_bits(t, delta) for t in got)
    film, matrix = GC.film(9, 6, n_nodes), GC.matrix(n_nodes)
    delta = R.glare_kernels_scaled(bases[0], 550.0, n_nodes, 0.0, taps)
    if taps <= 9:
        assert GC.same_bits(GO.apply(film, delta, matrix).reshape(-1, 3), SO.project(film, matrix).reshape(-1, 3))


def test_an_asymmetric_base_function_comes_out_point_flipped_at_its_own_wavelength():
    """Node 0 of any film sits at 380 nm: with lambda0 = 380 its s is exactly 1, u = 2 R - i is an integer, the interpolation
    weights are 1 and 0, and the table is the base function turned by 180 degrees over its sum -- a gather table whose impulse
    response is the base function unflipped."""
    for taps in (3, 9, 33):
        psf = GC.asymmetric_psf(taps)
        assert not GC.same_bits(psf, psf[::-1, ::-1]) and not GC.same_bits(psf, psf[::-1]) and not GC.same_bits(psf, psf[:, ::-1])
        got = R.glare_kernels_scaled(psf, 380.0, 2, 1.0, taps)[0]
        flipped = psf[::-1, ::-1].astype(np.float64)
        want = (flipped / GO._sequential_sum(flipped)).astype(np.float32)
        assert GC.same_bits(got, want)
        # the impulse response: an impulse at q gives the base function centred on q, unflipped
        film = np.zeros((2, taps, taps), np.float32)
        film[0, taps // 2, taps // 2] = 1.0
        matrix = np.zeros((2, 3), np.float32)
        matrix[0] = 1.0
        tables = np.stack([got, got])
        response = GO.apply(film, tables, matrix)[:, :, 0]
        assert GC.same_bits(response, (psf.astype(np.float64) / GO._sequential_sum(flipped)).astype(np.float32))


def test_the_halo_of_a_white_impulse_is_red_outside_and_blue_inside():
    """Every node 1.0 at one pixel, the veil scaled by wavelength from 550 nm, the CIE observer: along the row through the
    impulse Z / X falls strictly from radius 2 to radius R.  An XYZ-space blur keeps Z / X constant: it cannot produce this.
    r0 is a quarter of R: far beyond r0 the veil is the power law d^-3, whose scaled copies differ by a constant factor only --
    there the fringe has saturated and Z / X is level, its last digits the bilinear resampling's, not the wavelength's."""
    n_nodes, taps, r0 = 16, 33, 4.0
    R_ = taps // 2
    psf = R.glare_psf_veil(65, r0)
    tables = R.glare_kernels_scaled(psf, 550.0, n_nodes, 1.0, taps)
    film = np.zeros((n_nodes, 1, 2 * R_ + 1), np.float32)
    film[:, 0, R_] = 1.0
    out = GO.apply(film, tables, R.spectral_observer_cie1931(n_nodes)).astype(np.float64)[0]
    for side in (1, -1):
        ratio = np.array([out[R_ + side * d, 2] / out[R_ + side * d, 0] for d in range(2, R_ + 1)])
        print("Z / X at radius 2 .. %d: %s" % (R_, " ".join("%.4f" % v for v in ratio)))
        assert (out[:, 0] > 0).all() and (np.diff(ratio) < 0).all()
    # ... and one table for every node does keep it constant, up to rounding
    same = np.repeat(tables[8:9], n_nodes, axis=0)
    flat = GO.apply(film, same, R.spectral_observer_cie1931(n_nodes)).astype(np.float64)[0]
    ratio = flat[:, 2] / flat[:, 0]
    assert np.ptp(ratio) <= 1e-5 * ratio.mean()


def test_the_helpers_refuse_what_the_header_says_and_write_nothing():
    out = np.full(81 * 9 * 9, 7.0, np.float32)
    P = out.ctypes.data_as(C.c_void_p)
    veil = lib.rl_glare_psf_veil
    assert veil(9, 2.0, None) == RL_E_INVALID and "null output" in last()
    for taps in (0, 2, 64, 66, 67, 0xFFFFFFFF):
        assert veil(taps, 2.0, P) == RL_E_INVALID and "taps %d is not odd and in 1 .. RL_GLARE_MAX_TAPS = 65" % taps in last()
        assert veil(taps, float("nan"), P) == RL_E_INVALID and "taps" in last()                 # the taps before r0
    for r0 in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert veil(9, r0, P) == RL_E_INVALID and "r0" in last()
    assert veil(65, 2.0, np.zeros(65 * 65, np.float32).ctypes.data_as(C.c_void_p)) == 0
    psf = np.ones((3, 3), np.float32)
    S = psf.ctypes.data_as(C.c_void_p)
    scaled = lib.rl_glare_kernels_scaled
    assert scaled(None, 3, 550.0, 81, 0.5, 9, P) == RL_E_INVALID and scaled(S, 3, 550.0, 81, 0.5, 9, None) == RL_E_INVALID
    for psf_taps in (0, 2, 258, 259, 0xFFFFFFFF):
        assert scaled(S, psf_taps, 550.0, 81, 0.5, 9, P) == RL_E_INVALID and "psf_taps" in last()
    for lambda0 in (0.0, -550.0, float("nan"), float("inf")):
        assert scaled(S, 3, lambda0, 81, 0.5, 9, P) == RL_E_INVALID and "lambda0" in last()
    for n_nodes in (0, 1, 402):
        assert scaled(S, 3, 550.0, n_nodes, 0.5, 9, P) == RL_E_INVALID and "n_nodes" in last()
    for strength in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert scaled(S, 3, 550.0, 81, strength, 9, P) == RL_E_INVALID and "strength" in last()
    for taps in (0, 2, 66, 67):
        assert scaled(S, 3, 550.0, 81, 0.5, taps, P) == RL_E_INVALID and "taps" in last()
    for bad in (-1.0, float("nan"), float("inf"), -0.5):
        entry = psf.copy()
        entry[1, 2] = bad
        assert scaled(entry.ctypes.data_as(C.c_void_p), 3, 550.0, 81, 0.5, 9, P) == RL_E_INVALID and "psf entry 5" in last()
    # a function that gives a node nothing: all zero; and one whose only sample the longest wavelengths push off a 1-tap table's centre
    zero = np.zeros((3, 3), np.float32)
    assert scaled(zero.ctypes.data_as(C.c_void_p), 3, 550.0, 81, 0.5, 9, P) == RL_E_INVALID and "gives node 0 nothing" in last()
    corner = np.zeros((3, 3), np.float32)
    corner[0, 0] = 1.0
    assert scaled(corner.ctypes.data_as(C.c_void_p), 3, 550.0, 2, 0.5, 1, P) == RL_E_INVALID and "gives node 0 nothing" in last()
    assert GO.kernels_scaled(corner, 550.0, 2, 0.5, 1) is None
    assert (out == 7.0).all()                                                                     # nothing was written by any of them
    with pytest.raises(ValueError):
        R.glare_kernels_scaled(np.ones((3, 5), np.float32), 550.0, 81, 0.5, 9)


# ---- the checks that come before the device -------------------------------------------------------------------------------------------

def test_create_checks_its_arguments_in_order_before_the_device():
    """Null output, zero size, the node count, the taps, pixels x nodes, and only then the device; the handle is left null."""
    def create(w, h, nodes, taps, out):
        return lib.rl_glare_unit_create(0, w, h, nodes, taps, out)

    def refused(w, h, nodes, taps, message):
        handle = C.c_void_p(POISON)
        assert create(w, h, nodes, taps, C.byref(handle)) == RL_E_INVALID, (message, w, h, nodes, taps, last())
        assert message in last() and handle.value is None, (message, w, h, nodes, taps, last(), handle.value)

    for args in ((4, 4, 81, 9), (0, 0, 81, 9), (4, 4, 1, 9), (4, 4, 81, 2), (65536, 65536, 81, 9)):   # the null output comes first
        assert create(*args, None) == RL_E_INVALID and last() == "null output handle"
    for nodes, taps in ((81, 9), (1, 9), (81, 2), (0, 0)):                                            # ... then the zero size
        for w, h in [(0, 4), (4, 0), (0, 0), (0, 0xFFFFFFFF)]:
            refused(w, h, nodes, taps, "zero-sized glare unit")
    for nodes in (0, 1, 402, 0xFFFFFFFF):                                                             # ... then the node count
        for taps, (w, h) in ((9, (4, 4)), (0, (4, 4)), (66, (65536, 65536))):
            refused(w, h, nodes, taps, "glare unit: n_nodes %d outside 2 .. RL_SPECTRAL_MAX_NODES = 401" % nodes)
    for taps in (0, 2, 64, 66, 67, 255, 0xFFFFFFFF):                                                  # ... then the taps
        for w, h in ((4, 4), (65536, 65536)):
            refused(w, h, 81, taps, "glare unit: taps %d is not odd and in 1 .. RL_GLARE_MAX_TAPS = 65" % taps)
    for w, h, nodes in [(46341, 46341, 2), (4096, 4096, 128), (65536, 128, 256), (0xFFFFFFFF, 0xFFFFFFFF, 401), (1 << 23, 1, 256), (65536, 32768, 2)]:         # ... then the size, in 64 bits
        refused(w, h, nodes, 65, "glare unit: %d x %d pixels x %d nodes exceed RL_MAX_PIXELS = 2^31 - 1" % (w, h, nodes))
    if R.device_count() == 0:                                                                         # what comes next is the device
        for nodes, taps in ((2, 1), (81, 33), (401, 65)):
            handle = C.c_void_p(POISON)
            assert create(4, 4, nodes, taps, C.byref(handle)) == RL_E_NO_DEVICE and handle.value is None, last()
        with pytest.raises(R.RlError) as e:
            R.GlareUnit(64, 36, 16, 9)
        assert e.value.code == RL_E_NO_DEVICE


class _Glare(C.Structure):
    """The first fields of a glare unit's handle, as the checks that come before any device work read them."""
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("n_nodes", C.c_uint32), ("taps", C.c_uint32),
                ("has_tables", C.c_uint32), ("rest", C.c_uint8 * 512)]


class _Spectral(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("n_nodes", C.c_uint32), ("rest", C.c_uint8 * 512)]


class _Gather(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_uint32), ("height", C.c_uint32), ("rest", C.c_uint8 * 512)]


def test_apply_checks_a_stand_in_handle_in_the_stated_order():
    """Nulls (RL_E_INVALID), no tables, the film, the dst (RL_E_STATE): all before any device work, on stand-ins for the handles."""
    unit = _Glare(0, 8, 6, 5, 9, 0)
    film, dst = _Spectral(0, 8, 6, 5), _Gather(0, 8, 6)
    matrix = np.zeros((5, 3), np.float32)
    M = matrix.ctypes.data_as(C.c_void_p)
    apply = lib.rl_glare_unit_apply
    U, F, D = C.byref(unit), C.byref(film), C.byref(dst)
    assert lib.rl_glare_unit_destroy(None) == 0
    for u, t in ((None, M), (U, None), (None, None)):
        assert lib.rl_glare_unit_set_kernels(u, t) == RL_E_INVALID and "null glare unit or tables" in last()
    for args in ((None, F, M, D), (U, None, M, D), (U, F, None, D), (U, F, M, None), (None, None, None, None)):
        assert apply(*args) == RL_E_INVALID and "null glare unit, film, matrix or dst" in last()
    wrong_film, wrong_dst = C.byref(_Spectral(0, 9, 6, 5)), C.byref(_Gather(0, 8, 7))
    assert apply(U, wrong_film, M, wrong_dst) == RL_E_STATE and "has no tables" in last()                 # no tables: before the film
    unit.has_tables = 1
    for other in (_Spectral(0, 9, 6, 5), _Spectral(0, 8, 7, 5), _Spectral(1, 8, 6, 5), _Spectral(0, 6, 8, 5)):
        assert apply(U, C.byref(other), M, wrong_dst) == RL_E_STATE and "spectral unit does not match the glare unit" in last()
    assert apply(U, C.byref(_Spectral(0, 8, 6, 4)), M, wrong_dst) == RL_E_STATE and "4 nodes against 5" in last()
    for other in (_Gather(0, 9, 6), _Gather(0, 8, 7), _Gather(1, 8, 6)):                                  # the film before the dst
        assert apply(U, F, M, C.byref(other)) == RL_E_STATE and "gather unit does not match the glare unit" in last()
    assert lib.rl_debug_glare_ms(None, None) == RL_E_INVALID and lib.rl_debug_glare_launches(None) == RL_E_INVALID


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------

def test_constants_and_entry_points_are_in_every_mirror():
    assert _lib.RL_GLARE_MAX_TAPS == 65 == R.RL_GLARE_MAX_TAPS
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert re.search(r"#define RL_GLARE_MAX_TAPS 65\b", header) and "pub const RL_GLARE_MAX_TAPS: u32 = 65;" in rust
    vp, u32, i, d = C.c_void_p, C.c_uint32, C.c_int, C.c_double
    S = _lib.SIGNATURES
    assert S["rl_glare_unit_create"] == (i, [i, u32, u32, u32, u32, C.POINTER(C.c_void_p)])       # device, width, height, nodes, taps, out
    assert S["rl_glare_unit_destroy"] == (i, [vp]) and S["rl_glare_unit_set_kernels"] == (i, [vp, vp])
    assert S["rl_glare_unit_apply"] == (i, [vp, vp, vp, vp])                                      # unit, film, matrix, dst
    assert S["rl_glare_psf_veil"] == (i, [u32, d, vp])
    assert S["rl_glare_kernels_scaled"] == (i, [vp, u32, d, u32, d, u32, vp])                     # psf, psf_taps, lambda0, nodes, strength, taps, out
    for name in ("rl_glare_unit_create", "rl_glare_unit_destroy", "rl_glare_unit_set_kernels", "rl_glare_unit_apply", "rl_glare_psf_veil",
                 "rl_glare_kernels_scaled"):
        assert re.search(r"\bint %s\(" % name, header) and "pub fn %s(" % name in rust and hasattr(lib, name), name
    assert "typedef struct RlGlareUnit RlGlareUnit;" in header and "pub enum RlGlareUnit {}" in rust
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    assert _lib.DEBUG_SIGNATURES["rl_debug_glare_launches"] == (i, [vp]) and _lib.DEBUG_SIGNATURES["rl_debug_glare_ms"] == (i, [vp, vp])
    assert "int rl_debug_glare_launches(uint64_t* out);" in debug and "rl_debug_glare" not in header and "rl_debug_glare" not in rust
    before = R.glare_launches()
    assert isinstance(before, int) and before >= 0
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_glare.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    for name in ("set_kernels", "apply", "launch_ms"):
        assert callable(getattr(R.GlareUnit, name))
    assert callable(R.glare_psf_veil) and callable(R.glare_kernels_scaled) and callable(R.glare_launches)


# ---- the command line -------------------------------------------------------------------------------------------------------------------

def test_the_command_line_takes_glare_and_refuses_it_with_direct(capsys):
    a = CLI.parse_args(["--glare", "g.png"])
    assert (a.glare, a.glare_psf, a.glare_r0, a.glare_strength, a.glare_taps, a.glare_lambda0, a.spectral_nodes) == ("g.png", None, 2.0, 0.3, 33, 550.0, 81)
    a = CLI.parse_args(["--glare", "g.png", "--glare-psf", "p.npy", "--glare-strength", "0.5", "--glare-taps", "9", "--glare-lambda0", "600",
                        "--spectral-nodes", "16"])
    assert (a.glare_psf, a.glare_strength, a.glare_taps, a.glare_lambda0, a.spectral_nodes) == ("p.npy", 0.5, 9, 600.0, 16)
    assert CLI.parse_args(["--glare", "g.png", "--glare-r0", "3.5"]).glare_r0 == 3.5
    assert CLI.parse_args([]).glare is None
    for argv, word in ((["--glare", "g.png", "--direct"], "--glare cannot be combined with --direct"),
                       (["--glare-taps", "9"], "--glare-taps needs --glare"), (["--glare-r0", "2"], "--glare-r0 needs --glare"),
                       (["--glare-psf", "p.npy"], "--glare-psf needs --glare"), (["--glare-strength", "1"], "--glare-strength needs --glare"),
                       (["--glare-lambda0", "550"], "--glare-lambda0 needs --glare"),
                       (["--glare", "g.png", "--glare-taps", "8"], "odd"), (["--glare", "g.png", "--glare-taps", "67"], "odd"),
                       (["--glare", "g.png", "--glare-strength", "1.5"], "0 .. 1"), (["--glare", "g.png", "--glare-r0", "0"], "greater than 0"),
                       (["--glare", "g.png", "--glare-psf", "p.npy", "--glare-r0", "2"], "give one")):
        with pytest.raises(SystemExit):
            CLI.parse_args(argv)
        assert word in capsys.readouterr().err, argv


# ---- the compiled kernel ----------------------------------------------------------------------------------------------------------------

# The bounds the kernel was built to: 64 VGPRs is the most at which eight waves fit a SIMD (the register file is no limit on
# occupancy); no static LDS, and at 65 taps a dynamic 58,640 bytes -- the tile with its halo and the node's table -- which a launch
# gets without asking (64 KiB) and which lets two workgroups share a CU.
VGPR_BOUND, LDS_BOUND = 64, 65536


def _lds_bytes(taps):
    stride, table_stride = (64 + taps - 1 + 3) // 4 * 4, (taps + 3) // 4 * 4
    return 4 * (stride * (16 + taps - 1) + taps * table_stride)


def test_the_glare_kernel_has_no_scratch_no_spills_no_fused_multiply_add_and_no_matrix_instruction(kernels):
    text = _device_build.device_build()[0]
    names = sorted(n for n in kernels if "rl_glare_kernel" in n)
    assert len(names) == 2 and sorted(n for n in kernels if "glare" in n) == names, sorted(kernels)      # the fast form and the exact skip
    for name in names:
        k = kernels[name]
        print("%s: %d VGPRs, %d SGPRs, %d SGPRs spilled, %d VGPRs spilled, %d bytes of scratch, %d bytes of static LDS"
              % (name, k["vgpr_count"], k["sgpr_count"], k["sgpr_spill_count"], k["vgpr_spill_count"], k["private_segment_fixed_size"],
                 k["group_segment_fixed_size"]))
        assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["private_segment_fixed_size"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k.get("agpr_count", 0) == 0 and k["vgpr_count"] <= VGPR_BOUND and k["group_segment_fixed_size"] == 0, (name, k)
        body = text[text.index("\n%s:" % name):text.index(".Lfunc_end", text.index("\n%s:" % name))]
        mnemonics = set(re.findall(r"^\s+([sv]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|buffer_[a-z0-9_]+|scratch_[a-z0-9_]+)", body, re.M))
        assert len(mnemonics) > 10 and "s_endpgm" in mnemonics, (name, sorted(mnemonics))
        fused = sorted(m for m in mnemonics if "fma" in m or "mad" in m and "f32" in m or "mac" in m or "mfma" in m or "dot" in m)
        assert not fused and not [m for m in mnemonics if m.startswith("scratch_")], (name, fused)
        assert "v_mul_f32" in " ".join(mnemonics) or "v_pk_mul_f32" in mnemonics, (name, sorted(mnemonics))
    fast = [n for n in names if "ILb0E" in n]
    assert len(fast) == 1
    body = text[text.index("\n%s:" % fast[0]):text.index(".Lfunc_end", text.index("\n%s:" % fast[0]))]
    assert "v_pk_mul_f32" in body and "v_pk_add_f32" in body and "ds_read_b128" in body            # two pixels to an operation, 16-byte window loads
    assert [_lds_bytes(t) for t in (1, 33, 65)] == [4 * (64 * 16 + 4), 23184, 58640] and all(_lds_bytes(t) <= LDS_BOUND for t in range(1, 66, 2))
    source = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "rl_glare.hip.h")).read()
    code = re.sub(r"//[^\n]*", "", source)
    assert "fmaf" not in code and "__builtin_amdgcn_mfma" not in code and "#include" not in code      # (rl_api.hip includes it after rl_core.h)
