"""The spectral film (rl_spectral_unit_*) without a GPU: the CPU restatement (tests/_spectral_oracle.py) against facts that do not
come from the code, the boundary of the C ABI (constants in every mirror, argument checks in the documented order, no CPU fallback,
the host-only observer helper), the compiled kernels' resources (hipcc cross-compiles here) and the command line's --spectral."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
import _image_cases as IC
import _oracle as O
import _spectral_cases as SC
import _spectral_oracle as SO
from _boundary import _Fake, _err
from _device_build import device_build, kernels  # noqa: F401  (kernels is a fixture)
from _image_cases import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID = -1
FUNCTIONS = ("rl_spectral_unit_create", "rl_spectral_unit_destroy", "rl_spectral_unit_clear", "rl_spectral_unit_plot",
             "rl_spectral_unit_plot_photons", "rl_spectral_unit_plot_photons_device", "rl_spectral_unit_download", "rl_spectral_unit_upload",
             "rl_spectral_unit_project", "rl_spectral_observer_cie1931")


# ---- the oracle against facts that do not come from the code ----------------------------------------------------------------------

def test_the_films_total_is_the_photons_total_intensity():
    """Inside [380, 780] nm no node is dropped, (1 - r) + r = 1 and the four weights sum to 1, so the film's total is the photons'.
    Roundings on a photon's eight terms: (1 - r), the product with p, (1 - cx), (1 - cy), the weight's product and the term's
    product -- at most 6 on a term, so the f64 sum of the terms is within 6 2^-24 sum |p| of sum p (doubled below: the weights of a
    photon beyond a border are larger than 1 in size); the film's adds are within splat_bound of that."""
    w, h = 64, 36
    ph = SC.demo_photons(w, h, 1 << 16)
    ph = ph[(ph["wavelength"] >= 380) & (ph["wavelength"] <= 780)]
    assert (ph["probability"] != 0).sum() > 6000
    for n_nodes in SC.NODES:
        film, k, s, exact = SO.splat(w, h, n_nodes, ph)
        total, want = float(film.astype(np.float64).sum()), float(ph["probability"].astype(np.float64).sum())
        bound = float(IC.splat_bound(k, s).sum()) + 12 * SO.U * float(np.abs(ph["probability"].astype(np.float64)).sum())
        print("%d nodes: total %.9g against %.9g, off by %.3g of the bound" % (n_nodes, total, want, abs(total - want) / bound))
        assert abs(total - want) <= bound
        assert not len(SO.violations(film, film, k, s, exact)[0])


def test_at_81_nodes_the_cie_projection_is_the_xyz_film():
    """2^16 oracle photons of the demo scene at 64 x 36 (seed 1, stream 0): project(observer) of the oracle's film against
    _oracle.plot of the same photons, within _spectral_oracle.identity_bound, which is derived there."""
    w, h = 64, 36
    ph = SC.demo_photons(w, h, 1 << 16)
    assert 6000 < (ph["probability"] != 0).sum() < 8000
    table = IC._cie_table()
    got = SO.project(SO.splat(w, h, 81, ph)[0], table)
    want = O.plot(w, h, ph)
    bound, s, k, nodes = SO.identity_bound(w, h, ph, table)
    d = np.abs(got.astype(np.float64) - want)
    on = s > 0
    print("up to %d terms and %d nodes on a pixel; largest difference %.3f of the bound, %.2f 2^-24 S"
          % (k.max(), nodes.max(), (d[on] / bound[on]).max(), (d[on] / (SO.U * s[on])).max()))
    assert on.sum() > 1000 and (d <= bound).all()
    assert not got[~on].any() and not want[~on].any()


def test_two_nodes_split_a_photon_linearly():
    ph = np.zeros(3, SC.PHOTON_DTYPE)
    ph["probability"] = 0.75
    ph["wavelength"] = [380.0, 780.0, 580.0]
    for i in range(3):
        film = SO.splat(1, 1, 2, ph[i:i + 1])[0].reshape(2)
        assert film.tolist() == [[0.75, 0.0], [0.0, 0.75], [0.375, 0.375]][i]
    assert SO.spacing(2) == 400.0 and SO.spacing(81) == 5.0 and SO.node_wavelengths(81)[[0, 1, 80]].tolist() == [380.0, 385.0, 780.0]
    # the fall-off beyond the ends: 377.5 nm leaves half in node 0, 782.5 nm half in node 80, 375 and 785 nm nothing
    ph["wavelength"] = [377.5, 782.5, 375.0]
    film = [SO.splat(1, 1, 81, ph[i:i + 1])[0].reshape(81) for i in range(3)]
    assert film[0][0] == 0.375 and not film[0][1:].any() and film[1][80] == 0.375 and not film[1][:80].any() and not film[2].any()
    ph["wavelength"] = [785.0, 374.9, 785.1]
    assert not SO.splat(1, 1, 81, ph)[0].any()


def test_the_synthetic_set_holds_what_it_says():
    ph = SC.synthetic_photons(64, 36)
    wl = set(ph["wavelength"].tolist())
    assert {375.0, 380.0, 780.0, 785.0} <= wl and set(SO.node_wavelengths(81).tolist()) <= wl
    for v in (375.0, 380.0, 780.0, 785.0):
        assert float(np.nextafter(np.float32(v), np.float32(0))) in wl and float(np.nextafter(np.float32(v), np.float32(1e3))) in wl
    for field in ("x", "y", "wavelength"):
        assert np.isnan(ph[field]).any() and (ph[field] == np.inf).any() and (ph[field] == -np.inf).any()
    p = ph["probability"]
    assert (p == 0).any() and (p < 0).any() and (p == np.inf).any() and (p == SC.TINY).any()
    assert (np.abs(ph["x"][np.isfinite(ph["x"])]) > 1).any() and (ph["x"] == 1).any() and (ph["x"] == -1).any()
    assert 2000 < SO.kept(ph).sum() < len(ph)


# ---- the boundary ---------------------------------------------------------------------------------------------------------------

def test_constants_and_entry_points_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    assert re.search(r"#define RL_SPECTRAL_MAX_NODES 401\b", header) and re.search(r"pub const RL_SPECTRAL_MAX_NODES: u32 = 401;", rust)
    assert _lib.RL_SPECTRAL_MAX_NODES == R.RL_SPECTRAL_MAX_NODES == SO.MAX_NODES == 401
    assert re.search(r"typedef struct RlSpectralUnit RlSpectralUnit;", header) and re.search(r"pub enum RlSpectralUnit \{\}", rust)
    for name in FUNCTIONS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
    # the same parameters in the same order, by count: the header's against the ctypes signature and the Rust declaration
    for name in FUNCTIONS:
        c_args = re.search(r"int %s\(([^;]*)\);" % name, header).group(1).split(",")
        rust_args = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rust, re.S).group(1).split(",")
        assert len(c_args) == len(rust_args) == len(_lib.SIGNATURES[name][1]), name
    assert re.search(r"int rl_debug_spectral_launches\(uint64_t out\[2\]\);", debug) and "rl_debug_spectral_launches" in _lib.DEBUG_SIGNATURES
    assert len(R.spectral_launches()) == 2 and _lib.lib.rl_debug_spectral_launches(None) == RL_E_INVALID
    assert _lib.lib.rl_spectral_unit_destroy(None) == 0
    # the header states the rules the tests hold the unit to
    for rule in ("floorf", "fl as a float", "DIFFERENCE from the XYZ film", "at most eight atomics", "node-major", "RL_E_STATE", "2\\^20",
                 "One user per spectral unit"):
        assert re.search(rule, header), rule


def test_arguments_are_checked_in_the_documented_order_with_no_device():
    """Every failure that comes before a handle is read or a device is touched, each with everything behind it wrong as well."""
    L = _lib.lib
    u, dst, photons = _Fake().ptr, _Fake().ptr, _Fake().ptr
    h = C.c_void_p()
    # create: a NULL out; a zero size; n_nodes; the cube, in 64 bits -- in this order, before the device (an index no machine has)
    assert L.rl_spectral_unit_create(99, 0, 0, 0, None) == RL_E_INVALID and b"null" in _err()
    assert L.rl_spectral_unit_create(99, 0, 36, 0, C.byref(h)) == RL_E_INVALID and b"zero" in _err()
    assert L.rl_spectral_unit_create(99, 64, 0, 500, C.byref(h)) == RL_E_INVALID and b"zero" in _err()
    for n_nodes in (0, 1, 402, 0xFFFFFFFF):
        assert L.rl_spectral_unit_create(99, 65536, 65536, n_nodes, C.byref(h)) == RL_E_INVALID and b"n_nodes" in _err(), n_nodes
    too_large = [(65536, 32768, 2), (65536, 65536, 401), (0xFFFFFFFF, 0xFFFFFFFF, 401), (1 << 16, 1 << 16, 2),   # (2^32 x 2 wraps in 32 bits)
                 (46341, 46341, 2), (1 << 15, 1 << 15, 2), (5360, 1000, 401), (1 << 30, 1, 2), (0xFFFFFFFF, 0x80000001, 2)]
    for w_, h_, n_ in too_large:
        assert L.rl_spectral_unit_create(99, w_, h_, n_, C.byref(h)) == RL_E_INVALID and b"RL_MAX_PIXELS" in _err(), (w_, h_, n_)
    assert not h.value
    # the splats
    assert L.rl_spectral_unit_plot(None, None, 3) == RL_E_INVALID and b"null" in _err()
    assert L.rl_spectral_unit_plot(u, None, 1) == RL_E_INVALID and b"null" in _err()
    for fn in (L.rl_spectral_unit_plot_photons, L.rl_spectral_unit_plot_photons_device):
        assert fn(None, None, 5) == RL_E_INVALID and b"null spectral unit" in _err()
        assert fn(None, photons, 0) == RL_E_INVALID and b"null spectral unit" in _err()
        assert fn(u, None, 5) == RL_E_INVALID and b"null photon buffer" in _err()
        assert fn(u, None, 0) == 0 and fn(u, photons, 0) == 0       # n = 0 does nothing
    assert L.rl_spectral_unit_clear(None) == RL_E_INVALID
    for fn in (L.rl_spectral_unit_download, L.rl_spectral_unit_upload):
        assert fn(None, photons) == RL_E_INVALID and fn(u, None) == RL_E_INVALID and b"null" in _err()
    # project: a NULL unit, matrix or dst
    for args in ((None, None, None), (None, photons, dst), (u, None, dst), (u, photons, None), (u, None, None)):
        assert L.rl_spectral_unit_project(*args) == RL_E_INVALID and b"null" in _err(), args
    # the observer: a NULL out, then n_nodes
    assert L.rl_spectral_observer_cie1931(0, None) == RL_E_INVALID and b"null" in _err()
    out = (C.c_float * (3 * 402))()
    for n_nodes in (0, 1, 402, 0xFFFFFFFF):
        assert L.rl_spectral_observer_cie1931(n_nodes, out) == RL_E_INVALID and b"n_nodes" in _err()
    assert not any(out)


@pytest.mark.skipif(R.device_count() > 0, reason="checks the no-GPU behaviour")
def test_the_spectral_unit_fails_loudly_without_a_device():
    with pytest.raises(R.RlError) as e:
        R.SpectralUnit(64, 36)
    assert e.value.code == -2  # RL_E_NO_DEVICE: there is no CPU implementation to fall back to
    with pytest.raises(R.RlError) as e:
        R.SpectralUnit(64, 36, n_nodes=1)
    assert e.value.code == RL_E_INVALID


def test_the_observer_helper_is_the_table_at_81_nodes_and_the_oracles_elsewhere():
    tab = json.load(open(os.path.join(ROOT, "tests", "golden", "cie1931_xyz.json")))
    table = np.stack([np.array(tab[k], np.float32) for k in "XYZ"], axis=1)
    got = R.spectral_observer_cie1931(81)
    assert got.shape == (81, 3) and got.dtype == np.float32 and got.tobytes() == table.tobytes()
    assert R.spectral_observer_cie1931().tobytes() == table.tobytes()
    for n_nodes in (2, 3, 401):
        got = R.spectral_observer_cie1931(n_nodes)
        want = np.zeros((n_nodes, 3), np.float32)
        for b, wavelength in enumerate(SO.node_wavelengths(n_nodes)):
            row = (C.c_float * 3)()
            O.lib().oracle_tristimulus(float(wavelength), row)
            want[b] = list(row)
        assert got.tobytes() == want.tobytes(), n_nodes
        assert same_bits(got, SC.matrix("cie", n_nodes))
        assert got[0].tobytes() == table[0].tobytes() and got[-1].tobytes() == table[80].tobytes()


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def test_spectral_kernels_use_no_scratch_and_no_lds(kernels):
    """Exactly the two new kernels carry rl_spectral_; neither uses scratch, spills or a dynamic stack; neither uses LDS: the splat
    needs no table, and the projection reads its matrix through wave-uniform loads."""
    mine = {n: k for n, k in kernels.items() if "rl_spectral_" in n}
    splat = [k for n, k in mine.items() if "rl_spectral_photons_kernel" in n]
    proj = [k for n, k in mine.items() if "rl_spectral_project_kernel" in n]
    assert len(splat) == 1 and len(proj) == 1 and len(mine) == 2, sorted(mine)
    for name, k in sorted(mine.items()):
        print("%s: %d VGPRs, %d SGPRs, %d bytes of LDS, %d bytes of scratch" % (name, k["vgpr_count"], k["sgpr_count"], k["group_segment_fixed_size"],
                                                                                    k["private_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["dynamic_stack"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    assert "rl_spectral.hip.h" in re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()


def _body(text, kernel):
    name = re.search(r"^(\S*%s\S*):" % kernel, text, re.M).group(1)
    start = text.index("\n%s:" % name)
    return text[start:text.index(".Lfunc_end", start)]


def test_the_kernels_instructions_are_the_contracts(kernels):
    """The projection accumulates with separate multiplies and adds (no fused or multiply-accumulate instruction anywhere in it),
    reads its matrix through scalar loads and its film through plain dword loads; the splat's atomics are no-return f32 adds, eight
    of them, without a compare-and-swap loop."""
    text = device_build()[0]
    proj, splat = _body(text, "rl_spectral_project_kernel"), _body(text, "rl_spectral_photons_kernel")
    assert not re.search(r"\bv_(fma|fmac|mac|mad|pk_fma)\w*_f32", proj)     # (the splat has some: the correctly rounded divide is made of them)
    assert re.search(r"\bv_mul_f32", proj) and re.search(r"\bv_add_f32", proj)
    assert re.search(r"\bs_load_dword", proj) and re.search(r"\bglobal_load_dword\b", proj)
    assert len(re.findall(r"\bglobal_atomic_add_f32\b", splat)) == 8 and "cmpswap" not in splat


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_the_command_line_takes_spectral_and_refuses_it_with_direct(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "1", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base)
    assert a.spectral is None and a.spectral_nodes == 81
    a = CLI.parse_args(base + ["--spectral", "cube.npy"])
    assert a.spectral == "cube.npy" and a.spectral_nodes == 81 and not a.direct
    a = CLI.parse_args(base + ["--spectral", "cube.npy", "--spectral-nodes", "31", "--features", "g", "--denoise", "clean.png"])
    assert (a.spectral, a.spectral_nodes, a.features, a.denoise) == ("cube.npy", 31, "g", "clean.png")
    with pytest.raises(SystemExit) as e:
        CLI.parse_args(base + ["--direct", "--spectral", "cube.npy"])
    told = capsys.readouterr().err
    assert e.value.code == 2 and "--spectral" in told and "--direct" in told, told
