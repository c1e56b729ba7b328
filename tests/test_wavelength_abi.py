"""The boundary of wavelength importance sampling's C ABI without a GPU: entry points and structs in every mirror, argument checks in
the documented order before any device work, no CPU fallback, and the command line's rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import robigo_luculenta_amd as R
from robigo_luculenta_amd import _lib
from robigo_luculenta_amd import __main__ as CLI
from _boundary import _Fake, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RL_E_INVALID, RL_E_NO_DEVICE, RL_E_STATE = -1, -2, -5
FUNCTIONS = ("rl_wavelength_table_create", "rl_wavelength_table_destroy", "rl_wavelength_table_download", "rl_wavelength_importance_cie1931",
             "rl_trace_unit_set_wavelengths", "rl_app_run_sampled")


def test_structs_and_entry_points_in_every_mirror():
    header = open(os.path.join(ROOT, "include", "robigo_luculenta.h")).read()
    debug = open(os.path.join(ROOT, "include", "robigo_luculenta_debug.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "ffi.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"typedef struct RlWavelengthTable RlWavelengthTable;", header) and re.search(r"pub enum RlWavelengthTable \{\}", rust)
    assert re.search(r"#define RL_WAVELENGTH_BINS 256", header) and re.search(r"pub const RL_WAVELENGTH_BINS: usize = 256;", rust)
    assert C.sizeof(_lib.RlWavelengthSampling) == 24
    offsets = {n: getattr(_lib.RlWavelengthSampling, n).offset for n, _ in _lib.RlWavelengthSampling._fields_}
    assert offsets == {"importance": 0, "n_nodes": 8, "reserved": 12, "uniform_share": 16}
    assert re.search(r"typedef struct RlWavelengthSampling \{", header) and re.search(r"#\[repr\(C\)\][^\n]*pub struct RlWavelengthSampling \{", rust)
    c_fields = re.search(r"typedef struct RlWavelengthSampling \{(.*?)\} RlWavelengthSampling;", header, re.S).group(1)
    assert re.findall(r"(\w+);", c_fields) == [n for n, _ in _lib.RlWavelengthSampling._fields_]
    assert re.findall(r"pub (\w+):", re.search(r"pub struct RlWavelengthSampling \{(.*?)\}", rust, re.S).group(1)) == [n for n, _ in _lib.RlWavelengthSampling._fields_]
    for name in FUNCTIONS:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES and re.search(r"pub fn %s\(" % name, rust) and re.search(r"int %s\(" % name, header), name
        c_args = re.search(r"int %s\(([^;]*)\);" % name, header).group(1).split(",")
        rust_args = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, rust, re.S).group(1).split(",")
        assert len(c_args) == len(rust_args) == len(_lib.SIGNATURES[name][1]), name
        assert name in integration, name
    assert re.search(r"int rl_debug_wavelength_variant_launches\(uint64_t out\[24\]\);", debug) and "rl_debug_wavelength_variant_launches" in _lib.DEBUG_SIGNATURES
    assert len(R.wavelength_variant_launches()) == 24 and _lib.lib.rl_debug_wavelength_variant_launches(None) == RL_E_INVALID
    assert _lib.lib.rl_wavelength_table_destroy(None) == 0
    # RlAppConfig keeps its layout
    assert C.sizeof(_lib.RlAppConfig) == 136, C.sizeof(_lib.RlAppConfig)
    # the header states the rules the tests hold the table to
    for rule in (r"m_j = \(g_j \+ g_\{j\+1\}\) \* 0\.5", r"d_j = 1 / \(n - 1\) for a NULL importance or G == 0, else u / \(n - 1\) \+ \(1 - u\) \* \(m_j / G\)",
                 r"T_i = \(\(double\)i / M\) \* C_\{n-1\}", r"lambda_i = 380 \+ \(400 / \(n - 1\)\) \* \(j \+ \(T_i - C_j\) / d_j\)",
                 r"W_i = \(float\)\(\(\(double\)Q_\{i\+1\} - \(double\)Q_i\) \* M / 400\.0\)", r"i = v >> 16", r"lambda = Q\[i\] \+ \(Q\[i\+1\] - Q\[i\]\) \* f",
                 r"value = emission \* W", r"must\W+outlive the renders"):
        assert re.search(rule, header), rule


def test_the_cie_importance_needs_no_device():
    out = np.zeros(81)
    assert _lib.lib.rl_wavelength_importance_cie1931(None) == RL_E_INVALID and b"null" in _err()
    assert _lib.lib.rl_wavelength_importance_cie1931(out.ctypes.data) == 0
    import _wavelength_oracle as WO
    assert out.tobytes() == WO.cie_importance().tobytes() and R.wavelength_importance_cie1931().tobytes() == out.tobytes()


def test_create_checks_its_arguments_in_the_documented_order_with_no_device():
    """NULL out; n_nodes outside 2 .. 4096; a share outside (0, 1] or NaN; the rule's own refusal -- each with everything behind it
    wrong as well, on a device index no machine has."""
    L = _lib.lib
    h = C.c_void_p(1)
    huge = np.full(81, 8.0e307)
    assert L.rl_wavelength_table_create(99, None, 0, 0.0, None) == RL_E_INVALID and b"null" in _err()
    for n in (0, 1, 4097, 0xFFFFFFFF):
        assert L.rl_wavelength_table_create(99, huge.ctypes.data, n, float("nan"), C.byref(h)) == RL_E_INVALID and b"n_nodes" in _err(), n
        assert not h.value
    for share in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert L.rl_wavelength_table_create(99, huge.ctypes.data, 81, share, C.byref(h)) == RL_E_INVALID and b"uniform_share" in _err(), share
    assert L.rl_wavelength_table_create(99, huge.ctypes.data, 81, 0.1, C.byref(h)) == RL_E_INVALID and b"overflows" in _err()
    # ... and only then the device
    rc = L.rl_wavelength_table_create(99, None, 2, 1.0, C.byref(h))
    assert rc in (RL_E_INVALID, RL_E_NO_DEVICE) and (b"device" in _err()) and not h.value


def test_set_and_download_check_their_handles_first():
    L = _lib.lib
    table = _Fake()
    unit = (C.c_uint8 * 4096)()          # (a stand-in as large as a trace unit: the last check reads its ticket)
    u = C.cast(unit, C.c_void_p)
    assert L.rl_wavelength_table_download(None, None, None) == RL_E_INVALID and b"null" in _err()
    assert L.rl_trace_unit_set_wavelengths(None, table.ptr) == RL_E_INVALID and b"null" in _err()
    C.cast(table.buf, C.POINTER(C.c_int32))[0] = 3            # a table on another device than the unit's
    assert L.rl_trace_unit_set_wavelengths(u, table.ptr) == RL_E_STATE and b"different devices" in _err()
    C.cast(table.buf, C.POINTER(C.c_int32))[0] = 0
    assert L.rl_trace_unit_set_wavelengths(u, table.ptr) == 0 and L.rl_trace_unit_set_wavelengths(u, None) == 0


def test_the_sampled_app_checks_the_sampling_before_any_device():
    L = _lib.lib
    huge = np.full(81, 8.0e307)
    cfg = _lib.RlAppConfig(64, 36, 99, 1, 4096, 1, 0, 0, 0, 1, 30000, 1, None, None, 0, 0, 0, 0, 0, 0, None, 0)
    target = _lib.RlErrorTarget(-1.0, 0.0, 0, 0)

    def run(sampling, target=None):
        return L.rl_app_run_sampled(C.byref(cfg), C.byref(target) if target else None, C.byref(sampling), None, None, None)

    assert L.rl_app_run_sampled(None, None, None, None, None, None) == RL_E_INVALID and b"null config" in _err()
    assert run(_lib.RlWavelengthSampling(huge.ctypes.data, 0, 1, float("nan")), target) == RL_E_INVALID and b"target" in _err()     # rl_app_run_to_error's own first
    assert run(_lib.RlWavelengthSampling(huge.ctypes.data, 0, 1, float("nan"))) == RL_E_INVALID and b"reserved" in _err()
    assert run(_lib.RlWavelengthSampling(huge.ctypes.data, 1, 0, float("nan"))) == RL_E_INVALID and b"n_nodes" in _err()
    assert run(_lib.RlWavelengthSampling(huge.ctypes.data, 81, 0, float("nan"))) == RL_E_INVALID and b"uniform_share" in _err()
    assert run(_lib.RlWavelengthSampling(huge.ctypes.data, 81, 0, 0.1)) == RL_E_INVALID and b"overflows" in _err()
    with pytest.raises(ValueError):
        R.app_run_to_error(64, 36, 1, wavelength_importance="d65")


@pytest.mark.skipif(R.device_count() > 0, reason="checks the no-GPU behaviour")
def test_the_table_fails_loudly_without_a_device():
    with pytest.raises(R.RlError) as e:
        R.WavelengthTable("cie", 0.1)
    assert e.value.code == RL_E_NO_DEVICE  # there is no CPU implementation to fall back to
    with pytest.raises(R.RlError) as e:
        R.app_run_to_error(64, 36, 1, photons_per_batch=4096, wavelength_importance="cie")
    assert e.value.code == RL_E_NO_DEVICE


def test_the_makefile_and_the_build_know_the_new_files():
    make = open(os.path.join(ROOT, "robigo_luculenta_amd", "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    assert "rl_wavelength.h" in hdrs
    assert "tests/wavelength_host" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_the_command_lines_rules_for_wavelength_sampling(capsys):
    base = ["--width", "64", "--height", "36", "--batches", "2", "--photons-per-batch", "4096", "--quiet"]
    a = CLI.parse_args(base)
    assert a.wavelength_importance is None and a.wavelength_uniform_share is None
    a = CLI.parse_args(base + ["--wavelength-importance", "cie"])
    assert (a.wavelength_importance, a.wavelength_uniform_share) == ("cie", 0.1)
    a = CLI.parse_args(base + ["--wavelength-importance", "cie", "--wavelength-uniform-share", "0.05", "--spectral", "cube.npy", "--target-error", "0.1"])
    assert (a.wavelength_importance, a.wavelength_uniform_share, a.spectral) == ("cie", 0.05, "cube.npy")
    for args, words in ((["--wavelength-uniform-share", "0.5"], ("--wavelength-uniform-share", "--wavelength-importance")),
                        (["--wavelength-importance", "d65"], ("--wavelength-importance",)),
                        (["--wavelength-importance", "cie", "--wavelength-uniform-share", "0"], ("--wavelength-uniform-share",)),
                        (["--wavelength-importance", "cie", "--wavelength-uniform-share", "1.5"], ("--wavelength-uniform-share",)),
                        (["--wavelength-importance", "cie", "--wavelength-uniform-share", "nan"], ("--wavelength-uniform-share",)),
                        (["--wavelength-importance", "cie", "--direct"], ("--direct", "draws its own wavelengths")),
                        (["--wavelength-importance", "cie", "--adaptive", "--target-error", "0.1", "--batches", "16"],
                         ("--adaptive", "draws its own wavelengths"))):
        with pytest.raises(SystemExit) as e:
            CLI.parse_args(base + args)
        told = capsys.readouterr().err
        assert e.value.code == 2 and all(word in told for word in words), (args, told)
