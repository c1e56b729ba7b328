"""The relight film's contract (include/robigo_luculenta.h, rl_relight_unit_*) restated in numpy: the routed splat (which records
are skipped, which cube the others go to; the photon's splat itself is _spectral_oracle's), the mix (the composed matrix, then
_spectral_oracle.project), rl_relight_gains_black_body, and the bound that holds a relit image to a re-traced one.  Test-only;
nothing is built at import."""
import numpy as np

import _spectral_oracle as SO

MAX_GROUPS = 16
DROP = 0xFF
NONE = 0xFFFFFFFF
BLACK_BODY = 0
U = SO.U
f32 = np.float32
SAMPLE_DTYPE = np.dtype([("ray", [("origin", "<f4", 3), ("wavelength", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")]),
                         ("x", "<f4"), ("y", "<f4"), ("reserved0", "<u4"), ("reserved1", "<u4")])                    # RlCameraSample
RESULT_DTYPE = np.dtype([("value", "<f4"), ("segments", "<u4"), ("object", "<u4"), ("end", "<u4")])                  # RlPathResult
PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])


def groups_of(objects, n_groups):
    """relight_groups: black bodies get 0, 1, ... in scan order, those beyond n_groups - 1 share the last; the others DROP."""
    lights = np.asarray(objects)["material_kind"] == BLACK_BODY
    table = np.full(len(lights), DROP, np.uint8)
    table[lights] = np.minimum(np.arange(int(lights.sum())), n_groups - 1)
    return table


def photons_of(samples, results):
    """The photon {x, y, value, wavelength} of every record, in order."""
    ph = np.zeros(len(samples), PHOTON_DTYPE)
    ph["x"], ph["y"], ph["wavelength"], ph["probability"] = samples["x"], samples["y"], samples["ray"]["wavelength"], results["value"]
    return ph


def route(samples, results, groups):
    """(photons, group int64) of the records the routed splat does not skip for their object or their group, in order.  (The
    spectral splat's own rules -- a zero value, a non-finite x, y or wavelength -- are applied by _spectral_oracle.)"""
    groups = np.asarray(groups, np.uint8)
    obj = results["object"].astype(np.int64)
    known = obj < len(groups)
    g = np.where(known, groups[np.where(known, obj, 0)], DROP).astype(np.int64)
    on = known & (g != DROP)
    return photons_of(samples, results)[on], g[on]


def kept(samples, results, groups):
    """Which records the routed splat does not skip."""
    groups = np.asarray(groups, np.uint8)
    obj = results["object"].astype(np.int64)
    known = obj < len(groups)
    g = np.where(known, groups[np.where(known, obj, 0)], DROP)
    return known & (g != DROP) & SO.kept(photons_of(samples, results))


def splat(w, h, n_nodes, n_groups, samples, results, groups, onto=None):
    """_spectral_oracle.splat per group: (film float32 (n_groups, n_nodes, h, w), k, S, exact) of the same shape."""
    photons, g = route(samples, results, groups)
    onto = None if onto is None else np.asarray(onto, np.float32).reshape(n_groups, n_nodes, h, w)
    parts = [SO.splat(w, h, n_nodes, photons[g == j], onto=None if onto is None else onto[j]) for j in range(n_groups)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


def compose(gains, matrix, n_groups):
    """c[g * n_nodes + b, k] = gains[g, b] * matrix[b, k], one f32 multiply; gains None: matrix[b, k] itself."""
    matrix = np.asarray(matrix, np.float32).reshape(-1, 3)
    if gains is None:
        return np.tile(matrix, (n_groups, 1))
    gains = np.asarray(gains, np.float32).reshape(n_groups, len(matrix))
    with np.errstate(all="ignore"):
        return (gains[:, :, None] * matrix[None, :, :]).reshape(-1, 3)


def mix(film, gains, matrix):
    """(n_pixels, 3) float32: _spectral_oracle.project of the n_groups * n_nodes planes under the composed matrix."""
    film = np.asarray(film, np.float32)
    n_groups, n_nodes = film.shape[:2]
    return SO.project(film.reshape(n_groups * n_nodes, -1), compose(gains, matrix, n_groups))


def boltzmann(wavelength, kelvins):
    """rl_boltzmann (material.rs:61-74) in float64, operation for operation."""
    h, k, c = 6.62606957e-34, 1.3806488e-23, 299792458.0
    f = c / (np.asarray(wavelength, np.float64) * 1.0e-9)
    with np.errstate(over="ignore"):
        return (2.0 * h * f * f * f) / (c * c * (np.exp(h * f / (k * np.float64(kelvins))) - 1.0))


def normalisation(kelvins, intensity):
    """rl_black_body_normalisation (material.rs:93-99): an f32 divide by the f32 peak."""
    wien = 2.897772126e-3
    return f32(intensity) / f32(boltzmann((wien / np.float64(f32(kelvins))) * 1.0e9, f32(kelvins)))


def intensity(wavelength, kelvins, intensity_):
    """get_intensity (material.rs:101-105): (float)rl_boltzmann((double)l, (double)kelvins) * normalisation, an f32 multiply."""
    l = np.asarray(wavelength, np.float32)
    return boltzmann(l.astype(np.float64), f32(kelvins)).astype(np.float32) * normalisation(kelvins, intensity_)


def gains_black_body(n_nodes, kelvins_from, intensity_from, kelvins_to, intensity_to):
    """rl_relight_gains_black_body: I_to / I_from at the nodes, an f32 divide; 0 where I_from is 0."""
    l = SO.node_wavelengths(n_nodes)
    a, b = intensity(l, kelvins_from, intensity_from), intensity(l, kelvins_to, intensity_to)
    with np.errstate(all="ignore"):
        return np.where(a == 0, f32(0), b / np.where(a == 0, f32(1), a)).astype(np.float32)


def ulps(got, want):
    """The distance in units of the last place between finite float32 arrays of the same sign."""
    return np.abs(np.asarray(got, np.float32).view(np.int32).astype(np.int64) - np.asarray(want, np.float32).view(np.int32).astype(np.int64))


# ---- a relit film against a re-traced one --------------------------------------------------------------------------------------

EXTRA_ROUNDINGS = 5


def retrace_bound(w, h, samples, results_a, results_b, light, gains, table, n_groups):
    """What holds mix(A's 81-node relight film, `gains` on the group of object `light`, the CIE table) to the XYZ film of B's
    results, B being A with that light's kelvins and intensity changed: (bound float64 (w * h, 3), data, rounding), bound = data +
    rounding, per pixel component.
      The data term.  A path that ended on the light has value_B = rho * value_A, rho the exact ratio of the two get_intensity at the
      path's wavelength.  Its photon lands on nodes n and n + 1 with the shares (1 - r) and r, so what the relit film holds of it is
      w v_A ((1 - r) g_n c_n + r g_n+1 c_n+1) against the re-traced w v_A rho ((1 - r) c_n + r c_n+1): with lerp(x) = (1 - r) x_n +
      r x_n+1 the difference is exactly  w v_A (lerp(c) (lerp(g) - rho) + r (1 - r) (g_n - g_n+1) (c_n - c_n+1)).  The first part is the
      interpolation error of the gains at the photon's wavelength; the second is what interpolating gain and observer separately
      differs from interpolating their product by.  data = the sum over the pixel's photons and slots of the magnitudes of both.
      rho is taken from the two f32 values of the path, divided in f64.  (A photon one of whose nodes lies outside the film -- none
      of a camera's -- is held node by node: |w v_A share c_n| |g_n - rho|.)
      The rounding term is _spectral_oracle.identity_bound's for B's photons, with n_groups * nodes in place of its nodes (the mix
      adds up to that many planes that are not zero) and EXTRA_ROUNDINGS = 5 more roundings per term: value_A and value_B each
      round their product with get_intensity (2), a gain is a rounded quotient and the library's may differ from the
      restatement's by the last bit of exp (2), and the composed coefficient is a rounded product (1); S is the larger of B's
      and of the relit film's sum of magnitudes."""
    table64 = np.asarray(table, np.float64).reshape(81, 3)
    gains64 = np.asarray(gains, np.float64).reshape(81)
    n_pixels = w * h
    photons_b = photons_of(samples, results_b)
    _, s_b, k, nodes = SO.identity_bound(w, h, photons_b, table)
    # the photons of the light, by A's values
    mine = (results_a["object"] == light)
    pa = photons_of(samples, results_a)
    lit = pa[mine]
    keep = SO.kept(lit)
    idx, terms = SO.splat_terms(w, h, 81, lit)
    lit = lit[keep]
    va, vb = lit["probability"].astype(np.float64), photons_b[mine][keep]["probability"].astype(np.float64)
    rho = vb / va
    f = (lit["wavelength"] - f32(380.0)) / SO.spacing(81)
    fl = np.floor(f)
    r = (f - fl).astype(np.float64)
    node = np.clip(fl, -1, 80).astype(np.int64)
    n0, n1 = np.clip(node, 0, 80), np.clip(node + 1, 0, 80)
    both = (idx[:, 0] >= 0) & (idx[:, 4] >= 0)
    pixel = np.where(idx[:, :4] >= 0, idx[:, :4], idx[:, 4:]) % n_pixels                       # (m, 4)
    t = np.abs(terms.astype(np.float64))                                                      # (m, 8): |w v_A (1 - r)|, |w v_A r|
    wv = t[:, :4] + t[:, 4:]                                                                  # |w v_A| up to the shares' rounding
    data = np.zeros((n_pixels, 3))
    relit_s = np.zeros((n_pixels, 3))
    for c in range(3):
        cn, cm = table64[n0, c], table64[n1, c]
        gn, gm = gains64[n0], gains64[n1]
        lerp_c, lerp_g = (1 - r) * cn + r * cm, (1 - r) * gn + r * gm
        inner = np.abs(lerp_c * (lerp_g - rho)) + np.abs(r * (1 - r) * (gn - gm) * (cn - cm))
        edge = (t[:, :4] * (idx[:, :4] >= 0)) * np.abs(cn * (gn - rho))[:, None] + (t[:, 4:] * (idx[:, 4:] >= 0)) * np.abs(cm * (gm - rho))[:, None]
        per_slot = np.where(both[:, None], wv * inner[:, None], edge)
        on = (idx[:, :4] >= 0) | (idx[:, 4:] >= 0)
        data[:, c] = np.bincount(pixel[on], weights=per_slot[on], minlength=n_pixels)
        mag = t[:, :4] * (idx[:, :4] >= 0) * np.abs(cn * gn)[:, None] + t[:, 4:] * (idx[:, 4:] >= 0) * np.abs(cm * gm)[:, None]
        relit_s[:, c] = np.bincount(pixel[on], weights=mag[on], minlength=n_pixels)
    # the relit film's magnitudes: the light's photons under the gains, everything else as B has it
    others = photons_b.copy()
    others["probability"][mine] = 0
    _, s_others, _, _ = SO.identity_bound(w, h, others, table)
    s = np.maximum(s_b, s_others + relit_s)
    rounding = (2 * k + n_groups * nodes + 6 + EXTRA_ROUNDINGS)[:, None] * U * s * 1.001
    return data + rounding, data, rounding
