"""What the accumulated XYZ film must add up to: the float64 sum of its photons, within a derived bound.

The film is two levels of float32: atomic adds of a launch's terms into a plot buffer (rl_plot_kernel, the fused trace kernel),
then the Kahan sum of the plot buffers over the gathers (rl_gather_kernel; between ranks that share a GPU one float32 add,
rl_plot_unit_add, comes first).  Here: the terms of a list of photons per gather interval (film_terms), the bound on the film's
distance from their exact sum (accumulation_bound), and whether a lost or doubled photon, launch or batch is certain to break
it (caught_if_lost, caught_if_group_lost).  tests/test_accumulation.py proves these on the CPU with the oracle's photons,
tests/test_gpu_accumulation.py holds the device's films and the App's buffer.raw to them.

This module imports numpy only.  The drivers at its end take the package as an argument and run the depth cases on its device;
tests/test_gpu_accumulation.py and tools/accumulation_depth.py share them."""
import numpy as np

import _image_cases as IC

U = 2.0 ** -24                     # unit roundoff of float32
KAHAN_GATHERS = 65536              # the gather count the bound is stated for: far above any these tests reach
PATHS = 9437184                    # the depth films: 16x9 at 65,536 paths per pixel, 64x36 at 4,096 paths per pixel
DEPTH_SHAPES = [(16, 9), (64, 36)]
DEPTH_SEED, DEPTH_STREAM = 11, 0
SLICE = 65536                      # the reference records are rendered un-fused in slices of this many paths
# G gathers of `launches` launches of `paths` paths each: G * launches * paths = PATHS
DEPTH_SPLITS = {1024: (1, 9216), 16: (9, 65536)}
assert all(g * l * p == PATHS for g, (l, p) in DEPTH_SPLITS.items())


# ---- terms --------------------------------------------------------------------------------------------------------

def lit_terms(w, h, photons):
    """IC.splat_terms of the photons with probability != 0 (the plot kernel skips the others; about 10.5 % of the demo
    scene's paths carry light): (their indices in `photons`, pixel indices (m, 4), float32 contributions (m, 4, 3))."""
    lit = np.flatnonzero(photons["probability"] != 0)
    idx, terms = IC.splat_terms(w, h, photons[lit])
    return lit, idx, terms


def _per_cell(cell, terms, n_cells):
    """k, S and the exact sum per (cell, component) of float32 terms (m, 3) that land on cells (m,): np.bincount with
    weights sums in float64 in the order of the array, as np.add.at does, in a fraction of its time."""
    t64 = terms.astype(np.float64)
    k = np.empty((n_cells, 3), np.int64)
    s = np.empty((n_cells, 3), np.float64)
    exact = np.empty((n_cells, 3), np.float64)
    for c in range(3):
        k[:, c] = np.bincount(cell, weights=(t64[:, c] != 0), minlength=n_cells).astype(np.int64)
        s[:, c] = np.bincount(cell, weights=np.abs(t64[:, c]), minlength=n_cells)
        exact[:, c] = np.bincount(cell, weights=t64[:, c], minlength=n_cells)
    return k, s, exact


def film_terms(w, h, photons, interval, n_intervals=None):
    """(k_j int64, S_j float64, exact_j float64), each (n_intervals, w * h, 3): per gather interval, pixel and component
    the number of nonzero terms, the sum of their magnitudes and their sum in float64 (exact to 2^-53 k_j S_j).
    interval: (n,) the gather interval every photon was accumulated in."""
    interval = np.asarray(interval, np.int64)
    if n_intervals is None:
        n_intervals = int(interval.max()) + 1 if len(interval) else 1
    lit, idx, terms = lit_terms(w, h, photons)
    cell = (interval[lit][:, None] * (w * h) + idx).reshape(-1)
    k, s, exact = _per_cell(cell, terms.reshape(-1, 3), n_intervals * w * h)
    shape = (n_intervals, w * h, 3)
    return k.reshape(shape), s.reshape(shape), exact.reshape(shape)


# ---- the bound ------------------------------------------------------------------------------------------------------

def kahan_bound(gathers, s):
    """Kahan's sum of `gathers` float32 values whose magnitudes add up to s lies within (2u + 3 G u^2) s of their exact sum
    (Higham, Accuracy and Stability of Numerical Algorithms, (4.8): 2u + O(G u^2); 3 G u^2 covers the second-order term for G u < 0.1)."""
    return (2 * U + 3 * gathers * U * U) * np.asarray(s, np.float64)


def accumulation_bound(k_j, s_j, ranks=1):
    """Per pixel component, how far the accumulated film may lie from the exact sum of its terms:

        sum_j max(k_j - 1, 0) u S_j (1 + 1e-6)      the splat of every interval, any order of the atomic adds (IC.splat_bound)
      + (ranks - 1) u S (1 + 1e-6)                  the float32 add between ranks that share a GPU (rl_plot_unit_add)
      + (2u + 3 * 65536 u^2) S (1 + 1e-6)           Kahan over the gathers (kahan_bound; 65536 costs under 1 % of 2u)

    with S = sum_j S_j.  k_j, s_j: (G, pixels, 3) from film_terms.  With (pixels, 3) arrays -- the k and S of the whole list, the
    partition into intervals unknown (the App) -- the first term is (k - 1) u S, which is at least that of every partition:
    k_j - 1 <= k - 1 and sum_j S_j = S."""
    k_j, s_j = np.asarray(k_j), np.asarray(s_j, np.float64)
    if k_j.ndim == 2:
        k_j, s_j = k_j[None], s_j[None]
    s = s_j.sum(axis=0)
    slack = 1 + 1e-6
    splat = IC.splat_bound(k_j, s_j).sum(axis=0)        # carries its own (1 + 1e-6)
    return splat + (ranks - 1) * U * s * slack + kahan_bound(KAHAN_GATHERS, s) * slack


def violations(got, exact, bound):
    """Indices (pixel, component) where got (float32) is not within bound of exact, and the largest |got - exact| / bound
    (0 / 0 counts as 0: a component no term lands on must be exactly zero)."""
    d = np.abs(np.asarray(got, np.float64) - exact)
    with np.errstate(all="ignore"):
        ratio = np.where(d == 0, 0.0, d / bound)
    return np.argwhere(~(d <= bound)), float(ratio.max()) if ratio.size else 0.0


# ---- what a loss must show ------------------------------------------------------------------------------------------------

def caught_if_lost(terms, idx, bound):
    """bool (m,): is a film that lacks (or doubles) photon i alone certain to break `bound`?  Such a film is held to the sum
    without (with twice) the photon by a bound no larger than this one, so it lies at least (the photon's total on a pixel
    component) - bound from the exact sum of the whole list: beyond bound wherever that total exceeds 2 * bound.
    terms (m, 4, 3), idx (m, 4): lit_terms; bound (pixels, 3)."""
    out = np.zeros(len(idx), bool)
    for lo in range(0, len(idx), 1 << 18):                               # in pieces: the (m, 4, 4, 3) product is large
        i, t64 = idx[lo:lo + (1 << 18)], terms[lo:lo + (1 << 18)].astype(np.float64)
        same = i[:, :, None] == i[:, None, :]                            # the slots of one photon that share a pixel
        total = (same[:, :, :, None] * t64[:, None, :, :]).sum(axis=2)   # (m, 4, 3): what the photon put on each slot's pixel
        out[lo:lo + (1 << 18)] = (np.abs(total) > 2 * bound[i]).any(axis=(1, 2))
    return out


def caught_if_group_lost(terms, idx, bound, group, n_groups=None):
    """bool (n_groups,): caught_if_lost for all the photons of a group (a launch, a batch) lost or doubled together.
    group: (m,) the group of every photon of `terms`."""
    group = np.asarray(group, np.int64)
    if n_groups is None:
        n_groups = int(group.max()) + 1 if len(group) else 0
    pixels = bound.shape[0]
    cell = (group[:, None] * pixels + idx).reshape(-1)
    flat = terms.reshape(-1, 3).astype(np.float64)
    total = np.stack([np.bincount(cell, weights=flat[:, c], minlength=n_groups * pixels) for c in range(3)], axis=1)
    return (np.abs(total.reshape(n_groups, pixels, 3)) > 2 * bound[None]).any(axis=(1, 2))


# ---- the Kahan gather (gather_unit.rs:49-64) and the sum it replaces, in float32 numpy ------------------------------------

def naive_sum(buffers):
    """The float32 running sum of plot buffers, one after the other: what the gather would hold without its compensation."""
    acc = np.zeros_like(np.asarray(buffers[0], np.float32))
    for px in buffers:
        acc = (acc + np.asarray(px, np.float32)).astype(np.float32)
    return acc


# ---- drivers of the depth cases (R: the package; no import of it here) ------------------------------------------------------

def device_records(R, scene, w, h, pin=None):
    """The device's un-fused records of paths [0, PATHS) of (DEPTH_SEED, DEPTH_STREAM), downloaded slice by slice: (path indices
    of the records that carry light, those records, all SLICE records of slice `pin` or None)."""
    t = R.TraceUnit(0, w, h, n_photons=SLICE)
    path, records, pinned = [], [], None
    for s in range(PATHS // SLICE):
        t.render(scene, seed=DEPTH_SEED, stream=DEPTH_STREAM, first_path_index=s * SLICE)
        ph = t.mapped_photons
        if s == pin:
            pinned = ph
        lit = np.flatnonzero(ph["probability"] != 0)
        path.append(lit + s * SLICE)
        records.append(ph[lit])
    return np.concatenate(path), np.concatenate(records), pinned


def run_depth_case(R, scene, w, h, fused, gathers, on_plot_buffer=None):
    """Accumulates the PATHS paths of a depth film on the device in `gathers` gathers (DEPTH_SPLITS) and returns the
    GatherUnit.  Nothing waits for the device or reads from it until the last gather is queued -- except on_plot_buffer(j, P_j),
    if given (un-fused only), which receives every plot buffer before its gather.
    fused, one launch per gather: two plot units take turns as the App's do, each gathered while the next launch splats into
    the other."""
    launches, n = DEPTH_SPLITS[gathers]
    g = R.GatherUnit(w, h)
    kw = dict(seed=DEPTH_SEED, stream=DEPTH_STREAM)
    if fused and launches == 1:
        traces = [R.TraceUnit(i, w, h, n_photons=64) for i in range(2)]
        plots = [R.PlotUnit(i, w, h) for i in range(2)]
        for j in range(gathers):
            traces[j & 1].render_fused(scene, plots[j & 1], n, first_path_index=j * n, **kw)
            if j:
                g.accumulate(plots[(j - 1) & 1])
        g.accumulate(plots[(gathers - 1) & 1])
    elif fused:
        t, p = R.TraceUnit(0, w, h, n_photons=64), R.PlotUnit(0, w, h)
        for j in range(gathers):
            for i in range(launches):
                t.render_fused(scene, p, n, first_path_index=(j * launches + i) * n, **kw)
            g.accumulate(p)
    else:
        t, p = R.TraceUnit(0, w, h, n_photons=n), R.PlotUnit(0, w, h)
        for j in range(gathers):
            for i in range(launches):
                t.render_async(scene, first_path_index=(j * launches + i) * n, **kw)
                p.plot([t])                               # the next render waits for this plot on the device
            if on_plot_buffer is not None:
                on_plot_buffer(j, p.tristimulus_buffer)
            g.accumulate(p)
    g.sync()                                              # the first wait: the trace and plot units go away on return
    return g


def error_figures(got, exact, bound, srgb=None, want_srgb=None):
    """What tools/accumulation_depth.py prints per case: max and median of |got - exact| / exact over the lit components, max of
    |got - exact| / bound, and max |delta sRGB|."""
    d = np.abs(np.asarray(got, np.float64) - exact)
    on = exact != 0
    out = {"max_rel": float((d[on] / exact[on]).max()), "median_rel": float(np.median(d[on] / exact[on])),
           "max_over_bound": violations(got, exact, bound)[1]}
    if srgb is not None:
        out["max_dsrgb"] = float(np.abs(srgb.astype(np.float64) - want_srgb).max())
    return out
