"""Cases for the image kernels (splat, gather, exposure, tonemap, add) at the shapes and values where they can go wrong.

No GPU here: shapes with the kernel paths each one reaches, seeded synthetic XYZ images, adversarial Kahan gather
states, a float32 numpy restatement of the splat (plot_unit.rs:56-95) with a per-pixel bound for atomically ordered
sums, and the bitwise comparison the tests use.  tests/test_image_cases.py proves these helpers on the CPU,
tests/test_gpu_image.py runs them against the device."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# rl_kernels.hip.h: rl_exposure_kernel reads each tile of RL_EXPOSURE_TILE pixels 16 at a time (n16 = count / 16) and adds
# the last count % 16 in a plain loop; rl_gather_kernel handles n_floats & 3 elements in a scalar tail on block 0.
EXPOSURE_TILE = 2048


# ---- shapes ------------------------------------------------------------------------------------------------------

def _shapes():
    out = []
    for n in range(1, 81):                                              # every pixel count 1..80
        out += [(n, 1), (1, n)]
    for k in (0, 1, 2, 5):                                              # around the exposure tile
        for r in (-1, 0, 1, 15, 16, 17, 31, 33):
            if EXPOSURE_TILE * k + r > 0:
                out.append((EXPOSURE_TILE * k + r, 1))
    out += [(7, 7), (3, 6), (5, 7), (130, 131), (333, 127), (101, 37)]  # width * height % 4 = 1, 2, 3 beyond one row
    out += [(1, 4097), (4097, 1), (37, 101), (3, 5)]                   # portrait and extreme aspects
    out += [(1919, 1079), (1279, 719)]                                   # odd large sizes
    out += [(1920, 1080), (3840, 2160)]
    seen, unique = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            unique.append(s)
    return unique


SHAPES = _shapes()
LARGE_SHAPES = [(1919, 1079), (1279, 719), (1920, 1080), (3840, 2160)]
SMALL_SHAPES = [s for s in SHAPES if s not in LARGE_SHAPES]
# trace + splat at odd shapes (tests/test_gpu_image.py)
SPLAT_SHAPES = [(1, 1), (2, 1), (1, 2), (3, 5), (1, 17), (17, 1), (37, 101), (101, 37), (333, 127), (1919, 1079)]
# the edge paths of tests/golden/edge_paths.json are rendered at a landscape, a portrait and a one-pixel-wide shape;
# the generator records whether each path reaches the splat at the first of them
EDGE_SHAPES = [(333, 127), (37, 101), (1, 17)]


def exposure_path(n_pixels):
    """Which code of rl_exposure_kernel the LAST tile of an image of n_pixels runs (every earlier tile is a full one:
    n16 = 128, the unrolled loop, then the `q < n16` pair).  Tiles = 1 is the launch without a prefetch of a next tile."""
    tiles = (n_pixels + EXPOSURE_TILE - 1) // EXPOSURE_TILE
    count = n_pixels - EXPOSURE_TILE * (tiles - 1)
    n16, tail = count // 16, count % 16
    if n16 == 0:
        reads = "no 16-pixel reads"
    elif n16 == 1:
        reads = "n16=1 (one read set, no loop)"
    elif n16 == 2:
        reads = "n16=2 (q < n16 pair, no loop)"
    elif n16 % 2:
        reads = "n16 odd (loop, then the single set)"
    else:
        reads = "n16 even (loop, then the q < n16 pair)"
    return {"tiles": tiles, "last_count": count, "n16": n16, "tail": tail,
            "path": "%s tile(s); last: %s, %s" % ("1 (no prefetch)" if tiles == 1 else str(tiles), reads,
                                                  "tail loop of %d" % tail if tail else "no tail loop")}


def gather_path(n_pixels):
    """rl_gather_kernel over 3 * n_pixels floats: float4 body of n4 lanes, scalar tail of (3 n) & 3 floats on block 0."""
    n_floats = 3 * n_pixels
    return {"n4": n_floats // 4, "tail": n_floats & 3,
            "path": "%s, %s" % ("float4 body of %d" % (n_floats // 4) if n_floats >= 4 else "no float4 body",
                                "scalar tail of %d" % (n_floats & 3) if n_floats & 3 else "no scalar tail")}


def coverage():
    """{(w, h): (exposure path, gather path)} -- what each shape reaches, for a reader of the tests."""
    return {s: (exposure_path(s[0] * s[1])["path"], gather_path(s[0] * s[1])["path"]) for s in SHAPES}


def shape_id(s):
    return "%dx%d" % s


# ---- synthetic XYZ images ---------------------------------------------------------------------------------------------
# Each class is a seeded function of (shape, seed) -> float32 (w * h, 3).  Where the class allows, the LAST pixel holds a
# value from the top of its range, so that a tail loop that drops or doubles it moves sum(Y) and sum(Y * Y).

def _rng(shape, seed, salt):
    return np.random.default_rng([seed, shape[0], shape[1], salt])


def xyz_loguniform(shape, seed):
    """Positive values over 24 decades (1e-12 .. 1e12: Y * Y stays finite), every mantissa drawn."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 1)
    v = (10.0 ** r.uniform(-12, 12, (n, 3))).astype(np.float32)
    v[-1] = np.float32(10.0 ** r.uniform(11.5, 12))
    return v


def xyz_outliers(shape, seed):
    """Values in [0, 1) with a few outliers of ~1e7 among them: the f32 sequential sum depends on where they sit."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 2)
    v = r.uniform(0, 1, (n, 3)).astype(np.float32)
    k = max(1, n // 500)
    v[r.integers(0, n, k)] = r.uniform(1e6, 1e7, (k, 3)).astype(np.float32)
    v[-1] = r.uniform(1e6, 1e7, 3).astype(np.float32)
    return v


def xyz_lone_tail(shape, seed):
    """All zero but the last pixel, which lies in the last count % 16 pixels of the last tile whenever that tile has such
    a tail: then only the exposure kernel's tail loop sees it."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 3)
    v = np.zeros((n, 3), np.float32)
    v[-1] = r.uniform(0.5, 2.0, 3).astype(np.float32)
    return v


def xyz_constant(shape, seed):
    """One value everywhere: mean * mean and sum(Y * Y) / n round apart, so the variance can come out negative (NaN)."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 4)
    return np.full((n, 3), np.float32(r.uniform(0.1, 10.0)), np.float32)


def xyz_yy_overflow(shape, seed):
    """Y of 1 .. 1e15 with a few of 2e19 .. 1e20 among them (the last pixel one of those): Y * Y overflows, so sum(Y * Y)
    and max_intensity are inf while sum(Y) and mean * mean stay finite."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 5)
    v = (10.0 ** r.uniform(0, 15, (n, 3))).astype(np.float32)
    k = max(1, n // 1000)
    v[r.integers(0, n, k)] = r.uniform(2e19, 1e20, (k, 3)).astype(np.float32)
    v[-1] = r.uniform(2e19, 1e20, 3).astype(np.float32)
    return v


def xyz_sum_overflow(shape, seed):
    """Y near the top of f32 (1e37 .. 3e38): sum(Y) itself overflows once there are a few pixels."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 6)
    return r.uniform(1e37, 3e38, (n, 3)).astype(np.float32)


def xyz_denormal(shape, seed):
    """Subnormal values only (their squares underflow to zero)."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 7)
    bits = r.integers(1, 1 << 23, (n, 3), dtype=np.uint32)
    bits[-1] = r.integers(1 << 22, 1 << 23, 3, dtype=np.uint32)
    return bits.view(np.float32)


def xyz_negative_nonfinite(shape, seed):
    """Values of either sign with NaN, +inf and -inf entries among them (in X and Z: a non-finite Y makes max_intensity
    NaN, which the NaN pixels of xyz_nonfinite_y cover) and negative zeros."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 8)
    v = (r.uniform(-1, 1, (n, 3)) * 10.0 ** r.uniform(-3, 3, (n, 3))).astype(np.float32)
    k = max(1, n // 16)
    for val in (np.nan, np.inf, -np.inf, -0.0):
        idx = r.integers(0, n, k)
        v[idx, r.choice([0, 2], k)] = val
    v[r.integers(0, n, k), 1] = -0.0
    v[-1, 1] = np.float32(-r.uniform(500, 1000))
    return v


def xyz_nonfinite_y(shape, seed):
    """Y with a NaN or an infinity among finite values: max_intensity is NaN or inf."""
    v = xyz_outliers(shape, seed)
    r = _rng(shape, seed, 9)
    v[int(r.integers(0, len(v))), 1] = [np.nan, np.inf, -np.inf][int(r.integers(0, 3))]
    return v


XYZ_CLASSES = {
    "loguniform": xyz_loguniform,
    "outliers": xyz_outliers,
    "lone_tail": xyz_lone_tail,
    "constant": xyz_constant,
    "yy_overflow": xyz_yy_overflow,
    "sum_overflow": xyz_sum_overflow,
    "denormal": xyz_denormal,
    "negative_nonfinite": xyz_negative_nonfinite,
    "nonfinite_y": xyz_nonfinite_y,
}


# ---- find_exposure (tonemap_unit.rs:55-69) in numpy, for the sensitivity tests -------------------------------------------

def exposure_from_sums(sum_y, sum_yy, n):
    n = np.float32(n)
    mean = np.float32(sum_y) / n
    sqr_mean = np.float32(sum_yy) / n
    with np.errstate(all="ignore"):
        return np.float32(mean + np.sqrt(np.float32(sqr_mean - mean * mean)))


def sequential_sums(xyz):
    """The reference's sums: f32, one pixel after the other (np.cumsum is a sequential accumulation, np.sum is not)."""
    y = np.ascontiguousarray(xyz[:, 1])
    with np.errstate(all="ignore"):
        return np.cumsum(y, dtype=np.float32), np.cumsum(y * y, dtype=np.float32)


def exposure_variants(xyz):
    """max_intensity as the reference computes it, and as a kernel that (dropped) loses the last pixel, (doubled) adds
    it twice, or (pairwise) sums with a tree (numpy's f32 np.sum) would."""
    n = len(xyz)
    sy, syy = sequential_sums(xyz)
    y = xyz[:, 1]
    with np.errstate(all="ignore"):
        last_yy = np.float32(y[-1] * y[-1])
        return {
            "sequential": exposure_from_sums(sy[-1], syy[-1], n),
            "dropped": exposure_from_sums(sy[-2] if n > 1 else 0.0, syy[-2] if n > 1 else 0.0, n),
            "doubled": exposure_from_sums(np.float32(sy[-1] + y[-1]), np.float32(syy[-1] + last_yy), n),
            "pairwise": exposure_from_sums(np.sum(y, dtype=np.float32), np.sum(y * y, dtype=np.float32), n),
        }


# ---- Kahan gather states (gather_unit.rs:49-64) ----------------------------------------------------------------------

def kahan_states(shape, seed):
    """(acc, comp, [px1, px2, px3]) as float32 (w * h, 3) arrays: accumulators with nonzero compensation, plot buffers that
    cancel them, large-plus-small sums whose low bits only the compensation keeps, and signed zeros, subnormals and
    non-finite values at the end of the buffer (where the gather kernel's scalar tail works)."""
    n = shape[0] * shape[1]
    r = _rng(shape, seed, 10)
    m = n * 3
    acc = (r.uniform(-1, 1, m) * 10.0 ** r.uniform(-4, 8, m)).astype(np.float32)
    comp = (acc * r.uniform(-1, 1, m) * 2.0 ** -24).astype(np.float32)        # nonzero compensation of the acc's size
    pxs = []
    for step in range(3):
        kind = r.integers(0, 4, m)
        px = np.empty(m, np.float32)
        px[kind == 0] = -acc[kind == 0] + r.uniform(-1e-3, 1e-3, (kind == 0).sum()).astype(np.float32)  # cancellation
        px[kind == 1] = r.uniform(0, 1, (kind == 1).sum()).astype(np.float32) * 1e-5                   # large + small
        px[kind == 2] = (r.uniform(-1, 1, (kind == 2).sum()) * 1e8).astype(np.float32)                  # small + large
        px[kind == 3] = comp[kind == 3] * np.float32(r.uniform(0.5, 2.0))                               # px ~ comp
        pxs.append(px)
    tail = [0.0, -0.0, np.float32(1e-45), np.float32(-3e-39), np.inf, -np.inf, np.nan, np.float32(3e38), np.float32(1e-30)]
    for k, val in enumerate(tail[: min(len(tail), m)]):
        (pxs[k % 3])[m - 1 - k] = val
    comp[m - 1] = np.float32(-1e-7)
    return acc.reshape(n, 3), comp.reshape(n, 3), [p.reshape(n, 3) for p in pxs]


def write_gather_raw(path, acc, comp):
    """The headerless buffer.raw that GatherUnit.load reads (gather_unit.rs:68-92): tristimulus then compensation."""
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(acc, np.float32).tobytes())
        f.write(np.ascontiguousarray(comp, np.float32).tobytes())


# ---- the splat (plot_unit.rs:56-95) in float32 numpy --------------------------------------------------------------------

def _cie_table():
    tab = json.load(open(os.path.join(HERE, "golden", "cie1931_xyz.json")))
    return np.stack([np.array(tab[k], np.float32) for k in "XYZ"], axis=1)   # (81, 3)


_CIE = None


def tristimulus(wavelength):
    """cie1931.rs:20-48 for an array of wavelengths: float32 (n, 3)."""
    global _CIE
    if _CIE is None:
        _CIE = _cie_table()
    wl = np.asarray(wavelength, np.float32)
    with np.errstate(all="ignore"):
        indexf = (wl - np.float32(380.0)) / np.float32(5.0)
        fl = np.floor(indexf)
        ok = np.isfinite(fl) & (fl >= -1) & (fl <= 80)
        index = np.where(ok, fl, 0).astype(np.int64)
        rem = (indexf - index.astype(np.float32))[:, None]
        one = np.float32(1.0)
        a = _CIE[np.clip(index, 0, 80)]
        b = _CIE[np.clip(index + 1, 0, 80)]
        inner = a * (one - rem) + b * rem
        lo = _CIE[0][None, :] * rem
        hi = _CIE[80][None, :] * (one - rem)
    out = np.where((index == -1)[:, None], lo, np.where((index == 80)[:, None], hi, inner))
    return np.where(ok[:, None], out, np.float32(0)).astype(np.float32)


def splat_terms(w, h, photons):
    """Pixel indices (n, 4) and float32 contributions (n, 4, 3) of every photon, in the reference's order:
    (py1, px1) c11, (py1, px2) c21, (py2, px1) c12, (py2, px2) c22."""
    f = np.float32
    aspect = f(w) / f(h)
    x = photons["x"].astype(np.float32)
    y = photons["y"].astype(np.float32)
    cie = tristimulus(photons["wavelength"]) * photons["probability"].astype(np.float32)[:, None]
    px = (x * f(0.5) + f(0.5)) * (f(w) - f(1.0))
    py = (y * aspect * f(0.5) + f(0.5)) * (f(h) - f(1.0))
    px1 = np.clip(np.floor(px).astype(np.int64), 0, w - 1)
    px2 = np.clip(np.ceil(px).astype(np.int64), 0, w - 1)
    py1 = np.clip(np.floor(py).astype(np.int64), 0, h - 1)
    py2 = np.clip(np.ceil(py).astype(np.int64), 0, h - 1)
    cx = px - px1.astype(np.float32)
    cy = py - py1.astype(np.float32)
    one = f(1.0)
    wts = np.stack([(one - cx) * (one - cy), cx * (one - cy), (one - cx) * cy, cx * cy], axis=1)
    idx = np.stack([py1 * w + px1, py1 * w + px2, py2 * w + px1, py2 * w + px2], axis=1)
    return idx, (cie[:, None, :] * wts[:, :, None]).astype(np.float32)


def splat(w, h, photons):
    """(image float32 (w * h, 3) summed in the oracle's order, k_p int (w * h, 3), S_p float64 (w * h, 3), exact float64
    (w * h, 3)): k_p counts the nonzero contributions to each pixel component, S_p is the sum of their magnitudes and
    exact their sum in float64 (exact to 2^-53 S_p)."""
    idx, terms = splat_terms(w, h, photons)
    idx = idx.reshape(-1)
    terms = terms.reshape(-1, 3)
    img = np.zeros((w * h, 3), np.float32)
    np.add.at(img, idx, terms)
    k = np.zeros((w * h, 3), np.int64)
    np.add.at(k, idx, (terms != 0).astype(np.int64))
    s = np.zeros((w * h, 3), np.float64)
    np.add.at(s, idx, np.abs(terms.astype(np.float64)))
    exact = np.zeros((w * h, 3), np.float64)
    np.add.at(exact, idx, terms.astype(np.float64))
    return img, k, s, exact


def splat_bound(k, s):
    """Per pixel component: any order of k float32 adds onto zero (k - 1 of them round) lands within (k - 1) 2^-24 S of
    the exact sum (the 1e-6 covers the float64 sum's own error); with k <= 2 every order gives the same bits."""
    return (k - 1).clip(0).astype(np.float64) * 2.0 ** -24 * s * (1 + 1e-6)


def splat_violations(got, want, k, s, exact):
    """Indices (pixel, component) where got is not within splat_bound of the exact sum, or (k <= 2) not want's bits; and
    the worst excess.  (Two rounded orders may lie twice the bound apart, so got is held to the exact sum, not to want.)"""
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - exact)
    bound = splat_bound(k, s)
    bad = np.where(k <= 2, got.view(np.uint32) != np.asarray(want, np.float32).view(np.uint32), ~(d <= bound))
    return np.argwhere(bad), (float((d - bound)[bad].max()) if bad.any() else 0.0)


def splat_leave_one_out(w, h, photons):
    """For every photon, whether the film `splat` returns with that photon alone taken out would still pass: (by splat_violations
    against the k, S and exact of the whole list, by np.allclose(rtol=2e-5, atol=1e-6 max) alone), two bool arrays (n,).
    Vectorised: a photon changes only the components its four terms land on, so the film without it is, on each of those, the
    float32 nearest to (image - the photon's terms on that pixel), and every other component is the image's own, which passes."""
    idx, terms = splat_terms(w, h, photons)
    img, k, s, exact = splat(w, h, photons)
    t64 = terms.astype(np.float64)
    same = idx[:, :, None] == idx[:, None, :]                           # (n, 4, 4): the slots of one photon that share a pixel
    removed = (same[:, :, :, None] * t64[:, None, :, :]).sum(axis=2)    # (n, 4, 3): what the photon put on each slot's pixel
    at = img[idx]                                                       # (n, 4, 3)
    without = (at.astype(np.float64) - removed).astype(np.float32)
    d = np.abs(without.astype(np.float64) - exact[idx])
    bad = np.where(k[idx] <= 2, without.view(np.uint32) != at.view(np.uint32), ~(d <= splat_bound(k[idx], s[idx])))
    scale = float(np.abs(img).max()) if img.size else 0.0
    far = ~(np.abs(without.astype(np.float64) - at) <= 1e-6 * scale + 2e-5 * np.abs(at.astype(np.float64)))
    return ~bad.any(axis=(1, 2)), ~far.any(axis=(1, 2))

# ---- comparison -------------------------------------------------------------------------------------------------------

def same_bits(got, want):
    """Bitwise equality, except that positions where both are NaN count as equal (host and device may differ in a NaN's
    sign or payload).  uint8 arrays are compared exactly."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return got.tobytes() == want.tobytes()
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    eq = got.view(u) == want.view(u)
    return bool(np.all(eq | (np.isnan(got) & np.isnan(want))))


def first_difference(got, want):
    """A short description of where same_bits fails, for assertion messages."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        bad = ~((got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want)))
    else:
        bad = got != want
    idx = np.flatnonzero(bad)
    if not len(idx):
        return "no difference"
    i = idx[0]
    return "%d of %d differ; first at %d: got %r want %r" % (len(idx), got.size, i, got[i], want[i])


# ---- edge paths (tests/golden/edge_paths.json, tools/gen_edge_paths.py) ------------------------------------------------
# Each entry is [seed, stream, path index, flags, reaches the splat at EDGE_SHAPES[0] (0 / 1)]; flags say which of block 0's
# draws sits exactly at its end, as the oracle computes it:
EDGE_X_MINUS, EDGE_X_PLUS, EDGE_Y_MINUS, EDGE_Y_PLUS, EDGE_WL_380, EDGE_WL_780 = 1, 2, 4, 8, 16, 32
EDGE_NAMES = {EDGE_X_MINUS: "x=-1", EDGE_X_PLUS: "x=+1", EDGE_Y_MINUS: "y draw=-1", EDGE_Y_PLUS: "y draw=+1",
              EDGE_WL_380: "wavelength=380", EDGE_WL_780: "wavelength=780"}


def edge_flags(closed01_words):
    """Flags of block-0 draws given closed01 of words 0 (wavelength), 1 (x) and 2 (y): float32 (n, 3) -> int (n,)."""
    c = np.asarray(closed01_words, np.float32)
    f = np.float32
    wl = c[:, 0] * f(400.0) + f(380.0)           # rl_get_wavelength
    x = c[:, 1] * f(2.0) - f(1.0)                # rl_get_bi_unit
    y = c[:, 2] * f(2.0) - f(1.0)
    flags = np.zeros(len(c), np.int64)
    for mask, cond in ((EDGE_X_MINUS, x == -1), (EDGE_X_PLUS, x == 1), (EDGE_Y_MINUS, y == -1), (EDGE_Y_PLUS, y == 1),
                       (EDGE_WL_380, wl == 380), (EDGE_WL_780, wl == 780)):
        flags |= np.where(cond, mask, 0)
    return flags


def load_edge_paths():
    return json.load(open(os.path.join(HERE, "golden", "edge_paths.json")))
