"""Full-width RNG coordinates for the tests of the ray kernels: (seed, stream, first path index) cases whose upper halves are
set or whose path range carries from the low into the high counter word inside one launch, per-state path indices whose 64 lanes
share no high word, `segments` at the edges of 32 bits, and the draws of a case from tools/independent_paths.py's numpy Philox
alone (no rl_rng.h).  tests/test_rng_width.py proves the cases and holds the CPU oracle to the numpy words at them,
tests/test_gpu_rng_width.py holds every kernel to the oracle.  Nothing is built at import."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 36
N_TRACE = 4160     # 65 whole waves: a blocking render of a multiple of 64 paths joins an open launch
N_QUERY = 2113     # 33 waves and a tail of one
M32 = (1 << 32) - 1
LAST = (1 << 64) - 1   # first + n must stay below it (rl_api.hip: path_range_check)

Case = namedtuple("Case", "id seed stream first why")
CASES = [
    Case("carry-mid-wave", 7, 1, (1 << 32) - 2081,
         "the carry into the high counter word falls at lane 33 of wave 32, with a key the suite already trusts"),
    Case("carry-wave-edge", 7, 1, 3 * (1 << 32) - 2048, "the carry falls exactly between two waves, high word >= 2"),
    Case("seed-high", 0xA5A5A5A500000007, 1, 0, "only k1 differs from a tested configuration"),
    Case("stream-high", 7, 0xFFFFFFFF, 0, "c3 all ones"),
    Case("stream-msb", 7, 0x80000001, 0, "c3 with bit 31 set (the second stream of stream-high)"),
    Case("sign-carry", 0x8000000000000000, 0x80000000, (1 << 63) - 2081, "the carry into bit 63"),
    Case("top", (1 << 64) - 1, (1 << 32) - 1, (1 << 64) - 2 - N_TRACE, "the last legal range"),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
CARRY_LANE = {"carry-mid-wave": (32, 33), "carry-wave-edge": (32, 0), "sign-carry": (32, 33)}   # (wave, lane) of the first path past the multiple
ORACLE_BLOCKS = (0, 1, 2, 3, (1 << 31) + 1)

# low words that are float NaN, -0, denormal and infinity patterns: the words ride in float registers
FLOAT_WORDS = (0x7F800001, 0x7FC00000, 0xFFC00001, 0x80000000, 0x00000001, 0x7F800000)
SPECIAL_PATHS = (0, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2)
SEGMENT_EDGES = (0, 1, 4095, 4096, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0x7F800001, 0x7FFFFFFD, 0x7FFFFFFE, 0x80000000,
                 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF)


def paths_of(first, n):
    """The path indices first .. first + n - 1 as uint64."""
    return np.uint64(first) + np.arange(n, dtype=np.uint64)


def carry_position(first, n, bit=32):
    """(wave, lane) of the first path of first .. first + n - 1 whose index is a multiple of 2^bit, or None."""
    step = 1 << bit
    at = (-first) % step
    if at == 0 or at >= n:
        return None
    return at // 64, at % 64


_ip = None


def independent():
    """tools/independent_paths.py, with its Philox checked against Random123's published vectors."""
    global _ip
    if _ip is None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import independent_paths as ip
        ip._philox_kat()
        _ip = ip
    return _ip


def numpy_words(seed, stream, paths, block):
    """(n, 4) uint32: the words of `block` for uint64 `paths` of (seed, stream), by the numpy Philox."""
    ip = independent()
    paths = np.asarray(paths, np.uint64)
    n = len(paths)
    block = np.broadcast_to(np.asarray(block, np.uint64), (n,))
    w = ip.philox4x32_10(paths & np.uint64(M32), paths >> np.uint64(32), block, np.full(n, stream, np.uint64), seed & M32,
                         (seed >> 32) & M32, rounds=ip.PHILOX_ROUNDS)
    return np.stack(w, axis=1).astype(np.uint32)


def numpy_camera(seed, stream, first, n, w=W, h=H):
    """(x, y, wavelength) float32 of paths first .. first + n - 1 on a w x h film: block 0's words through the conversions of
    rl_rng.h (the top 24 bits times 2^-24, times 2^24 / (2^24 - 1); * 400 + 380; * 2 - 1; y over the aspect ratio)."""
    f32 = np.float32
    b0 = numpy_words(seed, stream, paths_of(first, n), 0)
    closed = lambda u: (u >> np.uint32(8)).astype(f32) * f32(5.9604644775390625e-8) * (f32(16777216.0) / f32(16777215.0))
    wavelength = closed(b0[:, 0]) * f32(400.0) + f32(380.0)
    x = closed(b0[:, 1]) * f32(2.0) - f32(1.0)
    y = (closed(b0[:, 2]) * f32(2.0) - f32(1.0)) / (f32(w) / f32(h))
    assert x.dtype == y.dtype == wavelength.dtype == np.float32
    return x, y, wavelength


def mixed_path_indices(n, seed=2026):
    """n uint64 path indices no `begin` makes: half random full 64-bit values; then groups of four -- two that share the low word
    under different high words, two that share the high word over different low words; and, at the front of that second half,
    SPECIAL_PATHS and every FLOAT_WORDS pattern as a low word (under a zero and under a random high word) and as a high word."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    q = n // 2
    rest = n - q
    lo = rng.integers(0, 1 << 32, rest, dtype=np.uint64)
    hi = rng.integers(0, 1 << 32, rest, dtype=np.uint64)
    k = np.arange(rest)
    lo[k % 4 == 1] = lo[k[k % 4 == 1] - 1]       # the same low word as the neighbour before, another high word
    hi[k % 4 == 3] = hi[k[k % 4 == 3] - 1]       # the same high word as the neighbour before, another low word
    out[q:] = (hi << np.uint64(32)) | lo
    fixed = list(SPECIAL_PATHS)
    for w in FLOAT_WORDS:
        fixed += [w, (int(rng.integers(1, 1 << 32)) << 32) | w, (w << 32) | int(rng.integers(0, 1 << 32))]
    assert len(fixed) <= rest
    start = q + 4 * ((rest - len(fixed)) // 8)   # in the middle of the second half, on a group boundary: the groups before it stay
    out[start:start + len(fixed)] = np.array(fixed, dtype=np.uint64)
    return out


def edge_segments(n):
    """n uint32 `segments`, cycling through SEGMENT_EDGES."""
    return np.array(SEGMENT_EDGES, np.uint32)[np.arange(n) % len(SEGMENT_EDGES)]
