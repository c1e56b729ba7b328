#!/usr/bin/env python3
"""Generates tests/golden/edge_paths.json from the CPU oracle (oracle/rl_oracle.cpp).

Scans block 0 of rl_rng_block for a few (seed, stream) pairs and records path indices whose photon is drawn exactly at
an end of its range: x = -1 or +1, the y draw = -1 or +1, wavelength = 380 or 780 nm (each about once in 2^23-2^24
paths, so random batches almost never hold one).  Candidates whose oracle photon has probability > 0 at the landscape
edge shape are preferred (they reach the splat) and marked.  Entries: [seed, stream, path, flags, reaches splat]; the
flags are tests/_image_cases.py's EDGE_* bits.  Re-run after an intended change of the oracle or the RNG slot map."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _image_cases as IC  # noqa: E402
import _oracle as O  # noqa: E402

PAIRS = [(1, 0), (2, 3), (7, 1), (3, 2), (5, 0), (11, 4)]
PATHS_PER_PAIR = 1 << 26
CHUNK = 1 << 22
PER_KIND = 2  # entries kept per edge value


def scan(seed, stream):
    L = O.lib()
    block = np.zeros(CHUNK, np.uint32)
    out = np.zeros((CHUNK, 4), np.uint32)
    found = []
    for start in range(0, PATHS_PER_PAIR, CHUNK):
        path = np.arange(start, start + CHUNK, dtype=np.uint64)
        L.oracle_rng_blocks(seed, stream, O.ptr(path), O.ptr(block), O.ptr(out), CHUNK)
        top = out[:, :3] >> 8
        near = np.flatnonzero(((top == 0) | (top >= (1 << 24) - 4)).any(axis=1))   # the only words that can map to an end
        if not len(near):
            continue
        words = np.ascontiguousarray(out[near, :3])
        c = O.math_f32("closed01", words.view(np.float32).reshape(-1)).reshape(-1, 3)
        for i, f in zip(near, IC.edge_flags(c)):
            if f:
                found.append((start + int(i), int(f)))
    return found


def main():
    objs, cam = O.demo_scene_desc()
    scene = O.Scene(objs, cam)
    w, h = IC.EDGE_SHAPES[0]
    cands = []
    for seed, stream in PAIRS:
        for path, flags in scan(seed, stream):
            ph, _ = scene.render(w, h, seed, stream, path, 1)
            cands.append([seed, stream, path, flags, int(ph["probability"][0] > 0)])
    keep = []
    for mask in IC.EDGE_NAMES:
        mine = sorted([c for c in cands if c[3] & mask], key=lambda c: -c[4])
        for c in mine[:PER_KIND]:
            if c not in keep:
                keep.append(c)
    keep.sort()
    path = os.path.join(ROOT, "tests", "golden", "edge_paths.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in keep) + "\n]\n")
    for c in keep:
        print(c, [IC.EDGE_NAMES[m] for m in IC.EDGE_NAMES if c[3] & m])
    print("%d candidates, %d kept -> %s" % (len(cands), len(keep), path))


if __name__ == "__main__":
    main()
