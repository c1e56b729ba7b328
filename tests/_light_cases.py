"""What the GPU tests of the light calls share (tests/test_gpu_light.py, tests/test_gpu_light_film.py): the scenes with emitters to
sample and a sample buffer that holds the guard's fill."""
import numpy as np

import _guarded as G
import robigo_luculenta_amd as R
from test_gpu_step import _scene
from test_light_abi import _with_lights

SAMPLE = R.LIGHT_SAMPLE_DTYPE


def _lit_scene(name):
    objs, cam = _scene(name)
    if name.startswith("random") or name.endswith("prisms"):
        objs = _with_lights(np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), np.random.default_rng(len(name)))
    return np.ascontiguousarray(objs).view(R.OBJECT_DTYPE), cam


def _prefilled(n):
    return np.frombuffer(bytes([G.FILL]) * (32 * n), dtype=SAMPLE).copy()
