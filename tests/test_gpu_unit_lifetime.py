"""What a handle holds on the device from create to destroy (rl_debug_live_resources): every *_destroy gives back exactly what
its *_create and the handle's calls took, also with a render begun and never ended, and the timing getters keep their documented
contract across completed and rejected calls.  At 1 x 1 and at 33 x 17: odd in both axes, no multiple of the 16-pixel denoise and
error tiles nor of a wave, and more than one tile in x and in y.  The built-in demo scene, 4,096 photons or paths."""
import contextlib
import gc
import math

import numpy as np
import pytest

import _oracle as O
from _query_rays import DeviceBuffer

pytestmark = pytest.mark.gpu

import robigo_luculenta_amd as R  # a missing HIP library is a failure, never a skip

SHAPES = [(1, 1), (33, 17)]
N = 4096
ROUNDS = 20
RL_E_STATE = -5

# (device allocations, streams, plain events, timed pairs) that each handle's struct declares (csrc/rl_api.hip)
SCENE_PLAIN, SCENE_EMITTERS = (1, 0, 0, 0), (3, 0, 0, 0)
TRACE, PLOT, PLOT_EXTERNAL, GATHER, TONEMAP = (2, 1, 1, 0), (2, 1, 4, 0), (1, 1, 4, 0), (2, 1, 0, 0), (3, 0, 0, 0)
DENOISE, SPECTRAL, ERROR = (3, 0, 4, 1 + R.RL_DENOISE_MAX_ITERATIONS), (2, 1, 1, 2), (4, 1, 1, 2)


@pytest.fixture(scope="module")
def demo():
    objs, cam = R.builtin_scene_desc(R.SCENE_DEMO)
    emitters = R.description_emitters(objs)
    assert len(emitters) > 0
    return objs, cam, np.delete(objs, emitters), O.Scene(objs.view(O.OBJECT_DTYPE), O.RlCameraDesc.from_buffer_copy(bytes(cam)))


@contextlib.contextmanager
def alive(make, declared):
    """A handle from create to close(): while it lives the counts are at least `declared` above the reading before it, and after
    close() they are that reading again, whatever the handle's calls took meanwhile."""
    before = R.live_resources()
    unit = make()
    during = R.live_resources()
    assert all(d - b >= k for d, b, k in zip(during, before, declared)), (type(unit).__name__, before, during, declared)
    try:
        yield unit
        held = R.live_resources()
        assert all(d - b >= k for d, b, k in zip(held, before, declared)), (type(unit).__name__, before, held, declared)
    finally:
        unit.close()
    assert R.live_resources() == before, (type(unit).__name__, before, R.live_resources())


def positive(x):
    return math.isfinite(x) and x > 0.0


def one_round(objs, cam, plain_objs, w, h, tmp_path):
    """Every handle type: created, one call through each entry point that launches or copies, its getter read, closed."""
    xyz = np.full((w * h, 3), 0.25, dtype=np.float32)
    with contextlib.ExitStack() as stack:
        scene = stack.enter_context(alive(lambda: R.Scene(objs, cam), SCENE_EMITTERS))
        with alive(lambda: R.Scene(plain_objs, cam), SCENE_PLAIN) as plain:
            assert len(plain.emitters()) == 0 and len(scene.emitters()) > 0
        # (closed in reverse order, each against the reading before its create: a handle that takes more while it is used -- the
        # trace unit's and the gather unit's timed pairs -- does so before the next handle is created)
        plot = stack.enter_context(alive(lambda: R.PlotUnit(0, w, h), PLOT))
        trace = stack.enter_context(alive(lambda: R.TraceUnit(0, w, h, n_photons=N), TRACE))
        # trace: a render, a fused render into a plot unit (a launch of the unit's own, and one an open launch carries), stats()
        trace.render(scene, seed=2, stream=1, first_path_index=64)
        trace.render_fused(scene, plot, N, seed=2, stream=1, first_path_index=64)
        trace.render_fused_sync(scene, plot, N, seed=2, stream=1, first_path_index=64)
        paths, segments, kernel_ms = trace.stats()
        assert paths == 3 * N and segments >= paths and positive(kernel_ms)
        photons = trace.mapped_photons
        # plot: plot, clear, upload, download, exchange_stats -- and a unit on the caller's buffer, which is not the unit's to free
        plot.plot([trace])
        plot.clear()
        plot.upload(xyz)
        assert plot.tristimulus_buffer.tobytes() == xyz.tobytes()
        assert plot.exchange_stats() == (0, 0.0)
        mem = DeviceBuffer(xyz.nbytes)
        with alive(lambda: R.PlotUnit(1, w, h, external_xyz=mem.data_ptr()), PLOT_EXTERNAL) as outside:
            outside.upload(xyz)
        back = np.zeros_like(xyz)
        mem.download(back)  # still the caller's memory after the unit is gone
        assert back.tobytes() == xyz.tobytes()
        # gather: accumulate, save / load, gather_accumulate_ms
        gather = stack.enter_context(alive(lambda: R.GatherUnit(w, h), GATHER))
        gather.accumulate(plot)
        path = str(tmp_path / "buffer.raw")
        gather.save(path)
        gather.load(path)
        assert gather.tristimulus_buffer.tobytes() == xyz.tobytes()
        plot.upload(xyz)
        assert positive(R.gather_accumulate_ms(gather, plot))
        # tonemap: tonemap, rgb_buffer
        with alive(lambda: R.TonemapUnit(w, h), TONEMAP) as tonemap:
            tonemap.tonemap(gather)
            assert tonemap.rgb_buffer.shape == (w * h, 3)
        # denoise: 1 and RL_DENOISE_MAX_ITERATIONS passes, with and without guides, pass_ms
        guides = [stack.enter_context(alive(lambda: R.GatherUnit(w, h), GATHER)) for _ in range(3)]
        dst = stack.enter_context(alive(lambda: R.GatherUnit(w, h), GATHER))
        with alive(lambda: R.DenoiseUnit(w, h), DENOISE) as denoise:
            for iterations in (1, R.RL_DENOISE_MAX_ITERATIONS):
                for given in ((), guides):
                    denoise.denoise(gather, *given, dst=dst, iterations=iterations)
                    ms = denoise.pass_ms()
                    assert all(positive(x) for x in ms[:1 + iterations]) and not any(ms[1 + iterations:]), (iterations, ms)
        # spectral: plot, plot_photons from the host and from the device, project, download / upload, launch_ms
        with alive(lambda: R.SpectralUnit(w, h, 81), SPECTRAL) as spectral:
            spectral.plot([trace])
            spectral.plot_photons(photons)
            on_device = DeviceBuffer(photons.nbytes)
            on_device.upload(photons)
            spectral.plot_photons(on_device)
            spectral.project(R.spectral_observer_cie1931(81), dst)
            film = spectral.download()
            spectral.upload(film)
            assert spectral.download().tobytes() == film.tobytes()
            assert all(positive(x) for x in spectral.launch_ms())
        # error: two observe, estimate, download / upload, launch_ms
        with alive(lambda: R.ErrorUnit(w, h), ERROR) as error:
            for _ in range(2):
                plot.upload(xyz)
                error.observe(plot, N)
            stats, se, tiles = error.estimate()
            assert stats["observations"] == 2 and stats["paths"] == 2 * N
            s, q, k, n = error.download()
            error.upload(s, q, k, n)
            assert error.download()[0].tobytes() == s.tobytes()
            assert all(positive(x) for x in error.launch_ms())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_destroy_gives_back_what_create_and_the_calls_took(demo, shape, tmp_path):
    """Twenty rounds over every handle type: after each close() the four counts are the reading before the create, and after each
    round the reading before the first: nothing grows."""
    objs, cam, plain_objs, _ = demo
    gc.collect()  # (handles other tests dropped in a cycle go now, not between two readings)
    base = R.live_resources()
    for r in range(ROUNDS):
        one_round(objs, cam, plain_objs, shape[0], shape[1], tmp_path)
        assert R.live_resources() == base, (r, base, R.live_resources())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_units_closed_with_a_render_begun(demo, shape):
    """render_fused_begin into a plot unit, then the plot unit and the trace unit closed with the render never ended -- and the same
    for a begun un-fused render: the destroys end it, the counts balance, and an independent render on fresh units afterwards is
    the oracle's, bit for bit."""
    objs, cam, _, oscene = demo
    w, h = shape
    seed, stream, first = 3, 1, 128
    want, _ = oscene.render(w, h, seed, stream, first, N, threads=8)
    gc.collect()
    base = R.live_resources()
    scene = R.Scene(objs, cam)
    with_scene = R.live_resources()
    trace, plot = R.TraceUnit(0, w, h, n_photons=N), R.PlotUnit(0, w, h)
    trace.render_fused_begin(scene, plot, N, seed=seed, stream=stream, first_path_index=first)
    plot.close()
    trace.close()
    assert R.live_resources() == with_scene
    trace = R.TraceUnit(0, w, h, n_photons=N)
    trace.render_begin(scene, seed=seed, stream=stream, first_path_index=first)
    trace.close()
    assert R.live_resources() == with_scene
    fresh = R.TraceUnit(1, w, h, n_photons=N)
    fresh.render(scene, seed=seed, stream=stream, first_path_index=first)
    assert fresh.mapped_photons.tobytes() == want.tobytes()
    fresh.close()
    scene.close()
    assert R.live_resources() == base


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_timing_getters_keep_their_contract(demo, shape):
    """include/robigo_luculenta_debug.h: 0 before the first call; after a completed call every launched slot finite and > 0, and the
    denoise passes the call did not make 0; after a rejected call (a unit of another size: RL_E_STATE) what the last completed call
    left."""
    objs, cam, _, _ = demo
    w, h = shape
    scene = R.Scene(objs, cam)
    trace, plot, gather, dst = R.TraceUnit(0, w, h, n_photons=N), R.PlotUnit(0, w, h), R.GatherUnit(w, h), R.GatherUnit(w, h)
    other_gather, other_plot = R.GatherUnit(w + 1, h), R.PlotUnit(1, w, h + 1)
    denoise, spectral, error = R.DenoiseUnit(w, h), R.SpectralUnit(w, h, 81), R.ErrorUnit(w, h)

    def rejected(call, *args, **kwargs):
        with pytest.raises(R.RlError) as e:
            call(*args, **kwargs)
        assert e.value.code == RL_E_STATE and "does not match" in str(e.value), str(e.value)

    assert trace.stats() == (0, 0, 0.0) and plot.exchange_stats() == (0, 0.0)
    assert denoise.pass_ms() == [0.0] * (1 + R.RL_DENOISE_MAX_ITERATIONS)
    assert spectral.launch_ms() == (0.0, 0.0) and error.launch_ms() == (0.0, 0.0)
    rejected(denoise.denoise, gather, dst=other_gather)  # (rejected before the first completed call: still 0)
    assert denoise.pass_ms() == [0.0] * (1 + R.RL_DENOISE_MAX_ITERATIONS)

    trace.render(scene, seed=2, stream=1, first_path_index=64)
    plot.plot([trace])
    gather.accumulate(plot)
    denoise.denoise(gather, dst=dst, iterations=2)
    ms = denoise.pass_ms()
    assert all(positive(x) for x in ms[:3]) and ms[3:] == [0.0] * (R.RL_DENOISE_MAX_ITERATIONS - 2), ms
    rejected(denoise.denoise, gather, dst=other_gather, iterations=4)
    rejected(denoise.denoise, other_gather, dst=dst, iterations=4)
    assert denoise.pass_ms() == ms

    spectral.plot([trace])
    ms = spectral.launch_ms()
    assert positive(ms[0]) and ms[1] == 0.0, ms
    spectral.project(R.spectral_observer_cie1931(81), dst)
    ms = spectral.launch_ms()
    assert positive(ms[0]) and positive(ms[1]), ms
    rejected(spectral.project, R.spectral_observer_cie1931(81), other_gather)
    assert spectral.launch_ms() == ms

    trace.render_fused_sync(scene, plot, N, seed=2, stream=1, first_path_index=64)
    error.observe(plot, N)
    ms = error.launch_ms()
    assert positive(ms[0]) and ms[1] == 0.0, ms
    error.observe(plot, N)
    error.estimate()
    ms = error.launch_ms()
    assert positive(ms[0]) and positive(ms[1]), ms
    rejected(error.observe, other_plot, N)
    assert error.launch_ms() == ms
