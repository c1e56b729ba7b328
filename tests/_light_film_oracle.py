"""What rl_plot_unit_light_paths puts on the film and into `sampled`, restated in numpy as a pure function of the states, the
samples rl_scene_light_paths wrote for them, the scene's sampleable emitters, the camera samples and the `sampled` bytes the call
was given (include/robigo_luculenta.h: the vertex splat, the ending splat and its drop rule, the byte protocol).  The GPU tests
plot the photons this returns with the CPU oracle, and with rl_plot_unit_plot_photons beside it, and compare films."""
import numpy as np

SKIPPED, VISIBLE = 0, 3
END_EMITTER = 1
PHOTON_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("probability", "<f4"), ("wavelength", "<f4")])


def listed_states(n_states, list=None, n_list=None):
    """The states a call touches: the list's entries below n_states, each once; the identity list when list is None."""
    if list is None:
        return np.arange(n_states if n_list is None else n_list, dtype=np.int64)
    lst = np.asarray(list, dtype=np.uint32)[:len(list) if n_list is None else n_list].astype(np.int64)
    return np.unique(lst[lst < n_states])


def kept_values(states, samples, emitters, sampled, list=None, n_list=None, drop=True):
    """(value, new_sampled): value[i] is what state i puts on the film in this call (0 for a state that is not listed or has nothing
    to add); new_sampled is `sampled` after the call (None when sampled is None).  drop=False keeps every ending: the estimator
    that counts a sampled light twice, for the tests that must tell the two apart."""
    n = len(states)
    rows = listed_states(n, list, n_list)
    value = np.zeros(n, np.float32)
    vertex = np.zeros(n, bool)
    vertex[rows] = (samples["status"][rows] == VISIBLE) & (samples["value"][rows] != 0)
    value[vertex] = samples["value"][vertex]
    ending = np.zeros(n, bool)
    ending[rows] = (states["end"][rows] == END_EMITTER) & (states["value"][rows] != 0)
    if drop and sampled is not None:
        counted = (np.asarray(sampled)[:n] != 0) & np.isin(states["object"], np.asarray(emitters, dtype=np.uint32))
        ending &= ~counted
    assert not (vertex & ending).any()   # a state that has ended on an emitter is never sampled
    value[ending] = states["value"][ending]
    new_sampled = None
    if sampled is not None:
        new_sampled = np.array(sampled, dtype=np.uint8, copy=True)
        new_sampled[rows] = samples["status"][rows] != SKIPPED
    return value, new_sampled


def film_photons(states, samples, emitters, camera, sampled, list=None, n_list=None):
    """(photons, new_sampled): the photons rl_plot_unit_plot_photons is to plot for the film of one rl_plot_unit_light_paths call,
    in state order.  A state whose x or y is not finite is left out, as that call leaves it out."""
    ph, _, new_sampled = film_photon_rows(states, samples, emitters, camera, sampled, list, n_list)
    return ph, new_sampled


def film_photon_rows(states, samples, emitters, camera, sampled, list=None, n_list=None):
    """film_photons with, between the two, the state each photon comes from (a state gives at most one: a vertex splat where
    its sample is visible, an ending splat otherwise)."""
    value, new_sampled = kept_values(states, samples, emitters, sampled, list, n_list)
    with np.errstate(invalid="ignore"):
        on = (value != 0) & np.isfinite(camera["x"][:len(states)]) & np.isfinite(camera["y"][:len(states)])
    ph = np.zeros(int(on.sum()), PHOTON_DTYPE)
    ph["x"], ph["y"] = camera["x"][:len(states)][on], camera["y"][:len(states)][on]
    ph["probability"], ph["wavelength"] = value[on], states["wavelength"][on]
    return ph, np.flatnonzero(on), new_sampled
