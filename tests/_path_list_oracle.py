"""rl_scene_step_path_list restated in numpy on top of tests/_step_oracle.py: the listed states that are in range and live make
one segment in place (StepOracle.step_one, which is rl_scene_step_paths' contract record by record); the return value is the
stable list of the listed states that are live afterwards.  Entries >= n_states are skipped; states that are not listed are not
touched, nor are their hits.  Entries are taken to be distinct, as the header asks.  Test-only."""
import numpy as np

import _step_oracle as S


def step_list(oracle, states, seed, stream, list=None, n_list=None, flags=0, hits=None):
    """One listed step of `states` (and `hits`, or None) in place with the StepOracle `oracle`; list None is the identity list
    0 .. n_list - 1 (n_list defaults to len(states)).  Returns the survivors as a uint32 array, in the list's order."""
    n = len(states)
    if list is None:
        n_list = n if n_list is None else n_list
        assert n_list <= n            # RL_E_INVALID in the library
        entries = np.arange(n_list, dtype=np.uint32)
    else:
        entries = np.asarray(list, dtype=np.uint32)[:n_list]
    named = entries[entries < n].astype(np.int64)
    was_live = named[states["end"][named] == S.LIVE]
    if len(was_live):
        sub = states[was_live]
        sub_hits = None if hits is None else hits[was_live]
        oracle.step(sub, seed, stream, flags, hits=sub_hits)
        states[was_live] = sub
        if hits is not None:
            hits[was_live] = sub_hits
    return was_live[states["end"][was_live] == S.LIVE].astype(np.uint32)


def run(oracle, rays, seed, stream, first=0, max_steps=4096):
    """begin, then the listed loop from the identity list until the list is empty: (final states, steps taken)."""
    states = S.begin(rays, first)
    live, steps = None, 0
    while (live is None or len(live)) and steps < max_steps:
        live = step_list(oracle, states, seed, stream, list=live)
        steps += 1
    return states, steps
