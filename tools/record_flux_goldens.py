#!/usr/bin/env python3
"""Record what the reference's FluxObserver and its flux-oriented dq action processors do, as data: tests/golden/flux/flux_*.npz
(a folder of its own: every .npz directly under tests/golden is an oracle trajectory).

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way oracle/make_golden.py does
(through oracle/gymnasium_standin), builds the env with the reference's OWN wrappers, steps it with seeded random actions and calls
`reset()` whenever a step terminates.  Per run, everything as float64:

    actions          [K, A]        what the env was stepped with (abc duty cycles, or dq actions for the runs with a dq processor)
    abc_actions      [K, 3 | 6]    (dq runs) what the dq processor handed to the system beneath it
    state            [K, S + 2]    the wrapped system's normalised state after each step: the inner state, psi_abs, psi_angle
    terminated       [K]           the env's termination flag of each step; the env was reset after every step where it is set
    reset_state      [S + 2]       the state `reset()` returns (the same after every reset: the initialiser is constant)
    state_names, limits, nominal_state, state_space_low, state_space_high   of the wrapped system
    meta             JSON: env id, wrapper chain, tau, dead time, action amplitude and hold, the supply's u_nominal

A run must contain at least two terminations (checked here and again when the fixture is loaded): the action amplitude, then the number
of steps each random draw is held for, is scaled up until it does.

    MPLBACKEND=Agg python tools/record_flux_goldens.py [--out tests/golden/flux]

Read by tests/test_flux_observer_cpu.py and tests/test_gpu_flux_observer.py.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 300
# name -> (env id, wrapper chain as data, action width)
CASES = {
    "flux_scim_abc": ("Cont-CC-SCIM-v0", ["FluxObserver"], 3),
    "flux_scim_dq": ("Cont-CC-SCIM-v0", ["FluxObserver", "DqToAbcActionProcessor:SCIM"], 2),
    "flux_scim_dq_deadtime": ("Cont-CC-SCIM-v0", ["DeadTimeProcessor:1", "FluxObserver", "DqToAbcActionProcessor:SCIM"], 2),
    "flux_dfim_dq": ("Cont-CC-DFIM-v0", ["FluxObserver", "DqToAbcActionProcessor:DFIM"], 4),
}


def _wrappers(gem, chain):
    psw = gem.physical_system_wrappers
    out = []
    for spec in chain:
        kind, _, arg = spec.partition(":")
        if kind == "FluxObserver":
            out.append(psw.FluxObserver())
        elif kind == "DeadTimeProcessor":
            out.append(psw.DeadTimeProcessor(int(arg)))
        else:
            out.append(psw.DqToAbcActionProcessor.make(arg))
    return tuple(out)


def _run(gem, env_id, chain, width, amplitude, hold):
    env = gem.make(env_id, physical_system_wrappers=_wrappers(gem, chain))
    env = getattr(env, "unwrapped", env)
    ps = env.physical_system
    abc = []
    if any(c.startswith("DqToAbc") for c in chain):  # the outermost wrapper: tap what it hands to the system beneath it
        below = ps._physical_system
        below_simulate = below.simulate
        below.simulate = lambda a: (abc.append(np.array(a, dtype=float)), below_simulate(a))[1]
    rng = np.random.default_rng(7)
    actions = np.repeat(amplitude * rng.uniform(-1.0, 1.0, (K, width)), hold, axis=0)[:K]  # (each draw held for `hold` steps)
    (s0, _), _ = env.reset(seed=0)
    reset_state = np.array(s0, dtype=float)
    states, term = [], []
    for k in range(K):
        (s, _), _, t, _, _ = env.step(actions[k])
        states.append(np.array(s, dtype=float))
        term.append(bool(t))
        if t:
            (s0, _), _ = env.reset()
            assert np.array_equal(np.array(s0, dtype=float), reset_state), "the reset state is not a constant"
    data = dict(actions=actions, state=np.array(states), terminated=np.array(term, dtype=np.uint8), reset_state=reset_state,
                state_names=np.array([str(n) for n in ps.state_names]), limits=np.array(ps.limits, dtype=float),
                nominal_state=np.array(ps.nominal_state, dtype=float), state_space_low=np.array(ps.state_space.low, dtype=float),
                state_space_high=np.array(ps.state_space.high, dtype=float))
    if abc:
        data["abc_actions"] = np.array(abc)
    meta = dict(env_id=env_id, chain=chain, tau=float(ps.tau), dead_time=int(getattr(ps, "dead_time", 0) or 0), amplitude=float(amplitude), hold=int(hold),
                u_nominal=float(ps.unwrapped.supply.u_nominal))
    return data, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "flux"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    gem = make_golden.gem
    os.makedirs(args.out, exist_ok=True)
    for name, (env_id, chain, width) in CASES.items():
        # scale the actions until the run terminates twice: first the amplitude; at full amplitude the converter clips, and a doubly
        # fed machine under white-noise actions stays inside its limits, so from there on each random draw is held for longer
        for amplitude, hold in ((0.25, 1), (0.5, 1), (1.0, 1), (1.0, 4), (1.0, 16), (1.0, 64)):
            data, meta = _run(gem, env_id, chain, width, amplitude, hold)
            n_term = int(data["terminated"].sum())
            if n_term >= 2:
                break
        else:
            raise SystemExit(f"{name}: fewer than two terminations at every tried action scale")
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **data)
        print(f"{name}: amplitude {amplitude}, hold {hold}, {n_term} terminations in {K} steps, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
