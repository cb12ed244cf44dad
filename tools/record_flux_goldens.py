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

A second table, PARAM_CASES, records runs away from the reference's default machine: the non-default parameter sets of
oracle/make_golden.py (PARAM_SETS: l_sigs != l_sigr, p = 3), other control steps, a negative constant speed, a dead time of two steps and
a FluxObserver that is handed its currents in another order.  They are integrated with the reference's Euler solver (as the `*_euler`
goldens are), so a device env with the EulerSolver integrates identically.  Each of these files holds RUNS = three runs (action seeds
7, 8, 9) of K_PARAM = 200 steps on a leading axis: actions, abc_actions, state, terminated are [3, K, ...]; meta also carries the
make-kwargs exactly as passed (`overrides`), the seeds and the solver.  Conditions, asserted here and again by
tests/flux_fixtures.py:load_runs: l_sigs != l_sigr for the `param` cases; every run terminates at least twice and its longest episode has
at least 30 steps; for the dq cases the angle advance (0.5 + dead time) tau |omega| p is at least 0.02 rad.

Only files that do not exist yet are written; --force records every case again.

    MPLBACKEND=Agg python tools/record_flux_goldens.py [--out tests/golden/flux] [--force]

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
K_PARAM, SEEDS = 200, (7, 8, 9)
MIN_TERMINATIONS, MIN_LONGEST_EPISODE, MIN_ANGLE_ADVANCE = 2, 30, 0.02
# name -> (env id, wrapper chain as data, action width, key of make_golden.PARAM_SETS | None, tau | None, omega_fixed | None)
PARAM_CASES = {
    "flux_param_scim_abc": ("Cont-CC-SCIM-v0", ["FluxObserver"], 3, "scim", 5e-5, -120.0),
    "flux_param_scim_dq_dead2": ("Cont-CC-SCIM-v0", ["DeadTimeProcessor:2", "FluxObserver", "DqToAbcActionProcessor:SCIM"], 2, "scim", 2e-4, -120.0),
    "flux_param_dfim_dq": ("Cont-CC-DFIM-v0", ["FluxObserver", "DqToAbcActionProcessor:DFIM"], 4, "dfim", 2e-4, -100.0),
    "flux_scim_abc_perm": ("Cont-CC-SCIM-v0", ["FluxObserver:i_sb,i_sc,i_sa"], 3, None, None, None),
}


def _wrappers(gem, chain):
    psw = gem.physical_system_wrappers
    out = []
    for spec in chain:
        kind, _, arg = spec.partition(":")
        if kind == "FluxObserver":  # "FluxObserver" | "FluxObserver:i_sb,i_sc,i_sa" (the current names, in the order handed over)
            out.append(psw.FluxObserver(current_names=tuple(arg.split(","))) if arg else psw.FluxObserver())
        elif kind == "DeadTimeProcessor":
            out.append(psw.DeadTimeProcessor(int(arg)))
        else:
            out.append(psw.DqToAbcActionProcessor.make(arg))
    return tuple(out)


def _run(gem, env_id, chain, width, amplitude, hold, K=K, seed=7, **make_kwargs):
    env = gem.make(env_id, physical_system_wrappers=_wrappers(gem, chain), **make_kwargs)
    env = getattr(env, "unwrapped", env)
    ps = env.physical_system
    abc = []
    if any(c.startswith("DqToAbc") for c in chain):  # the outermost wrapper: tap what it hands to the system beneath it
        below = ps._physical_system
        below_simulate = below.simulate
        below.simulate = lambda a: (abc.append(np.array(a, dtype=float)), below_simulate(a))[1]
    rng = np.random.default_rng(seed)
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


def episode_lengths(terminated):
    """The lengths of the episodes of one run (the last one ends with the run)."""
    ends = np.nonzero(np.asarray(terminated))[0]
    return np.diff(np.concatenate([[-1], ends, [len(terminated) - 1]]))


def check_runs(name, terminated, meta):
    """The conditions a PARAM_CASES fixture must meet (see the module docstring); tests/flux_fixtures.py:load_runs states them again."""
    ov = meta["overrides"]
    mp = ov.get("motor", {}).get("motor_parameter")
    if "_param_" in name:
        assert mp is not None and mp["l_sigs"] != mp["l_sigr"], f"{name}: a `param` case needs l_sigs != l_sigr"
    for r, term in enumerate(terminated):
        assert int(term.sum()) >= MIN_TERMINATIONS, f"{name}, run {r}: {int(term.sum())} terminations"
        assert int(episode_lengths(term).max()) >= MIN_LONGEST_EPISODE, f"{name}, run {r}: longest episode {int(episode_lengths(term).max())} steps"
    if any(c.startswith("DqToAbc") for c in meta["chain"]):
        advance = (0.5 + meta["dead_time"]) * meta["tau"] * abs(ov["load"]["omega_fixed"]) * mp["p"]
        assert advance >= MIN_ANGLE_ADVANCE, f"{name}: an angle advance of {advance} rad"


def _record_param_case(make_golden, name, out):
    env_id, chain, width, key, tau, omega_fixed = PARAM_CASES[name]
    overrides = {}
    if key is not None:
        overrides["motor"] = dict(motor_parameter=dict(make_golden.PARAM_SETS[key]))
    if tau is not None:
        overrides["tau"] = tau
    if omega_fixed is not None:
        overrides["load"] = dict(omega_fixed=omega_fixed)  # (the Cont-CC envs' load is a ConstantSpeedLoad: the dict sets its speed)
    for amplitude, hold in ((0.25, 1), (0.5, 1), (1.0, 1), (1.0, 4), (1.0, 16), (1.0, 64)):  # (one scale for the three runs)
        runs = [_run(make_golden.gem, env_id, chain, width, amplitude, hold, K=K_PARAM, seed=seed, ode_solver=make_golden.make_solver("euler"),
                     **json.loads(json.dumps(overrides))) for seed in SEEDS]
        if all(int(d["terminated"].sum()) >= MIN_TERMINATIONS and int(episode_lengths(d["terminated"]).max()) >= MIN_LONGEST_EPISODE for d, _ in runs):
            break
    else:
        raise SystemExit(f"{name}: no tried action scale gives every run {MIN_TERMINATIONS} terminations and an episode of {MIN_LONGEST_EPISODE} steps")
    data, meta = dict(runs[0][0]), dict(runs[0][1], overrides=overrides, seeds=list(SEEDS), solver="euler", K=K_PARAM)
    for key_ in ("actions", "abc_actions", "state", "terminated"):
        if key_ in data:
            data[key_] = np.stack([d[key_] for d, _ in runs])
    for d, m in runs[1:]:  # everything else is the system's, not the run's
        assert m == runs[0][1] and all(np.array_equal(d[k], data[k]) for k in d if k not in ("actions", "abc_actions", "state", "terminated"))
    if omega_fixed is not None:  # the speed the table asks for is the speed of every recorded row
        j = list(data["state_names"]).index("omega")
        assert np.allclose(data["state"][..., j] * data["limits"][j], omega_fixed, rtol=1e-12, atol=0.0)
    check_runs(name, data["terminated"], meta)
    path = os.path.join(out, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **data)
    size = os.path.getsize(path)
    assert size < 256 * 1024, (name, size)
    print(f"{name}: amplitude {amplitude}, hold {hold}, terminations {[int(t.sum()) for t in data['terminated']]}, longest episodes "
          f"{[int(episode_lengths(t).max()) for t in data['terminated']]} in {K_PARAM} steps, {size} bytes -> {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "flux"))
    ap.add_argument("--force", action="store_true", help="record every case again (default: only the files that do not exist yet)")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    gem = make_golden.gem
    os.makedirs(args.out, exist_ok=True)
    todo = lambda name: args.force or not os.path.exists(os.path.join(args.out, name + ".npz"))  # noqa: E731
    for name in PARAM_CASES:
        if todo(name):
            _record_param_case(make_golden, name, args.out)
    for name, (env_id, chain, width) in CASES.items():
        if not todo(name):
            continue
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
