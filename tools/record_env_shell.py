#!/usr/bin/env python3
"""Record what the reference's env shell does when every stage acts at once, as data: tests/golden/env_shell/*.npz.

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way oracle/make_golden.py does
(through oracle/gymnasium_standin), builds the env with the reference's OWN StateNoiseProcessor (and FluxObserver), its own sub-episoded
reference generators and its own WeightedSumOfErrors reward, integrates with the reference's Euler solver (as the `*_euler` goldens do,
so the fp64 oracle with its Euler integrates identically), steps it and calls `reset()` whenever a step terminates.

Two random streams of the reference are written out instead of being restated: the noise the StateNoiseProcessor added (its `_noise`
rows, in the order `_add_noise` consumed them) and the parameters of every sub-episode the generators drew (the attributes the generator
keeps plus the scalar draws a recording proxy around its numpy Generator saw).  Per run, everything as float64:

    actions          [K, A]            what the env was stepped with, held: the PMSM full voltage (1, -1, -1), the SCIM 0.4 of it, so that its
                                       episodes last six or seven steps, not three -- every episode runs into the current limit
    draws            [K + 1, n_noisy]  row 0: the noise on the first reset state, row k + 1: the noise on the state of step k
    reset_draws      [n_resets, n_noisy]   the noise on every reset state (row 0 is draws[0]), reset_states the noisy states `reset()` gave
    states           [K, S]            the env's (noisy; with the observer: extended) normalised state after each step
    references       [K, n_ref]        the references the agent holds AFTER step k: the step's, or those of the reset that followed it
    reset_reference  [n_ref]           the references the first reset showed
    rewards, terminated [K]
    param_sets       [n_sets, 9]       column, length, amplitude, frequency, offset, phase [rad], width / high-low ratio, roll, superseded
                                       -- in the order drawn; superseded: drawn by the generator step of a terminating env step, whose
                                       value nobody acts on (the reset that follows draws the next set)
    meta             JSON: oracle/make_golden.py:describe(env) plus env id, solver, wrapper chain, noise description, generator kinds
                     and margins, the reward function's arrays, the wrapped system's state names and limits

The noise wrapper's rng is seeded here (the env's seed never reaches it), and the seeds are chosen so that the noise DECIDES: at least
one step terminates on the noisy row and not on the clean one, or the other way round (PMSM: steps 6, 14, 22 of 30).

Conditions, asserted here and again by tests/test_env_shell_cpu.py: at least two terminations, at least one step whose `terminated`
the noise decided, in the SCIM run regular steps with a defined field angle, and, in the PMSM run, a sub-episode that ends by itself.

    MPLBACKEND=Agg python tools/record_env_shell.py [--out tests/golden/env_shell]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_PMSM, K_SCIM = 30, 16
GEN_KW = dict(episode_lengths=(6, 12), frequency_range=(500, 2000), amplitude_range=(0.1, 0.4), offset_range=(-0.2, 0.2))
# name -> (env id, wrapper chain as data, noisy states, noise keywords, (generator kind, state) pairs, K, held action, seed)
CASES = {
    "pmsm_noise": ("Cont-CC-PMSM-v0", ["StateNoiseProcessor"], ["i_sd", "i_sq"], dict(scale=0.05), (("Sinusoidal", "i_sd"), ("Step", "i_sq")), K_PMSM,
                   (1.0, -1.0, -1.0), 25),
    "scim_noise_flux": ("Cont-CC-SCIM-v0", ["StateNoiseProcessor", "FluxObserver"], ["i_sa", "i_sd", "i_sq"], dict(scale=0.05),
                        (("Sinusoidal", "i_sd"), ("Sinusoidal", "i_sq")), K_SCIM, (0.4, -0.4, -0.4), 2),
}


class _Spy:
    """Passes every call on to a numpy Generator and keeps (method, value) of the scalar draws."""

    def __init__(self, rng):
        self._rng, self.log = rng, []

    def __getattr__(self, name):
        fn = getattr(self._rng, name)

        def call(*a, **k):
            v = fn(*a, **k)
            if np.ndim(v) == 0:
                self.log.append((name, float(v)))
            return v

        return call


def _hook_generator(gen, column, kind, tau, sets):
    """Every `_reset_reference` of this sub-generator appends the parameters of the sub-episode it drew to `sets`."""
    original = gen._reset_reference

    def hooked():
        spy = _Spy(gen._random_generator)
        gen._random_generator = spy
        try:
            original()
        finally:
            gen._random_generator = spy._rng
        extra = [v for _, v in spy.log]
        if kind == "Step":  # ..., the triangular high / low ratio, the roll's uniform (step_reference_generator.py:46-58)
            assert [m for m, _ in spy.log][-2:] == ["triangular", "uniform"]
            phase, width, roll = 0.0, extra[-2], float(int(1.0 / gen._frequency / tau * extra[-1]))
        else:  # ..., the phase's uniform (sinusoidal_reference_generator.py:64)
            assert kind == "Sinusoidal" and [m for m, _ in spy.log][-1:] == ["uniform"]
            phase, width, roll = extra[-1] * 2 * np.pi, 1.0, 0.0
        sets.append([column, int(gen._current_episode_length), float(gen._amplitude), float(gen._frequency), float(gen._offset), phase, width, roll, 0.0])

    gen._reset_reference = hooked


def _hook_noise(processor, draws):
    original = processor._add_noise

    def hooked(state):
        draws.append(np.array(processor._noise[processor._random_pointer], dtype=float))
        return original(state)

    processor._add_noise = hooked


def _record(make_golden, name):
    gem = make_golden.gem
    env_id, chain, noisy, noise_kw, generators, K, held, seed = CASES[name]
    psw, rg = gem.physical_system_wrappers, gem.reference_generators
    wrappers = [psw.StateNoiseProcessor(states=noisy, random_dist="normal", random_kwargs=noise_kw)]
    if "FluxObserver" in chain:
        wrappers.append(psw.FluxObserver())
    subs = [getattr(rg, kind + "ReferenceGenerator")(reference_state=state, **GEN_KW) for kind, state in generators]
    env = gem.make(env_id, ode_solver=make_golden.make_solver("euler"), physical_system_wrappers=tuple(wrappers),
                   reference_generator=rg.MultipleReferenceGenerator(subs))
    env = getattr(env, "unwrapped", env)
    ps = env.physical_system
    base = ps.unwrapped
    names = [str(n) for n in ps.state_names]
    order = sorted(range(len(subs)), key=lambda j: names.index(generators[j][1]))  # (the reference tensor follows the state order)
    sets, draws = [], []
    for column, j in enumerate(order):
        _hook_generator(subs[j], column, generators[j][0], float(base.tau), sets)
    processor = ps
    while type(processor).__name__ != "StateNoiseProcessor":
        processor = processor._physical_system
    _hook_noise(processor, draws)
    # the wrapper's `seed` only passes the env's seed inward; every reset spawns its rng from this sequence, which nobody else sets
    processor._seed_sequence = np.random.SeedSequence(seed)

    actions = np.tile(np.array(held, dtype=float), (K, 1))
    (s0, r0), _ = env.reset(seed=seed)
    reset_states, reset_draws = [np.array(s0, dtype=float)], [draws[-1]]
    step_draws = [draws[-1]]
    states, refs, rewards, term = [], [], [], []
    for k in range(K):
        n_sets = len(sets)
        (s, r), w, t, _, _ = env.step(actions[k])
        step_draws.append(draws[-1])
        states.append(np.array(s, dtype=float)), rewards.append(float(w)), term.append(bool(t))
        if t:
            for row in sets[n_sets:]:  # drawn by this step's generator advance: the reset below draws the set that is acted on
                row[-1] = 1.0
            (s, r), _ = env.reset()
            reset_states.append(np.array(s, dtype=float)), reset_draws.append(draws[-1])
        refs.append(np.array(r, dtype=float))
    sets = np.array(sets)
    assert int(np.sum(term)) >= 2, f"{name}: {int(np.sum(term))} terminations"
    natural = len(sets) - int(sets[:, -1].sum()) - len(subs) * (1 + int(np.sum(term)))
    assert natural >= (1 if name == "pmsm_noise" else 0), f"{name}: no sub-episode ended by itself"  # (the SCIM's episodes are shorter than a sub-episode)
    # the noise decided: the current limit (the only constraint a held voltage reaches), on the recorded row and on that row less its noise
    clean = np.array(states)
    clean[:, [names.index(s) for s in noisy]] -= np.array(step_draws[1:])
    over = lambda rows: rows[:, names.index("i_sd")] ** 2 + rows[:, names.index("i_sq")] ** 2 > 1.0  # noqa: E731
    assert np.array_equal(over(np.array(states)), np.array(term)), f"{name}: a termination the current limit does not explain"
    decided = np.nonzero(over(clean) != np.array(term))[0].tolist()
    assert decided, f"{name}: the noise decided no termination"

    rf = env._reward_function
    meta = make_golden.describe(env)
    lo, hi = env.reference_generator.reference_space.low, env.reference_generator.reference_space.high
    meta.update(env_id=env_id, solver="euler", chain=chain, K=K, episodic=True, constraints="default", action_frame="abc", dead_time_steps=0,
                noise=dict(states=noisy, dist="normal", kwargs=noise_kw), generator_keywords={k: list(v) for k, v in GEN_KW.items()},
                generators=[dict(kind=generators[j][0].lower(), state=generators[j][1], margin=[float(lo[c]), float(hi[c])]) for c, j in enumerate(order)],
                wrapped_state_names=names, wrapped_limits=[float(x) for x in ps.limits],
                state_space_low=[float(x) for x in ps.state_space.low], state_space_high=[float(x) for x in ps.state_space.high],
                reward=dict(weights=[float(x) for x in rf._reward_weights], powers=[float(x) for x in np.asarray(rf._n, dtype=float)],
                            state_length=[float(x) for x in rf._state_length], bias=float(rf._bias), violation_reward=float(rf._violation_reward),
                            referenced_states=[bool(x) for x in env.reference_generator.referenced_states]))
    print(f"{name}: the noise decided `terminated` at steps {decided}")
    return dict(actions=actions, draws=np.array(step_draws), reset_draws=np.array(reset_draws), reset_states=np.array(reset_states),
                states=np.array(states), references=np.array(refs), reset_reference=np.array(r0, dtype=float), rewards=np.array(rewards),
                terminated=np.array(term, dtype=np.uint8), param_sets=sets, meta=np.array(json.dumps(meta, sort_keys=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "env_shell"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    os.makedirs(args.out, exist_ok=True)
    for name in CASES:
        data = _record(make_golden, name)
        path = os.path.join(args.out, name + ".npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        assert size < 64 * 1024, (name, size)
        print(f"{name}: {int(data['terminated'].sum())} terminations at steps {np.nonzero(data['terminated'])[0].tolist()} in {len(data['terminated'])} steps, "
              f"{len(data['param_sets'])} parameter sets ({int(data['param_sets'][:, -1].sum())} superseded), {size} bytes -> {path}")


if __name__ == "__main__":
    main()
