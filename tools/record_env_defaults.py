#!/usr/bin/env python3
"""Record the per-id defaults of the reference's 54 env classes as data: tests/golden/env_defaults.json.

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way oracle/make_golden.py
does (oracle/gymnasium_standin and $GEM_REFERENCE/src on sys.path), calls `gem.make(env_id)` for every id and writes what its
reference generator and reward function resolved to after `set_modules` (with the reward function's `_state_length` and the physical
system's state-space bounds it is derived from): settings only, no trajectories.

    MPLBACKEND=Agg python tools/record_env_defaults.py [--out tests/golden/env_defaults.json]

`gym_electric_motor_amd.envs.default_env_modules` is checked against this file (tests/test_complete_env_cpu.py).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_IDS = [f"{a}-{c}-{m}-v0" for m in ("PermExDc", "SeriesDc", "ShuntDc", "ExtExDc", "PMSM", "SynRM", "SCIM", "EESM", "DFIM")
           for c in ("CC", "TC", "SC") for a in ("Finite", "Cont")]


def _import_reference():
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    return make_golden.gem


def _pair(v):
    return [float(v[0]), float(v[1])]


def record(env_id, gem):
    env = gem.make(env_id)
    env = getattr(env, "unwrapped", env)
    rg, rf, ps = env.reference_generator, env.reward_function, env.physical_system
    subs = getattr(rg, "_sub_generators", None) or [rg]
    names = [str(n) for n in ps.state_names]
    gens = []
    for g in subs:
        lo, hi = g._limit_margin  # resolved by set_modules: (low, high) in normalised units
        ir = g._initial_range if g._initial_range is not None else (lo, hi)
        gens.append(dict(kind=type(g).__name__, reference_state=str(g._reference_state), limit_margin=_pair((lo, hi)), initial_range=_pair(ir),
                         sigma_range=_pair(g._sigma_range), episode_len_range=[int(x) for x in g._episode_len_range]))
    return dict(
        state_names=names,
        reference_names=[str(n) for n in env.reference_names],
        referenced_states=[bool(x) for x in rg.referenced_states],
        generators=gens,
        reward=dict(_reward_weights=[float(x) for x in rf._reward_weights], _n=[float(x) for x in rf._n], _bias=float(rf._bias),
                    _violation_reward=float(rf._violation_reward), _gamma=float(rf._gamma), reward_range=_pair(rf.reward_range),
                    _state_length=[float(x) for x in rf._state_length]),
        state_space=dict(low=[float(x) for x in ps.state_space.low], high=[float(x) for x in ps.state_space.high]),
        reference_space=dict(low=[float(x) for x in rg.reference_space.low], high=[float(x) for x in rg.reference_space.high]),
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "env_defaults.json"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    gem = _import_reference()
    data = {env_id: record(env_id, gem) for env_id in ENV_IDS}
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(data)} env ids -> {args.out}")


if __name__ == "__main__":
    main()
