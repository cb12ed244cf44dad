#!/usr/bin/env python3
"""Record what the reference's observation-side wrappers make of a system, as data: tests/golden/obs_stage/.

TEST INFRASTRUCTURE ONLY -- never imported by the product package.  Imports the unmodified reference the way tools/record_env_defaults.py
does and writes

    metadata.json   per case: how the env was built (env id, wrapper chain, state filter) and what the WRAPPED reference system shows --
                    state_names, state_positions, limits, nominal_state, state-space low / high --, the env's state_filter indices, and
                    the lengths of the state `reset()` and `step()` hand out (they differ for CosSinProcessor(remove_angle=True))
    <case>.npz      for four cases 200 steps with constant actions, Euler solver at the env's tau: actions, the raw state of the inner
                    system, the wrapped system's state, the observation's state part, the terminated flags

    MPLBACKEND=Agg python tools/record_obs_stage.py [--out tests/golden/obs_stage]

Read by tests/test_obs_stage_cpu.py and tests/test_gpu_obs_stage.py.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHUNT_IDS = [f"{a}-{c}-ShuntDc-v0" for c in ("CC", "TC", "SC") for a in ("Finite", "Cont")]
K = 200

_SUM = dict(kind="CurrentSumProcessor", currents=["i_a", "i_e"], limit="max")
# case -> (env id, wrapper chain as data (None: what gem.make builds by itself), state_filter, constant action of the recorded run or None)
CASES = {f"shunt_{i.split('-')[0].lower()}_{i.split('-')[1].lower()}": (i, None, None, [0.05] if i == "Cont-CC-ShuntDc-v0" else None) for i in SHUNT_IDS}
CASES.update({
    "pmsm_cossin": ("Cont-CC-PMSM-v0", [dict(kind="CosSinProcessor", angle="epsilon", remove_angle=False)], None, [0.2, -0.1, 0.05]),
    "pmsm_cossin_remove": ("Cont-CC-PMSM-v0", [dict(kind="CosSinProcessor", angle="epsilon", remove_angle=True)], None, [0.2, -0.1, 0.05]),
    "scim_cossin_filter": ("Cont-CC-SCIM-v0", [dict(kind="CosSinProcessor", angle="epsilon", remove_angle=False)],
                           ["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"], None),
    "extex_sum": ("Cont-CC-ExtExDc-v0", [dict(kind="CurrentSumProcessor", currents=["i_a", "i_e"], limit="sum")], None, [0.3, 0.2]),
    "pmsm_sum_cossin": ("Cont-CC-PMSM-v0", [dict(kind="CurrentSumProcessor", currents=["i_sd", "i_sq"], limit="max"),
                                            dict(kind="CosSinProcessor", angle="epsilon", remove_angle=True)], None, None),
})


def _import_reference():
    from oracle import make_golden  # puts the gymnasium stand-in and the reference on sys.path, imports it

    return make_golden.gem


def _wrappers(gem, chain):
    psw = gem.physical_system_wrappers
    out = []
    for spec in chain:
        if spec["kind"] == "CurrentSumProcessor":
            out.append(psw.CurrentSumProcessor(tuple(spec["currents"]), limit=spec["limit"]))
        else:
            out.append(psw.CosSinProcessor(angle=spec["angle"], remove_angle=spec["remove_angle"]))
    return tuple(out)


def _floats(a):
    return [float(x) for x in np.asarray(a, dtype=float)]


def record(name, gem, out_dir):
    env_id, chain, state_filter, action = CASES[name]
    kw = {}
    if chain is not None:
        kw["physical_system_wrappers"] = _wrappers(gem, chain)
    if state_filter is not None:
        kw["state_filter"] = list(state_filter)
    if action is not None:
        from gym_electric_motor.physical_systems import solvers

        kw["ode_solver"] = solvers.EulerSolver()
    env = gem.make(env_id, **kw)
    env = getattr(env, "unwrapped", env)
    ps = env.physical_system
    inner = ps.unwrapped
    meta = dict(
        env_id=env_id, chain=chain if chain is not None else [_SUM], built_by="gem.make" if chain is None else "physical_system_wrappers",
        state_filter_names=state_filter, inner_state_names=[str(n) for n in inner.state_names],
        state_names=[str(n) for n in ps.state_names], state_positions={str(k): int(v) for k, v in ps.state_positions.items()},
        limits=_floats(ps.limits), nominal_state=_floats(ps.nominal_state), state_space_low=_floats(ps.state_space.low),
        state_space_high=_floats(ps.state_space.high), state_filter=[int(i) for i in env.state_filter], tau=float(ps.tau),
    )
    (state0, _), _ = env.reset(seed=0)
    meta["reset_state_len"] = int(len(ps.reset()))
    if action is None:
        (state1, _), *_ = env.step(env.action_space.sample() * 0)
        meta["step_state_len"] = int(len(ps.simulate(env.action_space.sample() * 0)))
        return meta
    # the recorded run: constant action (halved until the run does not terminate), the inner system's state tapped where the innermost
    # wrapper reads it
    raw, wrapped = [], []
    inner_simulate = inner.simulate
    inner.simulate = lambda a: (raw.append(np.array(inner_simulate(a), dtype=float)), raw[-1])[1]
    outer_simulate = ps.simulate
    ps.simulate = lambda a: (wrapped.append(np.array(outer_simulate(a), dtype=float)), wrapped[-1])[1]
    env._physical_system = ps
    for halvings in range(8):
        actions = np.tile(np.asarray(action, dtype=float) / 2 ** halvings, (K, 1))
        env.reset(seed=0)
        del raw[:], wrapped[:]
        obs, term = [], []
        for k in range(K):
            (s, _), _, t, _, _ = env.step(actions[k])
            obs.append(np.array(s, dtype=float))
            term.append(bool(t))
            if t:
                break
        if not any(term):
            break
    else:
        raise SystemExit(f"{name}: every tried constant action terminates; choose another one")
    meta["step_state_len"] = int(len(wrapped[0]))
    meta["solver"] = "euler"
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), actions=actions, raw_state=np.array(raw), wrapped_state=np.array(wrapped),
                        observation_state=np.array(obs), terminated=np.array(term, dtype=np.uint8))
    return meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "obs_stage"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    gem = _import_reference()
    os.makedirs(args.out, exist_ok=True)
    data = {name: record(name, gem, args.out) for name in CASES}
    with open(os.path.join(args.out, "metadata.json"), "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(data)} cases -> {args.out}")


if __name__ == "__main__":
    main()
