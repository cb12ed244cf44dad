"""GPU tests of the fused WeightedSumOfErrors reward itself (run with `-m gpu` on an MI355X), at the shapes the recorded runs do not
reach: states of length 1 beside states of length 2, 0 / 1 / 4 references, 1 .. 24 weighted states (the first four terms are evaluated
from registers, the others in a loop through memory), powers other than 1 and 2 (which send every term through that loop), every
remainder of the row groups of both kernels, float32 / float64, AoS / SoA, chunked launches.

The reward is a pure function of what a launch returned: every test evaluates tests/reward_restatement.py in float64 on the returned
observations, the references as the device received them and the returned done mask, and compares.  Weights, powers and lengths come
from tests/reward_path_cases.py (literals) and tests/golden/env_defaults.json (recorded from the reference), never from the reward
description the product derived.  Every run also tells the right restatement from the wrong ones of reward_path_cases.Case.mutants
on its own inputs, by 100 tolerances on more than half of its samples: a run that cannot is not a test of that path.

Measured errors, mutant separations and the cases per path: profiles/reward_paths.md (from the REWARD_PATHS lines printed below)."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reward_path_cases as rp  # noqa: E402
from reward_restatement import full_references, reward  # noqa: E402

RUNS = rp.pruned_runs()


def _random_actions(ps, lead, rng):
    """Uniform over the system's action space: [*lead, A] float64, [*lead] uint8, or [*lead, 2] uint8 (MultiDiscrete)."""
    sp = ps.action_space
    if hasattr(sp, "nvec"):
        return np.stack([rng.integers(0, int(v), lead) for v in sp.nvec], axis=-1).astype(np.uint8)
    if hasattr(sp, "n"):
        return rng.integers(0, int(sp.n), lead).astype(np.uint8)
    return rng.uniform(np.asarray(sp.low, dtype=np.float64), np.asarray(sp.high, dtype=np.float64), tuple(lead) + tuple(sp.shape))


def _run(case, dtype, K, n, layout, actions, refs, chunks=None):
    """-> (obs [K, n, S] float64, refs as the device received them [K, n, n_ref] float64, done [K, n] bool, reward [K, n] device dtype
    as numpy, last_launch()).  chunks: the K steps as several launches of these lengths."""
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make(case.env_id, n_envs=n, dtype=dtype, obs_layout=layout, auto_reset=True)
    ps = env.physical_system
    assert list(ps.state_names) == case.names
    ps.set_reward(referenced_states=case.ref_names, **case.set_reward_kwargs)
    tdt = getattr(torch, dtype)
    r_dev = torch.as_tensor(refs).to(device="cuda", dtype=tdt).contiguous()  # what the device receives, in the handle's dtype
    outs, k0 = [], 0
    for kc in (chunks or [K]):
        o, d, r = ps.rollout(actions[k0:k0 + kc], references=r_dev[k0:k0 + kc] if case.ref_cols else None,
                             reward_out=None if case.ref_cols else torch.empty((kc, n), dtype=tdt, device="cuda"))
        outs.append((o.clone(), d.clone(), r.clone()))
        k0 += kc
    torch.cuda.synchronize()
    launch = ps.last_launch()
    obs, done, rew = (torch.cat([x[i] for x in outs]) for i in range(3))
    if layout == "soa":
        obs = obs.permute(0, 2, 1)
    assert tuple(obs.shape) == (K, n, len(case.names)) and rew.dtype == tdt
    out = (obs.double().cpu().numpy(), r_dev.double().cpu().numpy(), done.cpu().numpy().astype(bool), rew.cpu().numpy(), launch)
    env.close()
    return out


@pytest.mark.parametrize("shape, dtype, K, pipelined, n", RUNS, ids=[f"{s}-{d}-K{k}-{'pipe' if p else 'single'}-n{n}" for s, d, k, p, n in RUNS])
def test_reward_against_the_restatement(shape, dtype, K, pipelined, n, monkeypatch):
    """One launch of K steps with the reward fused in, against the float64 restatement on what the launch returned:
      * |device - restatement| <= 4 x the measured relative error x (|bias| + sum_i w_i d_i ** n_i) per sample, and never more than the
        project's contract (1e-4 x reward scale in float32, 1e-9 in float64); the violation reward exact wherever `done` is set;
      * the launch took the kernel the run names;
      * the SoA layout gives the same reward bits; K == 9: three launches of 3 + 1 + 5 steps give the same bits;
      * every mutant of the restatement that changes this case's formula is at least 100 tolerances away on more than half of the
        non-terminated samples."""
    case = rp.Case(shape)
    if not pipelined and dtype == "float32":
        monkeypatch.setenv("GEMX_PIPE", "0")
    rng = np.random.default_rng(zlib.crc32(f"{shape}-{dtype}-{K}-{pipelined}-{n}".encode()))
    import gym_electric_motor_amd as ga

    probe = ga.make(case.env_id, n_envs=2, _defer_create=True).physical_system
    actions = _random_actions(probe, (K, n), rng)
    refs = rng.uniform(-0.8, 0.8, (K, n, len(case.ref_cols)))
    obs, refs64, done, rew, launch = _run(case, dtype, K, n, "aos", actions, refs)
    # (float32 with K >= 2 is what the pipelined kernel takes; float64 and single steps take the single-wave kernel)
    want_kernel = "advance_pipe_kernel" if (pipelined and dtype == "float32" and K >= 2) else "advance_kernel"
    assert want_kernel in launch, launch
    assert np.isfinite(obs).all() and refs64.dtype == np.float64
    if dtype == "float32":
        assert np.array_equal(refs64, refs.astype(np.float32).astype(np.float64))
    live = ~done
    want = case.reward(obs, refs64, done)
    # the same numbers from the restatement's own entry point, on the full-width arrays the reference's reward function holds
    assert np.array_equal(want, reward(obs, full_references(refs64, case.ref_cols, len(case.names)), done, case.weights, case.powers, case.length,
                                       case.bias, case.violation_reward))
    got = rew.astype(np.float64)
    assert (rew[done] == rew.dtype.type(case.violation_reward)).all()
    if rp.must_terminate(shape, K):
        assert done.any() and live.any(), (int(done.sum()), done.size)
    reward_scale = max(1.0, float(np.abs(want[live]).max())) if live.any() else 1.0
    bound = rp.bound(case, dtype, obs, refs64, reward_scale)
    err = np.abs(got - want)
    scale = case.scale(obs, refs64)
    ratio = float((err[live] / scale[live]).max()) if live.any() and (scale[live] > 0).all() else float("nan")
    print(f"REWARD_PATHS run {shape} {dtype} K={K} {want_kernel} n={n} general={int(case.general)} terminated={int(done.sum())}/{done.size} "
          f"max_rel_err={ratio:.3e} asserted_rel={rp.HEADROOM * rp.MEASURED[(dtype, case.general)]:.3e}")
    assert (err[live] <= bound[live]).all(), (ratio, float(err[live].max()))
    # sensitivity: what this run would have caught
    mutants = case.mutants()
    assert mutants, shape
    right = case.bias - case.terms(obs, refs64).sum(axis=-1)
    for name, f in mutants.items():
        far = np.abs(f(obs, refs64) - right)[live] >= rp.MUTANT_FACTOR * bound[live]
        sep = float(np.median(np.abs(f(obs, refs64) - right)[live] / np.maximum(bound[live], 1e-300))) if live.any() else float("nan")
        print(f"REWARD_PATHS mutant {shape} {dtype} K={K} '{name}' fraction_separated={far.mean() if live.any() else float('nan'):.3f} median_tolerances={sep:.2e}")
        assert live.any() and far.mean() > 0.5, (name, float(far.mean()) if live.any() else None)
    # layout and chunking: the same bits
    obs_s, _, done_s, rew_s, _ = _run(case, dtype, K, n, "soa", actions, refs)
    assert np.array_equal(rew_s, rew) and np.array_equal(done_s, done) and np.array_equal(obs_s, obs)
    if K == 9:
        obs_c, _, done_c, rew_c, _ = _run(case, dtype, K, n, "aos", actions, refs, chunks=[3, 1, 5])
        assert np.array_equal(rew_c, rew) and np.array_equal(done_c, done) and np.array_equal(obs_c, obs)


def test_every_mutant_and_every_path_is_covered():
    """The mutants a case leaves out are those that do not change its formula; between them the runs still apply every mutant many
    times, and every path of the device code has its cases."""
    mutant_runs, path_cases = {}, {}
    for shape, dtype, K, pipelined, n in RUNS:
        for m in rp.Case(shape).mutants():
            mutant_runs[m] = mutant_runs.get(m, 0) + 1
    for shape in rp.SHAPES:
        for p, on in rp.Case(shape).paths.items():
            if on:
                path_cases.setdefault(p, []).append(shape)
    assert set(mutant_runs) == {"all lengths 2", "len[t] for len[col]", "terms t >= 4 dropped", "two powers swapped", "un-referenced term against a reference"}
    assert min(mutant_runs.values()) >= 25, mutant_runs
    assert set(path_cases) == {"hot", "beyond-hot", "general", "general beyond-hot", "n_ref 0", "n_ref 4", "length 1"}
    assert all(len(v) >= 2 for v in path_cases.values()), path_cases
    for K in rp.K_VALUES:  # every K through both kernels in float32
        assert {p for s, d, k, p, n in RUNS if k == K and d == "float32"} == {True, False}
    assert {k for s, d, k, p, n in RUNS if d == "float64"} == set(rp.K_VALUES)
    assert sum(rp.must_terminate(s, k) for s, d, k, p, n in RUNS) >= 3
    for p, v in sorted(path_cases.items()):
        print(f"REWARD_PATHS path '{p}': {', '.join(v)}")


@pytest.mark.parametrize("env_id", sorted(rp.DEFAULTS))
def test_default_reward_of_every_env_id(env_id):
    """`make(env_id, reference_generator="default", reward_function="default")` for each of the 54 ids, 64 steps of random actions: at
    every step the returned reward against the restatement fed with the returned state, the reference shown BEFORE the step, `terminated`
    and the recorded defaults of the reference's env class (weights, powers, bias, violation reward, `_state_length`).  The project's
    contract: 1e-4 x reward scale (the largest |reward| outside terminations, at least 1), the violation reward exact; references stay
    inside the recorded reference space.  The speed-control ids of the series and shunt machines and the torque-control ids of the
    series machine divide by a length of 1."""
    import gym_electric_motor_amd as ga

    want = rp.DEFAULTS[env_id]
    n, K = 70, 64
    env = ga.make(env_id, n_envs=n, reference_generator="default", reward_function="default", seed=zlib.crc32(env_id.encode()) & 0xFFFF)
    ps = env.physical_system
    names = [s for s in want["state_names"] if s != "i_sum"]  # (a column the reference's shunt envs append; weight 0, asserted below)
    keep = [want["state_names"].index(s) for s in names]
    assert list(ps.state_names) == names and list(env.reference_names) == want["reference_names"]
    rw = want["reward"]
    w, pw, length = (np.array(rw[k])[keep] for k in ("_reward_weights", "_n", "_state_length"))
    assert all(rw["_reward_weights"][i] == 0.0 for i in range(len(want["state_names"])) if i not in keep)
    cols = [names.index(s) for s in want["reference_names"]]
    assert [names[i] for i in np.nonzero(w)[0]] == want["reference_names"]  # (the defaults weight the referenced states)
    lo, hi = np.array(want["reference_space"]["low"]), np.array(want["reference_space"]["high"])
    rng = np.random.default_rng(zlib.crc32(env_id.encode()))
    (state, ref), _ = env.reset()
    worst, scale, n_term = 0.0, 1.0, 0
    for k in range(K):
        prev = ref.double().cpu().numpy()
        assert (prev >= lo - 1e-6).all() and (prev <= hi + 1e-6).all(), k
        (state, ref), rew, terminated, _, _ = env.step(_random_actions(ps, (n,), rng))
        s, r, t = state.double().cpu().numpy(), rew.double().cpu().numpy(), terminated.cpu().numpy().astype(bool)
        host = reward(s, full_references(prev, cols, len(names)), t, w, pw, length, rw["_bias"], rw["_violation_reward"])
        assert (r[t] == np.float32(rw["_violation_reward"])).all(), k
        if (~t).any():
            scale = max(scale, float(np.abs(host[~t]).max()))
            worst = max(worst, float(np.abs(r - host)[~t].max()))
        n_term += int(t.sum())
    print(f"REWARD_PATHS default {env_id}: lengths {sorted(set(length[w != 0]))} max |reward - restatement| {worst:.3e} (bound {1e-4 * scale:.3e}), {n_term} terminations")
    assert worst < 1e-4 * scale
    env.close()
