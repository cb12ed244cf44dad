"""The policy rollout of the complete env on the device (csrc/gemx_policy_complete.hip): rows, references, reward, masks, statistics and
the generators' whole state bit for bit against `rollout_complete_episodic` of a twin env fed the returned actions; the actor element by
element against the float64 restatement (tests/policy_restatement.py) on the inputs `[state_prev[columns], refs_prev]`; both generator
kinds; per-env parameters and 256-lane workgroups; live weights under a captured graph; interleaving with `step()` and the other
rollouts.  N = 197: three waves and a tail of five lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_electric_motor_amd as ga
from gym_electric_motor_amd import _lib
from gym_electric_motor_amd.envs import default_env_modules
import policy_restatement as pr

pytestmark = pytest.mark.gpu
N, K = pr.N_ENVS, pr.K_STEPS
LANES = (0, 63, 64, 65, 196)
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")
DEV = "cuda:0"
N_REF = {"Cont-CC-PermExDc-v0": 1, "Finite-CC-PMSM-v0": 2, "Cont-SC-SCIM-v0": 1}


def _generator(env_id, kind, seed=0):
    """'default', or the all-Wiener generator with sub-episodes of 3 to 8 steps: boundaries fall inside the K steps."""
    if kind == "default":
        return "default"
    modules = default_env_modules(env_id)
    return ga.BatchedWienerProcessReferenceGenerator(reference_states=modules["reference_states"], seed=seed, **dict(modules["generator"], episode_lengths=(3, 9)))


def _make(env_id, M, gen, n=N, **kw):
    env = ga.make(env_id, n_envs=n, device=0, max_episode_steps=M, episode_statistics=True, reference_generator=gen() if callable(gen) else gen, **kw)
    env.reset()
    return env


def _policy(env_id, plan, act, squash, seed=3, n=N, k=K):
    """The restatement's plan, columns and noise; the first layer takes the selected columns and the env's n_ref references."""
    n_state, n_logit, _, five, bias = pr.ENVS[env_id]
    hidden, sel = pr.PLANS[plan]
    columns = five if sel == "five" else None
    cols = columns or list(range(n_state))
    layers = pr.make_layers(np.random.default_rng(11), len(cols) + N_REF[env_id], tuple(hidden) + (n_logit,), scale=0.5)
    layers[-1] = (layers[-1][0], (layers[-1][1] + np.float32(bias)).astype(np.float32))
    noise = pr.case_data(env_id, plan, False, True, seed=seed, n=n, k=k)[3]
    return ga.MLPPolicy(layers, activation=act, squash=squash, columns=columns), cols, torch.as_tensor(noise, device=DEV)


def _reset_obs(env, width):
    ps = env.physical_system
    buf = (C.c_double * 24)()
    assert ps._L.gemx_reset_observation(ps._handle, buf) == 0
    return np.array(buf[:width]).astype(np.float32).astype(np.float64)


def _check_actor(env, layers, activation, squash, cols, obs0, shown0, state, refs, ended, noise, actions):
    obs0, shown0, state, refs, actions = (t.cpu().numpy() for t in (obs0, shown0, state, refs, actions))
    refs_prev = np.concatenate([shown0[None], refs[:-1]], axis=0)  # the row shown in front of step k
    x = pr.inputs(state, ended, obs0, _reset_obs(env, state.shape[2]), cols, refs_prev)
    out, err = pr.forward(layers, activation, x, noise.cpu().numpy())
    if actions.dtype == np.uint8:
        idx, excused = pr.finite_action(out, err)
        wrong = (actions != idx) & ~excused
        print("finite: mismatches outside the excuse", int(wrong.sum()), "excused share", float(excused.mean()))
        assert not wrong.any() and excused.mean() <= 0.01
        for lane in LANES:
            assert not wrong[:, lane].any(), lane
    else:
        ref, bound = pr.continuous_action(out, err, squash)
        diff = np.abs(actions.astype(np.float64) - ref)
        print("continuous: max |action - restated|", float(diff.max()), "max ratio to the bound", float((diff / bound).max()))
        assert (diff <= bound).all()
        for lane in LANES:
            assert (diff[:, lane] <= bound[:, lane]).all(), lane


def _blob(env):
    return env.get_checkpoint()["reference_generator"]["blob"]


def _same(env, twin, got, want, stats=True):
    """(state, refs, reward, terminated, truncated[, stats]) against the twin's `rollout_complete_episodic`, then the episode stage's five
    fields, the ODE state, the references shown and the generators' checkpoint blob."""
    for name, a, b in zip(("state", "refs", "reward", "terminated", "truncated"), got[:5], want[:5]):
        assert torch.equal(a, b), name
    if stats:
        assert set(got[5]) == set(want[5])
        for key in want[5]:
            assert torch.equal(got[5][key], want[5][key]), key
    for f in FIELDS:
        assert torch.equal(getattr(env.pipeline.episode, f), getattr(twin.pipeline.episode, f)), f
    assert torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    assert torch.equal(env.reference_generator.references, twin.reference_generator.references)
    assert torch.equal(_blob(env), _blob(twin))
    for lane in LANES:
        for a, b in zip(got[:5], want[:5]):
            assert torch.equal(a[:, lane], b[:, lane]), lane


def _same_step(env, twin, a):
    r1, r2 = env.step(a), twin.step(a)
    torch.cuda.synchronize()
    assert torch.equal(r1[0][0], r2[0][0]) and torch.equal(r1[0][1], r2[0][1])  # (state, ref)
    for x, y in zip(r1[1:4], r2[1:4]):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


def _action(env_id, n=N, seed=1):
    rng = np.random.default_rng(seed)
    if pr.ENVS[env_id][2]:
        return torch.as_tensor(rng.integers(0, pr.ENVS[env_id][1], n).astype(np.uint8), device=DEV)
    return torch.as_tensor(rng.uniform(-1, 1, (n, pr.ENVS[env_id][1])).astype(np.float32), device=DEV)


def _run_case(env_id, M, plan, act, squash, gen, n=N, k=K, seed=3, **kw):
    """One rollout of env and twin -> everything the checks need; the comparisons of case 1 are made here."""
    env, twin = _make(env_id, M, gen, n=n, **kw), _make(env_id, M, gen, n=n, **kw)
    policy, cols, noise = _policy(env_id, plan, act, squash, seed=seed, n=n, k=k)
    obs0, shown0, blob0 = env.physical_system._obs.clone(), env.reference_generator.references.clone(), _blob(env).clone()
    got = env.rollout_policy_complete_episodic(policy, k, noise=noise, episode_statistics=True)
    launched = env.physical_system.last_launch()
    state, refs, reward, actions, term, trunc, stats = got
    want = twin.rollout_complete_episodic(actions, episode_statistics=True)
    torch.cuda.synchronize()
    _same(env, twin, (state, refs, reward, term, trunc, stats), want)
    ended = (term | trunc).cpu().numpy()
    _check_actor(env, policy.layers, act, squash, cols, obs0, shown0, state, refs, ended, noise, actions)
    _same_step(env, twin, _action(env_id, n))
    return env, twin, dict(term=term, trunc=trunc, ended=ended, blob0=blob0, blob1=_blob(env), launched=launched, state=state, want=want)


def _wiener_counters(blob, n, n_ref):
    """(n_sub, n_reset) [n_ref, N] of an all-Wiener checkpoint blob: the header, then value, sigma (8 bytes), left, n_sub, n_reset (4), t (8),
    every section padded to 8 bytes (csrc/gemx_refgen.hip)."""
    raw = blob.cpu().numpy()
    m = n * n_ref
    pad = lambda b: (b + 7) & ~7  # noqa: E731
    at = _lib.REFGEN_BLOB_HEADER_BYTES + 2 * pad(8 * m) + pad(4 * m)
    n_sub = raw[at:at + 4 * m].view(np.uint32).reshape(n_ref, n)
    at += pad(4 * m)
    return n_sub.astype(np.int64), raw[at:at + 4 * m].view(np.uint32).reshape(n_ref, n).astype(np.int64)


def _cases():
    out = []
    for ie, env_id in enumerate(pr.ENVS):
        for im, M in enumerate((5, 1000)):
            for ip, plan in enumerate(pr.PLANS):
                for ig, gen in enumerate(("default", "short")):
                    ia = (ie + ip + ig) % 2  # (activation and squash rotate as pr.cases() rotates them)
                    out.append((env_id, M, plan, ("relu", "tanh")[ia], "clip" if (im + ia) % 2 == 0 else "tanh", gen))
    return out


SEEN = {}


@pytest.mark.parametrize("env_id,M,plan,act,squash,gen", _cases())
def test_rows_references_reward_state_bit_for_bit_and_actor(env_id, M, plan, act, squash, gen):
    env, twin, r = _run_case(env_id, M, plan, act, squash, lambda: _generator(env_id, gen))
    if M == 5:
        assert r["trunc"].any()
    SEEN[("terminated", env_id)] = SEEN.get(("terminated", env_id), False) or bool(r["term"].any())
    SEEN["restart off lane 0"] = SEEN.get("restart off lane 0", False) or bool((r["ended"] != r["ended"][:, :1]).any())
    if gen == "short":  # a sub-episode boundary that is not behind a restart: more new sub-episodes than restarts
        (s0, r0), (s1, r1) = _wiener_counters(r["blob0"], N, N_REF[env_id]), _wiener_counters(r["blob1"], N, N_REF[env_id])
        assert ((s1 - s0) > (r1 - r0)).any()
    env.close(), twin.close()


def test_the_cases_exercised_terminations_and_restarts_off_lane_0():
    if ("terminated", "Cont-CC-PermExDc-v0") not in SEEN:  # (run on its own: the PermExDc cases first)
        for case in _cases():
            if case[0] == "Cont-CC-PermExDc-v0":
                test_rows_references_reward_state_bit_for_bit_and_actor(*case)
    assert SEEN[("terminated", "Cont-CC-PermExDc-v0")] and SEEN["restart off lane 0"]


PROFILES = [(False, "linear", "hold", "zero"), (True, "linear", "wrap", "random"), (False, "hold", "wrap", "random"), (True, "hold", "hold", "zero")]


@pytest.mark.parametrize("per_env,interpolation,end,start", PROFILES)
def test_profile_generator(per_env, interpolation, end, start):
    env_id, T = "Finite-CC-PMSM-v0", 37
    table = np.random.default_rng(21).uniform(-0.8, 0.8, (T, N, 2) if per_env else (T, 2)).astype(np.float32)
    tau = ga.make(env_id, n_envs=1, _defer_create=True).physical_system.tau
    gen = lambda: ga.ProfileReferenceGenerator(table, profile_tau=2.5 * tau, interpolation=interpolation, end=end, start=start, seed=5)  # noqa: E731
    env, twin, r = _run_case(env_id, 5, "64x64", "tanh", "tanh", gen)
    assert r["trunc"].any() and "gen=profile" in r["launched"]
    if start == "random":
        assert bool((env.reference_generator.state()["s"] != 0).any())
    env.close(), twin.close()


def test_env_parameters_and_large_batch_blocks():
    """A per-env parameter table (TAB = true), and the 256-lane workgroups of large batches (more than four waves per CU)."""
    n_big = 4 * 304 * 64 + 197
    for env_id, nn, table, k in (("Finite-CC-PMSM-v0", N, True, K), ("Cont-SC-SCIM-v0", n_big, False, 6)):
        extra = {}
        if table:  # every env its own stator resistance
            extra = dict(env_parameters=ga.EnvParameters(motor={"r_s": 18e-3 * np.random.default_rng(5).uniform(0.8, 1.2, nn)}))
        env, twin, r = _run_case(env_id, 5, "64x64", "tanh", "tanh", "default", n=nn, k=k, seed=9, **extra)
        launched = r["launched"]
        assert "policy_complete_rollout_kernel" in launched and (("tab=1" in launched and "x 64 threads" in launched) if table else ("tab=0" in launched and "x 256 threads" in launched)), launched
        assert torch.equal(r["state"][:, nn - 1], r["want"][0][:, nn - 1])
        env.close(), twin.close()


def test_weights_are_live_under_a_graph():
    """ONE captured graph: replay, set_weights, replay; after each of the three runs the twin's `rollout_complete_episodic(actions)` gives
    the same tensors, and the generators' blobs agree at the end."""
    env_id = "Cont-SC-SCIM-v0"
    env, twin = _make(env_id, 5, "default"), _make(env_id, 5, "default")
    policy, cols, noise = _policy(env_id, "64x64", "relu", "tanh", seed=4)
    ns, nl = pr.ENVS[env_id][0], pr.ENVS[env_id][1]
    state, refs, acts = torch.empty((K, N, ns), device=DEV), torch.empty((K, N, N_REF[env_id]), device=DEV), torch.empty((K, N, nl), device=DEV)
    reward = torch.empty((K, N), device=DEV)
    term, trunc = torch.empty((K, N), dtype=torch.uint8, device=DEV), torch.empty((K, N), dtype=torch.uint8, device=DEV)
    start = env.physical_system._obs.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch = env.bind_rollout_policy_complete_episodic(policy, K, state, refs, reward, acts, term, trunc, obs0=start, noise=noise, stream=side)
        launch()  # (outside the capture: loads the unit and builds the handle's one-step map)
        side.synchronize()
        runs = [[t.clone() for t in (state, refs, reward, acts, term, trunc)]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    new_layers = pr.make_layers(np.random.default_rng(12), len(cols) + N_REF[env_id], (64, 64, nl), scale=2.0)
    for layers in (None, new_layers):
        if layers is not None:
            policy.set_weights(layers)
        start.copy_(state[-1])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (state, refs, reward, acts, term, trunc)])
    assert not torch.equal(runs[1][3], runs[2][3])
    for st, rf, rw, actions, te, tr in runs:
        want = twin.rollout_complete_episodic(actions)
        torch.cuda.synchronize()
        for a, b in zip((st, rf, rw, te, tr), want):
            assert torch.equal(a, b)
    _same(env, twin, runs[-1][:3] + runs[-1][4:], want, stats=False)
    env.close(), twin.close()


def test_interleaving_with_step_and_the_other_rollouts():
    env_id = "Finite-CC-PMSM-v0"
    env, twin = _make(env_id, 5, "default"), _make(env_id, 5, "default")
    policy, cols, noise = _policy(env_id, "16", "relu", "tanh", seed=6)
    a0 = _action(env_id)
    truncated = False
    for _ in range(5):  # (the fifth step reaches M = 5: a reset is pending when the rollout starts)
        r1, r2 = env.step(a0), twin.step(a0)
        truncated = bool(torch.as_tensor(r1[3]).any())
    assert truncated
    obs0 = r1[0][0].clone()  # (the actor's input at k = 0 is whatever obs0 holds; the twin is fed the actions that come of it)
    got = env.rollout_policy_complete_episodic(policy, K, obs0=obs0, noise=noise)
    want = twin.rollout_complete_episodic(got[3])
    random_actions = torch.as_tensor(np.random.default_rng(2).integers(0, 8, (7, N)).astype(np.uint8), device=DEV)
    got2, want2 = env.rollout_complete_episodic(random_actions), twin.rollout_complete_episodic(random_actions)
    torch.cuda.synchronize()
    _same(env, twin, got[:3] + got[4:], want, stats=False)
    for a, b in zip(got2, want2):
        assert torch.equal(a, b)
    _same_step(env, twin, a0)
    assert torch.equal(_blob(env), _blob(twin)) and torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    env.close(), twin.close()


def test_the_physics_only_policy_rollout_is_untouched():
    """`rollout_policy_episodic` with a references tensor does what it did.  On a COMPLETE env with a time limit that is a ValueError, before
    and after this feature: the env's episode stage reads reward rows, which the physics-only families do not produce (the same holds for
    `rollout_episodic` there).  On the physics-only env of the same id it runs the old kernel, and its rows equal `rollout_episodic` of a twin
    fed the returned actions bit for bit."""
    env_id = "Finite-CC-PMSM-v0"
    layers, columns, refs, noise = pr.case_data(env_id, "5col", True, True)
    refs, noise = torch.as_tensor(refs, device=DEV), torch.as_tensor(noise, device=DEV)
    policy = ga.MLPPolicy(layers, activation="tanh", squash="tanh", columns=columns)
    complete = ga.make(env_id, n_envs=N, device=0, max_episode_steps=5, reference_generator="default")
    complete.reset()
    with pytest.raises(ValueError, match="has_reward"):
        complete.rollout_policy_episodic(policy, K, references=refs, noise=noise)
    env, twin = (ga.make(env_id, n_envs=N, device=0, max_episode_steps=5) for _ in range(2))
    env.reset(), twin.reset()
    got = env.rollout_policy_episodic(policy, K, references=refs, noise=noise)
    launched = env.physical_system.last_launch()
    want = twin.rollout_episodic(got[1])
    torch.cuda.synchronize()
    assert "gemx::policy_rollout_kernel" in launched and "libgemx_pl" in launched, launched
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[1]) and torch.equal(got[3], want[2])
    assert torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    complete.close(), env.close(), twin.close()
