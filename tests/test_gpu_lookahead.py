"""The lookahead rollout on the device (csrc/gemx_lookahead.hip): rows, references, reward, masks, the generators' blob and the episode
counters bit for bit against `rollout_complete_episodic` of a twin env fed the returned actions; reward == the chosen action's score;
the scores by brute force (`set_checkpoint`, `step(full(a))` per action); the selection against the numpy restatement; greedy at step 0;
a captured graph; interleaving with `step()`; masking by -inf noise; the library's own refusals.  N = 197: three waves and a tail of
five lanes; N = 330: six workgroups, the last with ten lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_electric_motor_amd as ga
from gym_electric_motor_amd import _lib
from gym_electric_motor_amd.envs import default_env_modules
import lookahead_restatement as lr

pytestmark = pytest.mark.gpu
N, K = 197, 48
LANES = (0, 63, 64, 65, 196)
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")
DEV = "cuda:0"
# a per-env parameter table: every env its own stator / armature resistance, 0.8 to 1.2 times the motor's default (components.py)
RESISTANCE = {"Finite-CC-PMSM-v0": ("r_s", 18e-3), "Finite-TC-ExtExDc-v0": ("r_a", 16e-3), "Finite-SC-SCIM-v0": ("r_s", 2.9338)}
NA = {"Finite-CC-PMSM-v0": 8, "Finite-SC-PermExDc-v0": 4, "Finite-TC-ExtExDc-v0": 16, "Finite-SC-SCIM-v0": 8}


def _generator(env_id, kind, n):
    """'default'; 'short': the all-Wiener generator with sub-episodes of 3 to 8 steps (boundaries inside the K steps); 'profile': a shared
    table of 37 rows with a random start row per episode."""
    modules = default_env_modules(env_id)
    if kind == "default":
        return "default"
    if kind == "short":
        return ga.BatchedWienerProcessReferenceGenerator(reference_states=modules["reference_states"], seed=0, **dict(modules["generator"], episode_lengths=(3, 9)))
    names = list(modules["reference_states"])
    table = np.random.default_rng(5).uniform(-0.5, 0.5, (37, len(names))).astype(np.float32)
    return ga.ProfileReferenceGenerator(table, reference_states=names, end="wrap", start="random", seed=3)


def _make(env_id, M, gen="default", n=N, table=False):
    kw = {}
    if table:
        key, nominal = RESISTANCE[env_id]
        kw = dict(env_parameters=ga.EnvParameters(motor={key: nominal * np.random.default_rng(5).uniform(0.8, 1.2, n)}))
    env = ga.make(env_id, n_envs=n, device=0, max_episode_steps=M, episode_statistics=True, reference_generator=_generator(env_id, gen, n), **kw)
    env.reset()
    return env


def _noise(env_id, n=N, k=K, seed=7):
    """Gumbel noise at the scale of the score differences, with some -inf entries"""
    rng = np.random.default_rng(seed)
    g = (-np.log(-np.log(rng.uniform(1e-6, 1 - 1e-6, (k, n, NA[env_id])))) * 0.05).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = -np.inf
    return torch.as_tensor(g, device=DEV)


def _blob(env):
    return env.get_checkpoint()["reference_generator"]["blob"]


def _same(env, twin, got, want, lanes=LANES):
    """(state, refs, reward, terminated, truncated) against the twin's `rollout_complete_episodic`, then the episode stage's five fields,
    the ODE state, the references shown and the generators' checkpoint blob."""
    for name, a, b in zip(("state", "refs", "reward", "terminated", "truncated"), got, want[:5]):
        assert torch.equal(a, b), name
    for f in FIELDS:
        assert torch.equal(getattr(env.pipeline.episode, f), getattr(twin.pipeline.episode, f)), f
    assert torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    assert torch.equal(env.reference_generator.references, twin.reference_generator.references)
    assert torch.equal(_blob(env), _blob(twin))
    for lane in lanes:
        for a, b in zip(got, want[:5]):
            assert torch.equal(a[:, lane], b[:, lane]), lane


def _same_step(env, twin, a):
    r1, r2 = env.step(a), twin.step(a)
    torch.cuda.synchronize()
    assert torch.equal(r1[0][0], r2[0][0]) and torch.equal(r1[0][1], r2[0][1])  # (state, ref)
    for x, y in zip(r1[1:4], r2[1:4]):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


def _rows_and_reward(env_id, M, gen, noisy, n=N, k=K, table=False, lanes=LANES):
    """Tests 1, 2 and the selection of 3 on one rollout -> (env, twin, outputs, noise)"""
    env, twin = _make(env_id, M, gen, n, table), _make(env_id, M, gen, n, table)
    noise = _noise(env_id, n, k) if noisy else None
    state, refs, reward, actions, term, trunc, scores = env.rollout_lookahead_complete_episodic(k, noise=noise, return_scores=True)
    launched = env.physical_system.last_launch()
    want = twin.rollout_complete_episodic(actions)
    torch.cuda.synchronize()
    assert "lookahead_rollout_kernel" in launched and "libgemx_la" in launched and f"tab={int(table)}" in launched, launched
    assert f"gen={'profile' if gen == 'profile' else 'wiener'}" in launched, launched
    assert actions.dtype == torch.uint8 and tuple(scores.shape) == (k, n, NA[env_id]) and int(actions.max()) < NA[env_id]
    _same(env, twin, (state, refs, reward, term, trunc), want, lanes)
    # 2. the reward pass's reward of the stored row is the chosen action's score
    chosen = torch.gather(scores, 2, actions.long().unsqueeze(2)).squeeze(2)
    assert torch.equal(reward.view(torch.int32), chosen.view(torch.int32))
    # 3 (selection). the action is the restated rule's choice on scores + noise
    picked = lr.select(lr.noisy(scores.cpu().numpy(), None if noise is None else noise.cpu().numpy()))
    assert np.array_equal(picked, actions.cpu().numpy())
    if M == 5:
        assert trunc.any()
    else:
        assert not trunc.any()
    return env, twin, (state, refs, reward, actions, term, trunc, scores), noise


CASES = [("Finite-CC-PMSM-v0", 5, "default", True, False), ("Finite-CC-PMSM-v0", 1000, "short", False, False), ("Finite-CC-PMSM-v0", 5, "profile", True, True),
         ("Finite-SC-PermExDc-v0", 5, "short", False, False), ("Finite-SC-PermExDc-v0", 1000, "profile", True, False),
         ("Finite-TC-ExtExDc-v0", 5, "default", True, False), ("Finite-TC-ExtExDc-v0", 1000, "profile", False, True),
         ("Finite-SC-SCIM-v0", 5, "profile", False, False), ("Finite-SC-SCIM-v0", 1000, "default", True, True), ("Finite-SC-SCIM-v0", 5, "short", True, False)]


@pytest.mark.parametrize("env_id,M,gen,noisy,table", CASES, ids=[f"{e}-M{m}-{g}{'-noise' if z else ''}{'-table' if t else ''}" for e, m, g, z, t in CASES])
def test_rows_reward_and_selection(env_id, M, gen, noisy, table):
    env, twin, out, _ = _rows_and_reward(env_id, M, gen, noisy, table=table)
    if table:  # the per-env values are felt: the same actions on the env's own parameters give other rows
        plain = _make(env_id, M, gen)
        assert not torch.equal(plain.rollout_complete_episodic(out[3])[0], out[0])
        plain.close()
    _same_step(env, twin, torch.zeros(N, dtype=torch.uint8, device=DEV))  # `step()` continues the same episodes
    env.close(), twin.close()


def test_several_workgroups_with_a_partial_last_one():
    n = 330
    env, twin, _, _ = _rows_and_reward("Finite-CC-PMSM-v0", 5, "default", True, n=n, k=12, lanes=(0, 63, 64, 319, 320, 329))
    env.close(), twin.close()


@pytest.mark.parametrize("env_id", list(NA))
def test_scores_by_brute_force(env_id):
    """At the first step, one right behind a restart and the last step: a twin brought to step k, then per action `set_checkpoint` and
    `step(full(a))` -- the reward it returns is scores[k, :, a] bit for bit.  Greedy at step 0 rides along: without noise reward[0] is at
    least a random-action twin's reward at step 0, element by element."""
    M = 5
    env, twin, out, noise = _rows_and_reward(env_id, M, "default", True)
    state, refs, reward, actions, term, trunc, scores = out
    twin.close()
    ended = (term | trunc).cpu().numpy()
    behind_restart = 1 + int(np.argmax(ended[:-1].any(axis=1)))
    assert ended[behind_restart - 1].any()
    for k in (0, behind_restart, K - 1):
        probe = _make(env_id, M)
        if k:
            probe.rollout_complete_episodic(actions[:k])
        ck = probe.get_checkpoint()
        for a in range(NA[env_id]):
            probe.set_checkpoint(ck)
            r = probe.step(torch.full((N,), a, dtype=torch.uint8, device=DEV))[1]
            torch.cuda.synchronize()
            assert torch.equal(r.view(torch.int32), scores[k, :, a].view(torch.int32)), (k, a)
        probe.close()
    env.close()
    # greedy at step 0, without noise
    env, rand = _make(env_id, M), _make(env_id, M)
    greedy = env.rollout_lookahead_complete_episodic(1)[2][0].clone()
    a = torch.as_tensor(np.random.default_rng(9).integers(0, NA[env_id], N).astype(np.uint8), device=DEV)
    other = rand.step(a)[1]
    torch.cuda.synchronize()
    assert bool((greedy >= other).all())
    env.close(), rand.close()


def test_masking():
    """a -inf column in the noise never appears in the actions; with all but one masked the one is always taken"""
    env_id = "Finite-CC-PMSM-v0"
    env = _make(env_id, 5)
    free = env.rollout_lookahead_complete_episodic(K)[3].clone()
    env.close()
    column = int(np.bincount(free.cpu().numpy().ravel(), minlength=8).argmax())  # the action the controller likes best
    env = _make(env_id, 5)
    noise = torch.zeros((K, N, 8), device=DEV)
    noise[:, :, column] = -np.inf
    masked = env.rollout_lookahead_complete_episodic(K, noise=noise)[3]
    assert not bool((masked == column).any()) and bool((free == column).any())
    noise.fill_(-np.inf)
    noise[:, :, 5] = 0.0
    only = env.rollout_lookahead_complete_episodic(K, noise=noise)[3]
    assert bool((only == 5).all())
    env.close()


def test_one_captured_graph_and_interleaving_with_step():
    """ONE captured graph of the bound launch, replayed twice, equals two eager calls of a twin; `step()` in between and behind continues
    the same episodes."""
    env_id = "Finite-SC-PermExDc-v0"
    env, twin = _make(env_id, 5, "short"), _make(env_id, 5, "short")
    ns, n_ref, na = len(env.physical_system.state_names), len(env.reference_names), NA[env_id]
    noise = _noise(env_id)
    state, refs, reward, scores = torch.empty((K, N, ns), device=DEV), torch.empty((K, N, n_ref), device=DEV), torch.empty((K, N), device=DEV), torch.empty((K, N, na), device=DEV)
    acts, term, trunc = (torch.empty((K, N), dtype=torch.uint8, device=DEV) for _ in range(3))
    a0 = torch.as_tensor(np.random.default_rng(1).integers(0, na, N).astype(np.uint8), device=DEV)
    for _ in range(5):  # (the fifth step reaches M = 5: a reset is pending when the first rollout starts)
        _same_step(env, twin, a0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch = env.bind_rollout_lookahead_complete_episodic(K, state, refs, reward, acts, term, trunc, noise=noise, scores_out=scores, stream=side)
        result = launch()  # (outside the capture: loads the unit and builds the handle's one-step map)
        assert result[3] is acts and result[6] is scores
        side.synchronize()
        runs = [[t.clone() for t in (state, refs, reward, acts, term, trunc, scores)]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (state, refs, reward, acts, term, trunc, scores)])
    assert not torch.equal(runs[1][0], runs[2][0])
    for run in runs:
        want = twin.rollout_lookahead_complete_episodic(K, noise=noise, return_scores=True)  # eager
        torch.cuda.synchronize()
        for a, b in zip(run, want):
            assert torch.equal(a, b)
    _same(env, twin, runs[-1][:3] + runs[-1][4:6], [want[0], want[1], want[2], want[4], want[5]])
    _same_step(env, twin, a0)
    got, want = env.rollout_lookahead_complete_episodic(7), twin.rollout_lookahead_complete_episodic(7)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    _same_step(env, twin, a0)
    env.close(), twin.close()


def test_the_librarys_own_refusals():
    """Python's checks bypassed: gemx_rollout_lookahead_complete on real handles."""
    L = _lib.load()
    L.gemx_last_error.restype = C.c_char_p

    def call_of(env, k=4, **over):
        call = _lib.GemxPolicyCall()
        ep = env.pipeline.episode
        call.struct_size, call.K, call.n_cols, call.n_ref, call.max_steps = C.sizeof(call), k, 0, len(env.reference_names), ep.max_steps
        n, ns = env.physical_system.n_envs, len(env.physical_system.state_names)
        keep = dict(raw=torch.empty((k, n, ns), device=DEV), refs=torch.empty((k, n, call.n_ref), device=DEV), acts=torch.empty((k, n), dtype=torch.uint8, device=DEV))
        call.refs_dev, call.length_dev, call.obs_out_dev = env._refs.data_ptr(), ep.length.data_ptr(), keep["raw"].data_ptr()
        for name, value in over.items():
            setattr(call, name, value)
        return call, keep

    def refused(env, word, refgen=True, refs_out=True, **over):
        call, keep = call_of(env, **over)
        gen = env.reference_generator._handle
        rc = L.gemx_rollout_lookahead_complete(env.physical_system._handle, C.byref(call), C.c_void_p(keep["refs"].data_ptr()) if refs_out else None,
                                               C.c_void_p(keep["acts"].data_ptr()), None, None, gen if refgen else None, None, None)
        msg = L.gemx_last_error().decode()
        assert rc != 0 and "lookahead rollout" in msg and word in msg, (rc, msg)

    cont = _make("Cont-CC-PMSM-v0", 5, n=64)
    refused(cont, "continuous converter")
    cont.close()
    env = _make("Finite-CC-PMSM-v0", 5, n=64)
    before, blob = env.physical_system.get_state().clone(), _blob(env).clone()
    refused(env, "K must be", K=0)
    refused(env, "max_steps", max_steps=0)
    refused(env, "actor fields", n_cols=1)
    refused(env, "exactly one", refgen=False)
    refused(env, "refs_out_dev", refs_out=False)
    refused(env, "n_ref", n_ref=1)
    refused(env, "16-byte aligned", obs_out_dev=env._refs.data_ptr() + 4)
    torch.cuda.synchronize()
    assert torch.equal(before, env.physical_system.get_state()) and torch.equal(blob, _blob(env))  # nothing was launched
    env.close()
    euler_dp = ga.make("Finite-CC-PMSM-v0", n_envs=64, device=0, max_episode_steps=5, reference_generator="default", converter=dict(interlocking_time=1e-6))
    euler_dp.reset()
    call, keep = call_of(euler_dp)
    rc = L.gemx_rollout_lookahead_complete(euler_dp.physical_system._handle, C.byref(call), C.c_void_p(keep["refs"].data_ptr()), C.c_void_p(keep["acts"].data_ptr()), None, None,
                                           euler_dp.reference_generator._handle, None, None)
    assert rc != 0 and "lookahead rollout: a converter interlocking time" in L.gemx_last_error().decode()
    euler_dp.close()
