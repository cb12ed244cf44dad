"""The policy rollout on the device (csrc/gemx_policy.hip): physics rows bit for bit against `rollout_episodic` fed the returned actions,
the actor element by element against the float64 restatement (tests/policy_restatement.py), live weights under a captured graph, and
interleaving with `step()`.  N = 197: three waves and a tail of five lanes.  The cases are tests/policy_restatement.py's table."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_electric_motor_amd as ga
from gym_electric_motor_amd.policy import device_tanh
import policy_restatement as pr

pytestmark = pytest.mark.gpu
N, K = pr.N_ENVS, pr.K_STEPS
LANES = (0, 63, 64, 65, 196)
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")
DEV = "cuda:0"


def _make(env_id, M, n=N, **kw):
    env = ga.make(env_id, n_envs=n, device=0, max_episode_steps=M, episode_statistics=True, **kw)
    env.reset()
    return env


def _dev(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


def _policy(env_id, plan, act, squash, use_refs, use_noise, seed=3, n=N, k=K):
    layers, columns, refs, noise = pr.case_data(env_id, plan, use_refs, use_noise, seed=seed, n=n, k=k)
    n_state = pr.ENVS[env_id][0]
    return ga.MLPPolicy(layers, activation=act, squash=squash, columns=columns), (columns or list(range(n_state))), _dev(refs), _dev(noise)


def _reset_obs(env, width):
    ps = env.physical_system
    buf = (C.c_double * 24)()
    assert ps._L.gemx_reset_observation(ps._handle, buf) == 0
    return np.array(buf[:width]).astype(np.float32).astype(np.float64)  # (the device holds it in fp32)


def _check_actor(env, layers, activation, squash, cols, obs0, traj, ended, refs, noise, actions):
    obs0, traj, actions = (t.cpu().numpy() for t in (obs0, traj, actions))
    x = pr.inputs(traj, ended, obs0, _reset_obs(env, traj.shape[2]), cols, None if refs is None else refs.cpu().numpy())
    out, err = pr.forward(layers, activation, x, None if noise is None else noise.cpu().numpy())
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


def _same_rows_and_episodes(env, twin, got, want):
    """(traj, terminated, truncated, stats) of the policy rollout against the twin's `rollout_episodic`, then the episode stage's five
    fields and the ODE state."""
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert set(got[3]) == set(want[3])
    for key in want[3]:
        assert torch.equal(got[3][key], want[3][key]), key
    for f in FIELDS:
        assert torch.equal(getattr(env.pipeline.episode, f), getattr(twin.pipeline.episode, f)), f
    assert torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    for lane in LANES:
        assert torch.equal(got[0][:, lane], want[0][:, lane]), lane


SEEN = {}  # (what the suite as a whole must have produced: checked by the test behind the parametrised one)


@pytest.mark.parametrize("env_id,M,plan,act,squash,use_refs,use_noise", pr.cases())
def test_rows_bit_for_bit_and_actor(env_id, M, plan, act, squash, use_refs, use_noise):
    env, twin = _make(env_id, M), _make(env_id, M)
    policy, cols, refs, noise = _policy(env_id, plan, act, squash, use_refs, use_noise)
    obs0 = env.physical_system._obs.clone()
    traj, actions, term, trunc, stats = env.rollout_policy_episodic(policy, K, references=refs, noise=noise, episode_statistics=True)
    want = twin.rollout_episodic(actions, episode_statistics=True)
    torch.cuda.synchronize()
    _same_rows_and_episodes(env, twin, (traj, term, trunc, stats), want)
    term2, trunc2 = want[1], want[2]
    ended = (term2 | trunc2).cpu().numpy()
    if M == 5:
        assert trunc2.any()
    SEEN[("terminated", env_id)] = SEEN.get(("terminated", env_id), False) or bool(term2.any())
    SEEN["restart off lane 0"] = SEEN.get("restart off lane 0", False) or bool((ended != ended[:, :1]).any())
    _check_actor(env, policy.layers, act, squash, cols, obs0, traj, ended, refs, noise, actions)
    env.close(), twin.close()


def test_the_cases_exercised_terminations_and_the_restart_input():
    """From the twins' results of the cases above: PermExDc produced terminations, and at least one env restarted at a row other than
    lane 0's (truncations come in step for every env: only terminations under per-lane noise or references do that)."""
    if ("terminated", "Cont-CC-PermExDc-v0") not in SEEN:  # (run on its own: the PermExDc cases first)
        for case in pr.cases():
            if case[0] == "Cont-CC-PermExDc-v0":
                test_rows_bit_for_bit_and_actor(*case)
    assert SEEN[("terminated", "Cont-CC-PermExDc-v0")] and SEEN["restart off lane 0"]


def test_env_parameters_and_large_batch_blocks():
    """A per-env parameter table (TAB = true), and the 256-lane workgroups of large batches (more than four waves per CU)."""
    n_big = 4 * 304 * 64 + 197
    for env_id, nn, table, k in (("Finite-CC-PMSM-v0", N, True, K), ("Cont-SC-SCIM-v0", n_big, False, 6)):
        extra = {}
        if table:  # every env its own stator resistance
            extra = dict(env_parameters=ga.EnvParameters(motor={"r_s": 18e-3 * np.random.default_rng(5).uniform(0.8, 1.2, nn)}))
        env, twin = _make(env_id, 5, n=nn, **extra), _make(env_id, 5, n=nn, **extra)
        policy, cols, refs, noise = _policy(env_id, "64x64", "tanh", "tanh", False, True, seed=9, n=nn, k=k)
        obs0 = env.physical_system._obs.clone()
        traj, actions, term, trunc, stats = env.rollout_policy_episodic(policy, k, noise=noise, episode_statistics=True)
        launched = env.physical_system.last_launch()
        want = twin.rollout_episodic(actions, episode_statistics=True)
        torch.cuda.synchronize()
        assert "policy_rollout_kernel" in launched and (("tab=1" in launched and "x 64 threads" in launched) if table else ("tab=0" in launched and "x 256 threads" in launched)), launched
        _same_rows_and_episodes(env, twin, (traj, term, trunc, stats), want)
        assert torch.equal(traj[:, nn - 1], want[0][:, nn - 1])
        _check_actor(env, policy.layers, "tanh", "tanh", cols, obs0, traj, (want[1] | want[2]).cpu().numpy(), refs, noise, actions)
        env.close(), twin.close()


def test_weights_are_live_under_a_graph():
    """ONE captured graph: replay (actions follow the old weights), set_weights, replay (actions follow the new ones); the episodes
    continue across the launches as consecutive unbound calls continue them."""
    env_id = "Cont-SC-SCIM-v0"
    env, twin = _make(env_id, 5), _make(env_id, 5)
    policy, cols, _, noise = _policy(env_id, "64x64", "relu", "tanh", False, True, seed=4)
    old_layers = policy.layers
    ns, nl = pr.ENVS[env_id][0], pr.ENVS[env_id][1]
    traj, acts = torch.empty((K, N, ns), device=DEV), torch.empty((K, N, nl), device=DEV)
    term, trunc = torch.empty((K, N), dtype=torch.uint8, device=DEV), torch.empty((K, N), dtype=torch.uint8, device=DEV)
    start = env.physical_system._obs.clone()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch = env.bind_rollout_policy_episodic(policy, K, traj, acts, term, trunc, obs0=start, noise=noise, stream=side)
        launch()  # (outside the capture: loads the unit and builds the handle's one-step map, as a first stepped launch must)
        side.synchronize()
        runs = [[t.clone() for t in (start, traj, acts, term, trunc)]]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    new_layers = pr.make_layers(np.random.default_rng(12), len(cols), (64, 64, nl), scale=2.0)
    for layers in (None, new_layers):  # replay; set_weights; replay again
        if layers is not None:
            policy.set_weights(layers)
        start.copy_(traj[-1])  # (the actor's input at k = 0 is whatever obs0 holds: the last row, every time)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (start, traj, acts, term, trunc)])
    assert not torch.equal(runs[1][2], runs[2][2])
    for (obs0, rows, actions, te, tr), layers in zip(runs, (old_layers, old_layers, policy.layers)):
        want = twin.rollout_episodic(actions)  # consecutive unbound calls: rows, masks, then counters and state
        torch.cuda.synchronize()
        assert torch.equal(rows, want[0]) and torch.equal(te, want[1]) and torch.equal(tr, want[2])
        _check_actor(env, layers, "relu", "tanh", cols, obs0, rows, (te | tr).cpu().numpy(), None, noise, actions)
    for f in FIELDS:
        assert torch.equal(getattr(env.pipeline.episode, f), getattr(twin.pipeline.episode, f)), f
    assert torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    env.close(), twin.close()


def test_interleaving_with_step():
    env_id = "Finite-CC-PMSM-v0"
    env, twin = _make(env_id, 5), _make(env_id, 5)
    policy, cols, refs, noise = _policy(env_id, "16", "relu", "tanh", False, True, seed=6)
    a0 = torch.as_tensor(np.random.default_rng(1).integers(0, 8, N).astype(np.uint8), device=DEV)
    for e in (env, twin):
        e.step(a0)
    traj, actions, term, trunc = env.rollout_policy_episodic(policy, K, noise=noise)
    t2, term2, trunc2 = twin.rollout_episodic(actions)
    r1, r2 = env.step(a0), twin.step(a0)
    torch.cuda.synchronize()
    assert torch.equal(traj, t2) and torch.equal(term, term2) and torch.equal(trunc, trunc2)
    assert torch.equal(r1[0], r2[0]) and torch.equal(env.physical_system.get_state(), twin.physical_system.get_state())
    for f in FIELDS:
        assert torch.equal(getattr(env.pipeline.episode, f), getattr(twin.pipeline.episode, f)), f
    env.close(), twin.close()


def test_device_tanh_error_is_what_the_bound_assumes():
    """The actor's tanh over 2^16 points of [-10, 10] against float64: the measured maximum the restatement's EPS_TANH doubles."""
    env = _make("Cont-SC-SCIM-v0", 5, n=64)
    x = torch.linspace(-10, 10, 2 ** 16, device=DEV, dtype=torch.float32)
    y = device_tanh(env.physical_system, x)
    torch.cuda.synchronize()
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - np.tanh(x.cpu().numpy().astype(np.float64))).max())
    print("device tanh: max abs error", err)
    assert err <= pr.EPS_TANH_MEASURED
    env.close()
