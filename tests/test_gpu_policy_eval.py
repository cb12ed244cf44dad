"""The policy evaluation pass on the device (csrc/gemx_policy_eval.hip): `out` reproduces the policy rollout's actions bit for bit and
lies within the float64 forward bound; the heads against the float64 restatement (tests/policy_eval_restatement.py); `last` and
mode="next"; the shapes at which the kernel takes another path."""
import ctypes as C

import numpy as np
import pytest
import torch

import gym_electric_motor_amd as ga
from gym_electric_motor_amd.policy import device_tanh
import policy_eval_restatement as per
import policy_restatement as pr

pytestmark = pytest.mark.gpu
N, K = pr.N_ENVS, pr.K_STEPS
DEV = "cuda:0"


def _make(env_id, M, n=N, **kw):
    env = ga.make(env_id, n_envs=n, device=0, max_episode_steps=M, episode_statistics=True, **kw)
    env.reset()
    return env


def _dev(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


def _reset_obs(env, width):
    ps = env.physical_system
    buf = (C.c_double * 24)()
    assert ps._L.gemx_reset_observation(ps._handle, buf) == 0
    return np.array(buf[:width]).astype(np.float32)


def _reproduces(env, policy, squash, out, noise, actions):
    """The action recomputed from the evaluated `out` equals the stored one at every row, bit for bit."""
    v = out if noise is None else out + noise
    if actions.dtype == torch.uint8:
        assert torch.equal(torch.argmax(v, dim=2).to(torch.uint8), actions)  # (the lowest index among the maxima)
    elif squash == "clip":
        assert torch.equal(torch.clamp(v, -1.0, 1.0), actions)
    else:
        assert torch.equal(device_tanh(env.physical_system, v.contiguous()), actions)


def _case(env_id, M, plan, act, squash, use_refs, use_noise):
    """One case of the policy rollout's table: `out` reproduces the stored actions and lies within the forward bound -> which of a
    terminated row, a truncated row and a row behind an ended one (the reset substitution) the run had."""
    env = _make(env_id, M)
    layers, columns, refs, noise = pr.case_data(env_id, plan, use_refs, use_noise)
    policy = ga.MLPPolicy(layers, activation=act, squash=squash, columns=columns)
    refs, noise = _dev(refs), _dev(noise)
    obs0 = env.physical_system._obs.clone()
    outs = env.rollout_policy_episodic(policy, K, references=refs, noise=noise, episode_statistics=True)
    traj, actions, term, trunc, stats = outs
    out = env.evaluate_policy_rollout(policy, outs, head="none", obs0=obs0, references=refs)
    torch.cuda.synchronize()
    assert out.shape == (K, N, policy.n_out) and out.dtype == torch.float32
    _reproduces(env, policy, squash, out, noise, actions)
    ended = stats["ended"]
    # within the forward bound of the float64 MLP on the restatement's inputs (the existing actor check's rule: no element outside it)
    cols = columns or list(range(traj.shape[2]))
    x = per.inputs(traj.cpu().numpy(), cols, obs0=obs0.cpu().numpy(), ended=ended.cpu().numpy(), reset_obs=_reset_obs(env, traj.shape[2]),
                   references=None if refs is None else refs.cpu().numpy())
    want, err = per.forward(layers, act, x)
    diff = np.abs(out.cpu().numpy().astype(np.float64) - want)
    print("max |out - float64|", float(diff.max()), "max ratio to the bound", float((diff / err).max()))
    assert (diff <= err).all()
    env.close()
    return {w for w, t in (("terminated", term), ("truncated", trunc), ("restart", ended[:-1])) if bool(t.any())}


@pytest.mark.parametrize("env_id,M,plan,act,squash,use_refs,use_noise", pr.cases())
def test_out_reproduces_the_rollouts_actions_bit_for_bit(env_id, M, plan, act, squash, use_refs, use_noise):
    _case(env_id, M, plan, act, squash, use_refs, use_noise)


def test_the_reset_substitution_is_reached_by_terminations_and_truncations():
    """The PermExDc cases under noise, run here: between them a terminated row, a truncated row and a row whose input is the reset
    observation -- the reproduction above is asserted on all of them."""
    seen = set()
    for case in pr.cases():
        if case[0] == "Cont-CC-PermExDc-v0" and case[6]:
            seen |= _case(*case)
    assert seen == {"terminated", "truncated", "restart"}, seen


@pytest.mark.parametrize("generator", ["default", "profile"])
@pytest.mark.parametrize("M", [5, 1000])
def test_complete_form_reproduces_the_actions(generator, M):
    env_id = "Cont-SC-SCIM-v0"
    kw = {"reference_generator": "default"}
    if generator == "profile":
        table = np.random.default_rng(21).uniform(-0.8, 0.8, (37, 1)).astype(np.float32)
        tau = ga.make(env_id, n_envs=1, _defer_create=True).physical_system.tau
        kw["reference_generator"] = ga.ProfileReferenceGenerator(table, profile_tau=2.5 * tau, interpolation="linear", end="wrap", start="random", seed=5)
    env = ga.make(env_id, n_envs=N, device=0, max_episode_steps=M, episode_statistics=True, **kw)
    obs = env.reset()
    n_ref = len(env.reference_names)
    obs0, shown0 = env.physical_system._obs.clone(), env._refs.clone()
    layers = pr.make_layers(np.random.default_rng(11), 14 + n_ref, (24, 40, 3), scale=0.5)
    policy = ga.MLPPolicy(layers, activation="tanh", squash="tanh")
    noise = _dev(pr.case_data(env_id, "64x64", False, True)[3])
    outs = env.rollout_policy_complete_episodic(policy, K, noise=noise, episode_statistics=True)
    state, refs, reward, actions, term, trunc, stats = outs
    out = env.evaluate_policy_complete_rollout(policy, outs, head="none", obs0=obs0, shown0=shown0)
    torch.cuda.synchronize()
    _reproduces(env, policy, "tanh", out, noise, actions)
    if M == 5:
        assert bool(trunc.any()) and bool(stats["ended"][:-1].any())
    # the complete form's row K (r[K] = refs[K-1]) and mode="next" (r[k] = refs[k]): the same bits where the rows coincide, and every
    # element within the forward bound of the float64 MLP on the restatement's inputs
    out2, out_last = env.evaluate_policy_complete_rollout(policy, outs, head="none", last=True, obs0=obs0, shown0=shown0)
    nxt = env.evaluate_policy_complete_rollout(policy, outs, head="none", mode="next")
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    ended = stats["ended"].cpu().numpy()
    np_ = lambda t: t.cpu().numpy()  # noqa: E731
    x = per.inputs(np_(state), list(range(14)), "seen", True, obs0=np_(obs0), ended=ended, reset_obs=_reset_obs(env, 14), refs=np_(refs), shown0=np_(shown0))
    want, err = per.forward(layers, "tanh", x)
    got = torch.cat([out, out_last[None]], dim=0).cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= err).all()
    want_n, err_n = per.forward(layers, "tanh", per.inputs(np_(state), list(range(14)), "next", refs=np_(refs)))
    assert (np.abs(np_(nxt).astype(np.float64) - want_n) <= err_n).all()
    following = np.concatenate([np_(out)[1:], np_(out_last)[None]], axis=0)
    assert np.array_equal(np_(nxt)[~ended.astype(bool)], following[~ended.astype(bool)])
    env.close()


def _rollout(env_id, n_out_policy=None, M=5, k=K, n=N, seed=3):
    env = _make(env_id, M, n=n)
    layers, columns, _, noise = pr.case_data(env_id, "16", False, True, seed=seed, n=n, k=k)
    policy = ga.MLPPolicy(layers, activation="tanh", squash="tanh")
    obs0 = env.physical_system._obs.clone()
    noise = _dev(noise)
    outs = env.rollout_policy_episodic(policy, k, noise=noise, episode_statistics=True)
    return env, policy, obs0, noise, outs


def _close(got, want):
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12), float(np.abs(got - want).max())


def _once_rounded(got32, got64):
    want = got64.astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got32.astype(np.float64) - want.astype(np.float64)) <= ulp).all()


def test_categorical_head():
    env, policy, obs0, noise, outs = _rollout("Finite-CC-PMSM-v0")
    out = env.evaluate_policy_rollout(policy, outs, head="none", obs0=obs0).cpu().numpy()
    lp64, h64 = env.evaluate_policy_rollout(policy, outs, head="categorical", obs0=obs0, dtype=torch.float64)
    lp32, h32 = env.evaluate_policy_rollout(policy, outs, head="categorical", obs0=obs0)
    torch.cuda.synchronize()
    wlp, wh = per.categorical(out, outs[1].cpu().numpy())
    _close(lp64.cpu().numpy(), wlp)
    _close(h64.cpu().numpy(), wh)
    assert lp32.dtype == torch.float32
    _once_rounded(lp32.cpu().numpy(), lp64.cpu().numpy())
    _once_rounded(h32.cpu().numpy(), h64.cpu().numpy())
    env.physical_system.check_errors()
    # an action outside the policy's outputs: the handle's error word, as any bad action
    bad = outs[1].clone()
    bad[3, 7] = 200
    lp, _ = policy.evaluate_rollout(outs[0], head="categorical", obs0=obs0, ended=outs[4]["ended"], reset_obs=_dev(_reset_obs(env, 14)), actions=bad,
                                    system=env.physical_system)
    with pytest.raises(AssertionError):
        env.physical_system.check_errors()
    assert bool(torch.isnan(lp[3, 7])) and int(torch.isnan(lp).sum()) == 1
    env.close()


@pytest.mark.parametrize("correction", [False, True])
def test_gaussian_head(correction):
    env, policy, obs0, noise, outs = _rollout("Cont-SC-SCIM-v0")
    out = env.evaluate_policy_rollout(policy, outs, head="none", obs0=obs0)
    pre = (out + noise).contiguous()
    log_std = torch.tensor([-0.5, 0.1, -1.3], device=DEV)
    kw = dict(head="gaussian", obs0=obs0, pre_squash=pre, log_std=log_std, squash_correction=correction)
    lp64, h64 = env.evaluate_policy_rollout(policy, outs, dtype=torch.float64, **kw)
    lp32, h32 = env.evaluate_policy_rollout(policy, outs, **kw)
    torch.cuda.synchronize()
    wlp, wh = per.gaussian(out.cpu().numpy(), pre.cpu().numpy(), log_std.cpu().numpy(), correction)
    _close(lp64.cpu().numpy(), wlp)
    _close(h64.cpu().numpy(), wh)
    _once_rounded(lp32.cpu().numpy(), lp64.cpu().numpy())
    _once_rounded(h32.cpu().numpy(), h64.cpu().numpy())
    env.close()


def test_value_head_last_and_next_feed_the_advantages():
    env, policy, obs0, noise, outs = _rollout("Cont-SC-SCIM-v0")
    traj, actions, term, trunc, stats = outs
    ended = stats["ended"]
    critic = ga.MLPPolicy(pr.make_layers(np.random.default_rng(4), 14, (24, 40, 1)), activation="tanh")
    reset = _dev(_reset_obs(env, 14))
    value, last_value = critic.evaluate_rollout(traj, head="value", last=True, obs0=obs0, ended=ended, reset_obs=reset)
    final_value = critic.evaluate_rollout(traj, head="value", mode="next")
    out, out_last = critic.evaluate_rollout(traj, head="none", last=True, obs0=obs0, ended=ended, reset_obs=reset)
    v64 = critic.evaluate_rollout(traj, head="value", obs0=obs0, ended=ended, reset_obs=reset, dtype=torch.float64)
    torch.cuda.synchronize()
    assert torch.equal(value, out[..., 0]) and torch.equal(last_value, out_last[..., 0]) and torch.equal(v64, value.double())
    # last=True: the (K + 1)-row problem built on the host, whose rows 1 .. K are "seen" rows of a trajectory shifted by one
    longer = torch.cat([traj, traj[-1:]], dim=0).contiguous()
    longer_ended = torch.cat([ended, ended[-1:]], dim=0).contiguous()
    v_long = critic.evaluate_rollout(longer, head="value", obs0=obs0, ended=longer_ended, reset_obs=reset)
    assert torch.equal(v_long[:K], value) and torch.equal(v_long[K], last_value)
    # next equals seen of the following step where the episode went on, and differs exactly where it ended
    following = torch.cat([value[1:], last_value[None]], dim=0)
    same = final_value == following
    e = ended.bool()
    assert bool(same[~e].all())
    # on the device: every row of final_value is the MLP of traj[k] and every row of `following` the MLP of the seen input, each within
    # its forward bound -- at the ended rows these are different inputs (below), and the outputs differ there
    x_next = per.inputs(traj.cpu().numpy(), list(range(14)), "next")
    for got, x in ((final_value, x_next), (following, per.inputs(traj.cpu().numpy(), list(range(14)), "seen", True, obs0=obs0.cpu().numpy(), ended=ended.cpu().numpy(),
                                                               reset_obs=reset.cpu().numpy())[1:])):
        want, err = per.forward(critic.layers, "tanh", x)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want[..., 0]) <= err[..., 0]).all()
    assert bool(e.any()) and not bool(same[e].any())
    x_seen = per.inputs(traj.cpu().numpy(), list(range(14)), "seen", True, obs0=obs0.cpu().numpy(), ended=ended.cpu().numpy(), reset_obs=reset.cpu().numpy())[1:]
    assert np.array_equal((x_next != x_seen).any(axis=2), e.cpu().numpy())
    # the three into ga.advantages: bit for bit the numpy restatement of gemx_returns_rows' row function on the same arrays
    reward = torch.rand(K, N, device=DEV)
    adv, ret = ga.advantages(reward, value, term, gamma=0.99, lam=0.95, last_value=last_value, ended=ended, final_value=final_value)
    torch.cuda.synchronize()
    r, v, lv, fv = (t.cpu().numpy().astype(np.float64) for t in (reward, value, last_value, final_value))
    tm, en = term.cpu().numpy().astype(bool), e.cpu().numpy()
    A, above = np.zeros(N), lv
    want_a, want_r = np.zeros((K, N)), np.zeros((K, N))
    for k in range(K - 1, -1, -1):
        v_next = np.where(en[k], np.where(~tm[k], fv[k], 0.0), above)
        delta = (r[k] + 0.99 * v_next) - v[k]
        A = np.where(en[k], delta, delta + (0.99 * 0.95) * A)
        want_a[k], want_r[k] = A, A + v[k]
        above = v[k]
    assert np.array_equal(adv.cpu().numpy(), want_a.astype(np.float32)) and np.array_equal(ret.cpu().numpy(), want_r.astype(np.float32))
    env.close()


@pytest.mark.parametrize("n,k", [(N, 1), (1, 7), (78021, 2)])
def test_shapes(n, k):
    """K = 1 (only obs0 is read), N = 1, and 78021 envs x 2 rows: several tiles per workgroup and a partial last tile."""
    env, policy, obs0, noise, outs = _rollout("Cont-SC-SCIM-v0", n=n, k=k, M=1 if k > 1 else 5)
    out = env.evaluate_policy_rollout(policy, outs, head="none", obs0=obs0)
    torch.cuda.synchronize()
    _reproduces(env, policy, "tanh", out, noise, outs[1])
    env.close()


def test_column_subset_out_of_order_and_the_widest_plan():
    """`columns` a strict subset in non-ascending order; input width 48 with widths 64 x 64 x 64, the limits."""
    rng = np.random.default_rng(9)
    S, n, k = 24, 130, 3
    traj, obs0 = torch.randn(k, n, S, device=DEV), torch.randn(n, S, device=DEV)
    ended = (torch.rand(k, n, device=DEV) < 0.3).to(torch.uint8)
    reset = torch.randn(n, S, device=DEV)  # (per env)
    for cols, n_ref, widths in (([20, 3, 11, 0, 7], 2, (24, 40, 3)), (list(range(23, -1, -1)), 4, (64, 64, 64))):
        # the widest plan reads 24 columns + 4 references = 28 inputs of the 48 a policy may have: a stored row has at most 24 columns
        refs, last_refs = torch.randn(k, n, n_ref, device=DEV), torch.randn(n, n_ref, device=DEV)
        layers = pr.make_layers(rng, len(cols) + n_ref, widths)
        policy = ga.MLPPolicy(layers, activation="relu", columns=cols)
        out, out_last = policy.evaluate_rollout(traj, last=True, obs0=obs0, ended=ended, reset_obs=reset, references=refs, last_references=last_refs)
        torch.cuda.synchronize()
        x = per.inputs(traj.cpu().numpy(), cols, "seen", True, obs0=obs0.cpu().numpy(), ended=ended.cpu().numpy(), reset_obs=reset.cpu().numpy(),
                       references=refs.cpu().numpy(), last_references=last_refs.cpu().numpy())
        want, err = per.forward(layers, "relu", x)
        got = torch.cat([out, out_last[None]], dim=0).cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= err).all()
        # ascending column order in the chain: the same policy with its columns (and weight columns) sorted gives the same bits
        order = np.argsort(cols)
        W0 = layers[0][0]
        W0s = np.concatenate([W0[:, order], W0[:, len(cols):]], axis=1)
        twin = ga.MLPPolicy([(W0s, layers[0][1])] + layers[1:], activation="relu", columns=sorted(cols))
        out2, _ = twin.evaluate_rollout(traj, last=True, obs0=obs0, ended=ended, reset_obs=reset, references=refs, last_references=last_refs)
        assert torch.equal(out, out2)


def test_one_graph_rollout_critic_advantages_and_log_probs():
    """ONE captured graph: the complete policy rollout -> the critic's value and last_value (last=True) -> ga.bind_advantages -> the
    actor's Gaussian log-probs.  Two replays, then new critic weights and new log_std values, then a third: every run equals the eager
    sequence on a twin env bit for bit, and the third differs from the second."""
    env_id, n_ref = "Cont-SC-SCIM-v0", 1
    envs = [ga.make(env_id, n_envs=N, device=0, max_episode_steps=5, reference_generator="default") for _ in range(2)]
    for e in envs:
        e.reset()
    env, twin = envs
    n_ref = len(env.reference_names)
    actor = ga.MLPPolicy(pr.make_layers(np.random.default_rng(11), 14 + n_ref, (24, 40, 3), scale=0.5), activation="tanh", squash="tanh")
    critic = ga.MLPPolicy(pr.make_layers(np.random.default_rng(4), 14 + n_ref, (64, 64, 1)), activation="tanh")
    noise = _dev(pr.case_data(env_id, "64x64", False, True)[3])
    pre = torch.randn(K, N, 3, device=DEV)
    log_std = torch.tensor([-0.5, 0.1, -1.3], device=DEV)
    reset = _dev(_reset_obs(env, 14))
    f32 = lambda *shape: torch.empty(shape, device=DEV)  # noqa: E731
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=DEV)  # noqa: E731
    state, refs, acts, reward = f32(K, N, 14), f32(K, N, n_ref), f32(K, N, 3), f32(K, N)
    term, trunc, ended = u8(K, N), u8(K, N), u8(K, N)
    value, last_value, adv, ret, lp, ent = f32(K, N), f32(N), f32(K, N), f32(K, N), f32(K, N), f32(K, N)
    start, shown0 = env.physical_system._obs.clone(), f32(N, n_ref)
    results = (state, refs, reward, acts, term, trunc, value, last_value, adv, ret, lp, ent)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rollout = env.bind_rollout_policy_complete_episodic(actor, K, state, refs, reward, acts, term, trunc, obs0=start, noise=noise, stream=side)
        values = critic.bind_evaluate_rollout(state, head="value", last=True, obs0=start, ended=ended, reset_obs=reset, refs=refs, shown0=shown0, n_ref=n_ref,
                                              value_out=value, value_last=last_value, stream=side)
        gae = ga.bind_advantages(reward, value, term, gamma=0.99, lam=0.95, last_value=last_value, ended=ended, advantage_out=adv, return_out=ret, stream=side)
        log_probs = actor.bind_evaluate_rollout(state, head="gaussian", obs0=start, ended=ended, reset_obs=reset, refs=refs, shown0=shown0, n_ref=n_ref,
                                                pre_squash=pre, log_std=log_std, squash_correction=True, log_prob_out=lp, entropy_out=ent, stream=side)

        def sequence():
            shown0.copy_(env._refs)  # (the references shown in front of the rollout: the rollout moves the env's own row on)
            rollout()
            torch.bitwise_or(term, trunc, out=ended)
            values()
            gae()
            log_probs()

        sequence()  # (outside the capture: loads the units and builds the handle's one-step map)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sequence()

    def eager(start_t):
        shown_t = twin._refs.clone()
        st, rf, rw, ac, te, tr = twin.rollout_policy_complete_episodic(actor, K, obs0=start_t, noise=noise)
        en = torch.bitwise_or(te, tr)
        v, lv = critic.evaluate_rollout(st, head="value", last=True, obs0=start_t, ended=en, reset_obs=reset, refs=rf, shown0=shown_t, n_ref=n_ref)
        a, r = ga.advantages(rw, v, te, gamma=0.99, lam=0.95, last_value=lv, ended=en)
        l, h = actor.evaluate_rollout(st, head="gaussian", obs0=start_t, ended=en, reset_obs=reset, refs=rf, shown0=shown_t, n_ref=n_ref, pre_squash=pre,
                                      log_std=log_std, squash_correction=True)
        torch.cuda.synchronize()
        return (st, rf, rw, ac, te, tr, v, lv, a, r, l, h)

    def compare(start_t):
        want = eager(start_t)
        for name, a, b in zip("state refs reward actions terminated truncated value last_value advantage returns log_prob entropy".split(), results, want):
            assert torch.equal(a, b), name
        return [t.clone() for t in results]

    runs = [compare(start.clone())]
    for change in (False, False, True):
        if change:
            critic.set_weights(pr.make_layers(np.random.default_rng(13), 14 + n_ref, (64, 64, 1)))
            log_std.copy_(torch.tensor([0.3, -0.7, 0.2], device=DEV))
        start.copy_(state[-1])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        runs.append(compare(start.clone()))
    for i in (6, 7, 8, 10, 11):  # value, last_value, advantage, log_prob, entropy: the third replay read the new weights and the new log_std
        assert not torch.equal(runs[2][i], runs[3][i]), i
    for e in envs:
        e.close()
