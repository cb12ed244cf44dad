"""The policy evaluation pass without a GPU: every refusal before any device call, the restatement's input construction against plain
loops, and its heads against scipy / mpmath."""
import numpy as np
import pytest
import torch

import gym_electric_motor_amd as ga
import policy_eval_restatement as per
import policy_restatement as pr

K, N, S = 3, 5, 14


def _policy(n_in=S, n_out=8, columns=None):
    return ga.MLPPolicy(pr.make_layers(np.random.default_rng(1), n_in, (16, n_out)), activation="tanh", columns=columns)


def _base(**over):
    kw = dict(obs0=torch.zeros(N, S), ended=torch.zeros(K, N, dtype=torch.uint8), reset_obs=torch.zeros(S))
    kw.update(over)
    return kw


TRAJ = torch.zeros(K, N, S)
U8 = torch.zeros(K, N, dtype=torch.uint8)
REFUSALS = [  # (policy kwargs, traj, call kwargs, exception, a piece of its own message)
    ({}, TRAJ, _base(obs0=torch.zeros(N, S + 1)), ValueError, "obs0 must have shape"),
    ({}, TRAJ, _base(ended=torch.zeros(K, N, dtype=torch.int32)), ValueError, "ended must have dtype"),
    ({}, TRAJ.transpose(0, 1).contiguous().transpose(0, 1), _base(), ValueError, "traj must be contiguous"),
    ({}, TRAJ, _base(), ValueError, "traj must be a device tensor"),
    ({"n_in": S + 1}, TRAJ, _base(), ValueError, "the policy's first layer takes"),
    ({}, TRAJ, _base(head="value"), ValueError, "head='value' needs a policy with one output"),
    ({}, TRAJ, _base(head="categorical", actions=torch.zeros(K, N)), ValueError, "takes the stored uint8 actions"),
    ({"n_out": 3}, TRAJ, _base(head="gaussian", log_std=torch.zeros(3)), ValueError, "head='gaussian' needs pre_squash"),
    ({"n_out": 3}, TRAJ, _base(head="gaussian", pre_squash=torch.zeros(K, N, 3)), ValueError, "head='gaussian' needs pre_squash"),
    ({}, TRAJ.half(), _base(), NotImplementedError, "traj is half precision"),
    ({}, TRAJ, _base(obs0=torch.zeros(N, S, dtype=torch.bfloat16)), NotImplementedError, "obs0 is half precision"),
    ({}, torch.zeros(K, N, 25), _base(), ValueError, "a stored row has at most 24"),
    ({}, TRAJ, dict(mode="next", last=True), ValueError, "mode='next' cannot be combined with last=True"),
    ({}, TRAJ, _base(head="categorical", actions=U8, last=True), ValueError, "last=True has no meaning"),
]


@pytest.mark.parametrize("pkw,traj,kw,exc,msg", REFUSALS, ids=[r[4][:28] for r in REFUSALS])
def test_refusals_before_any_device_call(pkw, traj, kw, exc, msg):
    env = ga.make("Finite-CC-PMSM-v0", n_envs=N, max_episode_steps=5, _defer_create=True)
    policy = _policy(**pkw)
    with pytest.raises(exc, match=msg):
        policy.evaluate_rollout(traj, system=env.physical_system, **kw)
    with pytest.raises(exc, match=msg):  # the bound form: before its outputs are inspected (none is given here)
        policy.bind_evaluate_rollout(traj, system=env.physical_system, **kw)
    assert policy._handle is None and env.physical_system._handle is None


def test_input_construction_against_plain_loops():
    rng = np.random.default_rng(5)
    traj, obs0, reset = rng.normal(size=(K, N, S)), rng.normal(size=(N, S)), rng.normal(size=S)
    refs, shown0, last_refs = rng.normal(size=(K, N, 2)), rng.normal(size=(N, 2)), rng.normal(size=(N, 2))
    ended = np.zeros((K, N), dtype=np.uint8)
    ended[0, 1] = ended[1, 1] = ended[1, 3] = ended[2, 4] = ended[2, 0] = 1
    cols = [12, 0, 5]
    for complete in (False, True):
        for last in (False, True):
            rows = K + 1 if last else K
            want = np.zeros((rows, N, len(cols) + 2))
            for k in range(rows):
                for e in range(N):
                    o = obs0[e] if k == 0 else (reset if ended[k - 1, e] else traj[k - 1, e])
                    if complete:
                        r = shown0[e] if k == 0 else refs[k - 1, e]
                    else:
                        r = last_refs[e] if k == K else refs[k, e]
                    want[k, e] = [o[c] for c in cols] + list(r)
            kw = dict(refs=refs, shown0=shown0) if complete else dict(references=refs, last_references=last_refs)
            got = per.inputs(traj, cols, "seen", last, obs0=obs0, ended=ended, reset_obs=reset, **kw)
            assert np.array_equal(got, want)
    nxt = per.inputs(traj, cols, "next", refs=refs)
    assert np.array_equal(nxt, np.concatenate([traj[:, :, cols], refs], axis=2))
    seen = per.inputs(traj, cols, "seen", True, obs0=obs0, ended=ended, reset_obs=reset, refs=refs, shown0=shown0)
    differs = (nxt != seen[1:]).any(axis=2)
    assert np.array_equal(differs, ended.astype(bool))


def test_heads_against_scipy():
    from scipy.special import logsumexp
    from scipy.stats import norm

    rng = np.random.default_rng(7)
    z = rng.uniform(-20, 20, (40, 8))
    a = rng.integers(0, 8, 40)
    lp, h = per.categorical(z, a)
    logp = z - logsumexp(z, axis=1, keepdims=True)
    assert np.allclose(lp, logp[np.arange(40), a], rtol=1e-13, atol=1e-13)
    assert np.allclose(h, -(np.exp(logp) * logp).sum(axis=1), rtol=1e-13, atol=1e-13)
    z3, u, ls = rng.uniform(-20, 20, (40, 3)), rng.uniform(-20, 20, (40, 3)), rng.uniform(-1, 1, 3)
    lp, h = per.gaussian(z3, u, ls)
    assert np.allclose(lp, norm.logpdf(u, loc=z3, scale=np.exp(ls)).sum(axis=1), rtol=1e-13, atol=1e-13)
    assert np.allclose(h, norm.entropy(scale=np.exp(ls)).sum(), rtol=1e-13, atol=1e-13)


def test_tanh_correction():
    u = np.linspace(-6, 6, 241)
    try:
        import mpmath

        mpmath.mp.dps = 40
        want = np.array([float(mpmath.log(1 - mpmath.tanh(mpmath.mpf(float(v))) ** 2)) for v in u])
    except ImportError:
        want = np.log(1.0 - np.tanh(u) ** 2)
    assert np.allclose(per.tanh_correction(u), want, rtol=1e-12, atol=1e-13)
