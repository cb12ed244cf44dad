"""GPU tests of the device-side StateNoiseProcessor (csrc/gemx_statenoise.hip, state_noise.py): the zero-noise identity with the fused path
(in-kernel constraints, auto-reset, fused reward), the stage's arithmetic against `gemx_noise_draws` / `gemx_reward_rows` / a float64
constraint check, the three distributions, the streams (seeds, shards, graph replay, checkpoint), the noise-free twin, the stages behind
the noise and the rollout refusals.  No test restates the Philox stream on the host: `gemx_noise_draws` is the seam."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reward_path_cases as rp  # noqa: E402

N = 193  # a partial workgroup (256 fp32 / 128 fp64 rows per tile), rows no multiple of the tile


def _noise(ga, states, dist="normal", **kw):
    return ga.StateNoiseProcessor(states, dist, kw)


def _actions(env, K, seed):
    """Per-env constant actions (a held duty cycle / switching vector drives the currents over their limits within a few steps)."""
    import torch

    rng = np.random.default_rng(seed)
    space = env.physical_system.action_space
    if hasattr(space, "n"):
        a = np.repeat(rng.integers(0, int(space.n), (1, N)), K, axis=0).astype(np.uint8)
        return torch.as_tensor(a).cuda()
    a = np.repeat(rng.uniform(-1, 1, (1, N, int(space.shape[0]))), K, axis=0)
    return torch.as_tensor(a).cuda()


def _run(env, actions):
    """reset + K steps of a complete env -> stacked clones (state, refs, reward, terminated), row 0 of state / refs: after reset."""
    import torch

    (s, r), _ = env.reset()
    S, R, W, T = [s.clone()], [r.clone()], [], []
    for k in range(actions.shape[0]):
        (s, r), w, t, _, _ = env.step(actions[k].to(env.physical_system._want_dtype))
        S.append(s.clone()), R.append(r.clone()), W.append(w.clone()), T.append(t.clone())
    torch.cuda.synchronize()
    return torch.stack(S), torch.stack(R), torch.stack(W), torch.stack(T)


IDENTITY = {
    "permex": ("Cont-CC-PermExDc-v0", ["i", "omega"], dict(), ()),
    "pmsm_finite": ("Finite-CC-PMSM-v0", ["i_sd", "i_sq"], dict(tau=1e-4), ()),
    "pmsm_dead2": ("Cont-CC-PMSM-v0", ["i_sd", "i_sq", "epsilon"], dict(), "dead2"),
    "pmsm_random_init": ("Cont-CC-PMSM-v0", ["i_sd", "i_sq"], dict(motor=dict(motor_initializer=dict(random_init="uniform"))), ()),
}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(IDENTITY))
def test_zero_noise_is_the_fused_path(case, dtype):
    """normal(0, 0): the external constraint check, the reward arithmetic and the reset feedback (masked gemx_reset in front of the next
    step; with random initialisers it draws what the in-kernel reset draws) give the bits of the env without the wrapper."""
    import torch

    import gym_electric_motor_amd as ga

    env_id, states, kw, extra = IDENTITY[case]
    extra = (ga.DeadTimeProcessor(2),) if extra == "dead2" else ()
    K = 48
    kw = dict(kw, n_envs=N, dtype=dtype, reference_generator="default", seed=5)
    plain = ga.make(env_id, physical_system_wrappers=extra, **kw)
    noisy = ga.make(env_id, physical_system_wrappers=extra + (_noise(ga, states, scale=0.0),), **kw)
    assert noisy.physical_system._cfg.auto_reset == 0 and plain.physical_system._cfg.auto_reset == 1
    a = _actions(plain, K, seed=1)
    want, got = _run(plain, a), _run(noisy, a)
    share = float(want[3].any(dim=0).float().mean())
    print(f"{case} {dtype}: lanes that terminate at least once {share:.3f}, terminations {int(want[3].sum())}")
    assert share >= 0.10
    for name, w, g in zip(("state", "refs", "reward", "terminated"), want, got):
        assert torch.equal(w, g), (name, int((w != g).sum()))
    plain.close(), noisy.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("env_id", ["Cont-CC-PMSM-v0", "Cont-CC-PermExDc-v0"])
def test_stage_arithmetic(env_id, dtype):
    """state_out == state_in + draws bit for bit on the noisy columns, the other columns untouched; the reward is gemx_reward_rows' on
    (state_out, done_out); done against a float64 recomputation (squared constraint: rows within 1e-5 of the threshold skipped, at
    most 1 % of them; limit constraint: exact).  normal(0, 0.6) on zero currents: sum x^2 is exponential with mean 0.72, ~25 % violate."""
    import torch

    import gym_electric_motor_amd as ga

    pmsm = "PMSM" in env_id
    states = ["i_sd", "i_sq"] if pmsm else ["i", "omega"]
    kw = dict(n_envs=N, dtype=dtype, reference_generator="default", seed=21, reward_function=dict(reward_power=2) if pmsm else "default")
    # (the limit constraint on one column: normal(0, 1) violates |x| > 1 in 32 % of the rows; 0.6 would give 9.6 %)
    env = ga.make(env_id, physical_system_wrappers=(_noise(ga, states, scale=0.6 if pmsm else 1.0),), **kw)
    plain = ga.make(env_id, **kw)
    stage, td = env.state_noise, env.physical_system._tdtype
    idx, K = stage.indices, 8
    g = torch.Generator(device="cuda").manual_seed(3)
    rows = (torch.rand((K, N, stage.n_in), generator=g, device="cuda", dtype=torch.float64) * 0.6 - 0.3).to(td)
    rows[..., idx] = 0
    refs = (torch.rand((K, N, stage.n_ref), generator=g, device="cuda", dtype=torch.float64) - 0.5).to(td)
    draws = stage.draws(0, K)
    out, done, reward = torch.empty_like(rows), torch.empty((K, N), dtype=torch.uint8, device="cuda"), torch.empty((K, N), dtype=td, device="cuda")
    want_reward = torch.empty_like(reward)
    for k in range(K):
        stage.step(rows[k], refs[k], out[k], done[k], reward[k])
        plain._refs.copy_(refs[k])
        plain.bind_reward_rows(out[k][None], refs[k][None], done[k][None], want_reward[k][None])()
    assert stage.get_position() == K
    keep = [j for j in range(stage.n_in) if j not in idx]
    assert torch.equal(out[..., idx], rows[..., idx] + draws) and torch.equal(out[..., keep], rows[..., keep])
    assert torch.equal(reward, want_reward)
    x = out.double()
    if pmsm:
        sq = (x[..., idx] ** 2).sum(-1)
        near = (sq - 1).abs() < 1e-5
        assert float(near.float().mean()) <= 0.01
        want_done = sq > 1
        assert torch.equal(done.bool()[~near], want_done[~near])
    else:
        want_done = x[..., idx[0]].abs() > 1  # LimitConstraint on 'i' alone: the noisy omega does not terminate
        assert torch.equal(done.bool(), want_done)
    share = float(done.float().mean())
    print(f"{env_id} {dtype}: share of violating rows {share:.3f}")
    assert 0.10 <= share <= 0.90
    # in place: the same rows
    stage.set_position(0)
    buf = rows[0].clone()
    stage.step(buf, refs[0], buf, done[0].clone(), None)
    assert torch.equal(buf, out[0])
    # a view at an odd element offset (the dword path of the tile)
    stage.set_position(0)
    flat = torch.zeros(N * stage.n_in + 1, dtype=td, device="cuda")
    view = flat[1:].view(N, stage.n_in)
    view.copy_(rows[0])
    stage.step(view, refs[0], view, done[0].clone(), None)
    assert torch.equal(view, out[0]) and float(flat[0]) == 0.0
    env.close(), plain.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", sorted(rp.SHAPES))
def test_stage_reward_equals_the_reward_pass_on_every_shape(shape, dtype):
    """The stage's reward is reward_row's (csrc/gemx_reward.hpp) at every shape of reward_path_cases -- hot terms, terms beyond them, the
    pow() path, 0 / 1 / 4 references: bit for bit gemx_reward_rows' on (state_out, refs, done_out), and exactly the violation reward on
    the rows that are done.  One step of 259 rows (a full fp32 tile and three rows, two fp64 tiles and three) under normal(0, 0) noise on
    one column, so state_out is the input.  Rows are uniform in (-0.5, 0.5): no limit fires and at most three squares sum to 0.75 < 1;
    every third row carries 1.5 in the lowest constrained column, which fires a limit (1.5 > 1) or a squared constraint (2.25 > 1).
    Then once more into an output view at an odd element offset (the dword path of the tile)."""
    import ctypes as C

    import torch

    import gym_electric_motor_amd as ga
    from gym_electric_motor_amd import _lib
    from gym_electric_motor_amd.state_noise import StateNoiseStage

    case, n = rp.Case(shape), 259
    env = ga.make(case.env_id, n_envs=n, dtype=dtype, obs_layout="aos")
    ps = env.physical_system
    assert list(ps.state_names) == case.names
    rc = ps.set_reward(referenced_states=case.ref_names, **case.set_reward_kwargs)
    limit_mask, squared_mask = int(ps._cfg.limit_mask), int(ps._cfg.squared_mask)
    constrained = limit_mask | squared_mask
    assert constrained and bin(squared_mask).count("1") <= 3
    spec = dict(states=[case.names[0]], dist="normal", kwargs=dict(scale=0.0), limit_mask=limit_mask, squared_mask=squared_mask)
    stage = StateNoiseStage(ps, spec, rc).create(n, 0, dtype)
    td, n_ref = ps._tdtype, len(case.ref_cols)
    assert stage.n_in == len(case.names) and stage.n_ref == n_ref

    g = torch.Generator(device="cuda").manual_seed(17)
    rows = (torch.rand((n, stage.n_in), generator=g, device="cuda", dtype=torch.float64) - 0.5).to(td)
    violate = torch.arange(n, device="cuda") % 3 == 0
    rows[violate, (constrained & -constrained).bit_length() - 1] = 1.5
    refs = ((torch.rand((n, n_ref), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 1.6).to(td) if n_ref else None

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def check(out):
        done, reward = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=td, device="cuda")
        stage.step(rows, refs, out, done, reward)
        assert torch.equal(out, rows)
        assert torch.equal(done.bool(), violate)
        want = torch.empty_like(reward)
        _lib.check(ps._L.gemx_reward_rows(ps._handle, ptr(out), ptr(refs), None, ptr(done), 1, ptr(want), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert torch.equal(reward, want), int((reward != want).sum())
        assert bool((reward[violate] == case.violation_reward).all())
        return reward

    first = check(torch.empty_like(rows))
    flat = torch.zeros(n * stage.n_in + 1, dtype=td, device="cuda")
    assert torch.equal(check(flat[1:].view(n, stage.n_in)), first) and float(flat[0]) == 0.0
    stage.close(), env.close()


def _cdf(dist, p0, p1, x):
    if dist == "normal":
        return 0.5 * (1 + np.vectorize(math.erf)((x - p0) / (p1 * math.sqrt(2))))
    if dist == "uniform":
        return np.clip((x - p0) / (p1 - p0), 0, 1)
    z = (x - p0) / p1
    return np.where(z < 0, 0.5 * np.exp(z), 1 - 0.5 * np.exp(-z))


DISTS = {  # dist -> (numpy keywords, per-column mean, std, kurtosis)
    "normal": (dict(loc=[0.1, -0.2], scale=[0.5, 2.0]), lambda a, b: (a, b, 3.0)),
    "uniform": (dict(low=[-1.0, 0.0], high=[1.0, 3.0]), lambda a, b: ((a + b) / 2, (b - a) / math.sqrt(12), 1.8)),
    "laplace": (dict(loc=[0.0, 1.0], scale=[0.3, 1.0]), lambda a, b: (a, b * math.sqrt(2), 6.0)),
}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("dist", sorted(DISTS))
def test_distributions(dist, dtype):
    """Per column, 193 envs x 64 positions: one-sample KS against the closed-form CDF (D < 1.95 / sqrt(n), alpha = 0.001), mean and standard
    deviation within 4 standard errors, correlations between neighbouring envs and consecutive positions below 4 / sqrt(n)."""
    import gym_electric_motor_amd as ga

    kwargs, moments = DISTS[dist]
    env = ga.make("Cont-CC-PermExDc-v0", n_envs=N, dtype=dtype, seed=1234, physical_system_wrappers=(ga.StateNoiseProcessor(["omega", "i"], dist, kwargs),))
    d = env.state_noise.draws(0, 64).double().cpu().numpy()
    n = 64 * N
    keys = list(kwargs)
    for c in range(2):
        p0, p1 = kwargs[keys[0]][c], kwargs[keys[1]][c]
        x = np.sort(d[..., c].ravel())
        F = _cdf(dist, p0, p1, x)
        D = max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(0, n) / n))
        mean, std, kurt = moments(p0, p1)
        se_mean, se_std = std / math.sqrt(n), std * math.sqrt((kurt - 1) / (4 * n))
        z = (d[..., c] - mean) / std
        r_env, r_pos = float(np.mean(z[:, :-1] * z[:, 1:])), float(np.mean(z[:-1] * z[1:]))
        print(f"{dist} {dtype} column {c}: D {D:.4f} (< {1.95 / math.sqrt(n):.4f}), mean {x.mean():+.4f} ({mean:+.4f} +- {4 * se_mean:.4f}), "
              f"std {x.std():.4f} ({std:.4f} +- {4 * se_std:.4f}), r_env {r_env:+.4f}, r_pos {r_pos:+.4f} (< {4 / math.sqrt(n):.4f})")
        assert D < 1.95 / math.sqrt(n)
        assert abs(x.mean() - mean) < 4 * se_mean and abs(x.std() - std) < 4 * se_std
        assert abs(r_env) < 4 / math.sqrt(n) and abs(r_pos) < 4 / math.sqrt(n)
    env.close()


def test_streams_seeds_shards_and_consumption():
    import torch

    import gym_electric_motor_amd as ga

    w = lambda: (_noise(ga, ["i_sd", "i_sq", "omega"], "laplace", scale=[0.1, 0.2, 0.3]),)  # noqa: E731  (three slots: two Philox blocks)
    mk = lambda n=N, seed=7, base=0: ga.make("Cont-CC-PMSM-v0", n_envs=n, seed=seed, env_base=base, physical_system_wrappers=w())  # noqa: E731
    a, b, c = mk(), mk(), mk(seed=8)
    K = 16
    da = a.state_noise.draws(0, K)
    assert torch.equal(da, b.state_noise.draws(0, K)) and not torch.equal(da, c.state_noise.draws(0, K))
    assert torch.equal(a.state_noise.draws(5, 3), da[5:8])  # (chunked == one-shot; the position did not move)
    assert a.state_noise.get_position() == 0
    # K steps consume what draws(0, K) lists
    zeros = torch.zeros((N, 14), device="cuda")
    for k in range(K):
        out, _, _ = a.state_noise.step(zeros)
        assert torch.equal(out[:, a.state_noise.indices], da[k]), k
    assert a.state_noise.get_position() == K
    # two half-size handles with env_base == one whole handle
    lo, hi = mk(n=96), mk(n=N - 96, base=96)
    assert torch.equal(torch.cat((lo.state_noise.draws(0, K), hi.state_noise.draws(0, K)), dim=1), da)
    for e in (a, b, c, lo, hi):
        e.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_graph_replay_and_checkpoint(dtype):
    """K replays of a captured `bind_step` graph == K eager steps (the stream position and the done feedback live on the device);
    `set_checkpoint` on a fresh env resumes bit for bit."""
    import torch

    import gym_electric_motor_amd as ga

    K = 24
    kw = dict(n_envs=N, dtype=dtype, seed=2, physical_system_wrappers=(_noise(ga, ["i_sd", "i_sq"], scale=0.05), ga.CosSinProcessor()))
    eager, graphed = (ga.make("Cont-CC-PMSM-v0", reference_generator="default", **kw) for _ in range(2))
    a = _actions(eager, 1, seed=3)[0].to(eager.physical_system._tdtype).contiguous()
    side = torch.cuda.Stream()
    step, obs, reward, done = graphed.bind_step(a, stream=side)
    step_t, obs_t, reward_t, done_t = eager.bind_step(a)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start; the twin gets the same history
        for _ in range(3):
            step()
        graphed.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(3):
        step_t()
    eager.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    terminations = 0
    for k in range(K):
        g.replay()
        step_t()
        torch.cuda.synchronize()
        for name, x, y in (("state", obs[0], obs_t[0]), ("refs", obs[1], obs_t[1]), ("reward", reward, reward_t), ("terminated", done, done_t)):
            assert torch.equal(x, y), (name, k)
        terminations += int(done.sum())
    assert terminations > 0 and graphed.state_noise.get_position() == eager.state_noise.get_position() == 3 + 1 + K
    eager.close(), graphed.close()
    # checkpoint (the physics-only env: state, done mask waiting for its reset, stream position)
    first, second = (ga.make("Cont-CC-PMSM-v0", **kw) for _ in range(2))
    first.reset()
    for _ in range(7):
        first.step(a)
    ck = first.get_checkpoint()
    assert ck["state_noise"]["position"] == 8  # (the reset row is noised too)
    tail = [tuple(t.clone() for t in (first.step(a)[0], first.physical_system.done)) for _ in range(9)]
    second.reset()
    second.set_checkpoint(ck)
    for k, (s, d) in enumerate(tail):
        s2 = second.step(a)[0]
        assert torch.equal(s2, s) and torch.equal(second.physical_system.done, d), k
    assert sum(int(d.sum()) for _, d in tail) > 0
    first.close(), second.close()
    # the complete env's checkpoint carries the Wiener generators and the references the noisy reward reads, too
    first, second = (ga.make("Cont-CC-PMSM-v0", reference_generator="default", **kw) for _ in range(2))
    first.reset()
    for _ in range(7):
        first.step(a)
    ck = first.get_checkpoint()
    assert ck["state_noise"]["position"] == 8 and set(ck["reference_generator"]) == {"blob", "references"}
    tail = []
    for _ in range(9):
        (s, r), w, d, _, _ = first.step(a)
        tail.append((s.clone(), r.clone(), w.clone(), d.clone()))
    second.reset()
    second.step(-a)  # (nothing of the second env is at its create-time zero)
    second.set_checkpoint(ck)
    for k, want in enumerate(tail):
        (s, r), w, d, _, _ = second.step(a)
        for name, x, y in zip(("state", "refs", "reward", "terminated"), (s, r, w, d), want):
            assert torch.equal(x, y), (name, k)
    assert sum(int(t[3].sum()) for t in tail) > 0 and not torch.equal(tail[0][1], tail[-1][1])
    first.close(), second.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_noise_free_twin(dtype):
    """A second system without constraints and auto-reset, driven by the same actions and reset on the noisy env's previous `terminated`,
    produces the noisy env's pre-noise rows bit for bit; a lane terminated at step k shows at k + 1 one step from the reset state."""
    import torch

    import gym_electric_motor_amd as ga

    K = 32
    kw = dict(n_envs=N, dtype=dtype, seed=4)
    noisy = ga.make("Cont-CC-PMSM-v0", physical_system_wrappers=(_noise(ga, ["i_sd", "i_sq"], "uniform", low=-0.3, high=0.3),), **kw)
    twin, fresh = (ga.make("Cont-CC-PMSM-v0", constraints=(), auto_reset=False, **kw) for _ in range(2))
    a = _actions(noisy, 1, seed=6)[0].to(noisy.physical_system._tdtype).contiguous()
    noisy.reset(), twin.reset()
    prev, checked = None, 0
    for k in range(K):
        if prev is not None:
            twin.physical_system.reset(mask=prev)
        raw = twin.step(a)[0]
        state, _, term, _, _ = noisy.step(a)
        assert torch.equal(noisy.pipeline.physical_system._obs, raw), k
        assert not torch.equal(state, raw)
        if prev is not None and bool(prev.any()):
            fresh.reset()
            one = fresh.step(a)[0]
            lanes = prev.bool()
            assert torch.equal(raw[lanes], one[lanes]), k
            checked += int(lanes.sum())
        prev = term.clone()
    assert checked > 0
    for e in (noisy, twin, fresh):
        e.close()


def test_stages_behind_the_noise_read_the_noisy_row():
    import torch

    import gym_electric_motor_amd as ga

    K = 24
    mods = ga.default_env_modules("Cont-CC-PMSM-v0")
    env = ga.make("Cont-CC-PMSM-v0", n_envs=N, seed=9, reference_generator="default", flatten_observation=True,
                  physical_system_wrappers=(_noise(ga, ["i_sd", "i_sq", "epsilon"], scale=0.05), ga.CosSinProcessor(remove_angle=True)),
                  observed_states=["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"])
    gen = ga.BatchedWienerProcessReferenceGenerator(reference_states=mods["reference_states"], seed=9, **mods["generator"]).set_modules(env.physical_system)
    a = _actions(env, 1, seed=10)[0].float().contiguous()
    obs, _ = env.reset()
    gen.reset()
    refs = gen.step(None)
    stage, pipe = env.observation_stage, env.pipeline
    assert torch.equal(obs, stage.apply(pipe.noisy, refs))
    seen = 0
    for k in range(K):
        obs, reward, term, _, _ = env.step(a)
        refs = gen.step(term)  # the complete env's generators restart exactly on the noisy `terminated` lanes
        assert torch.equal(obs, stage.apply(pipe.noisy, refs)), k
        assert not torch.equal(pipe.noisy, env.physical_system._obs)
        seen += int(term.sum())
    assert seen > 0
    env.close(), gen.close()


def test_rollout_entry_points_raise():
    import torch

    import gym_electric_motor_amd as ga

    w = (_noise(ga, ["i"], scale=0.1),)
    env = ga.make("Cont-CC-PermExDc-v0", n_envs=N, physical_system_wrappers=w)
    a = torch.zeros((4, N, 1), device="cuda")
    for call in (lambda: env.rollout(a), lambda: env.rollout_synthetic(4),
                 lambda: env.bind_rollout(a, torch.empty((4, N, 5), device="cuda"), torch.empty((4, N), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(NotImplementedError, match="StateNoiseProcessor"):
            call()
    env.close()
    env = ga.make("Cont-CC-PermExDc-v0", n_envs=N, physical_system_wrappers=w, reference_generator="default")
    outs = (torch.empty((4, N, 5), device="cuda"), torch.empty((4, N, 1), device="cuda"), torch.empty((4, N), device="cuda"),
            torch.empty((4, N), dtype=torch.uint8, device="cuda"))
    for call in (lambda: env.rollout_complete(a), lambda: env.rollout_complete_synthetic(4), lambda: env.bind_rollout_complete(a, *outs)):
        with pytest.raises(NotImplementedError, match="StateNoiseProcessor"):
            call()
    env.close()
