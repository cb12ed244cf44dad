"""GPU tests of the device-side episode time limit and episode statistics (csrc/gemx_episode.hip, episodes.py): the stage alone and its
rows pass against the numpy restatement (tests/episode_restatement.py) -- every comparison exact --, the env with a time limit against a
second env that the test itself resets and whose generators it restarts, the mask reaching the noise stage's restart and the flux
observer's reset, HIP-graph replay, checkpoints, and each keyword alone."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling module: the restatement)

pytestmark = pytest.mark.gpu

STEPS = 7
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")


def _bits(t):
    """A tensor's bits (float64 / int32 / uint8 compared as integers: bit-equal, not merely equal)."""
    import torch

    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(got, want, what):
    import torch

    want = torch.as_tensor(np.ascontiguousarray(want))
    if got.dtype == torch.int32:
        want = want.to(torch.int32)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))


def _table(K, N, dtype, seed):
    """done bytes at p ~ 0.2 and rewards of both signs and several magnitudes, as device tensors and numpy arrays."""
    import torch

    rng = np.random.default_rng(seed)
    done = (rng.random((K, N)) < 0.2).astype(np.uint8)
    reward = (rng.standard_normal((K, N)) * 10.0 ** rng.integers(-3, 4, (K, N))).astype(np.float32 if dtype == "float32" else np.float64)
    return torch.as_tensor(done).cuda(), torch.as_tensor(reward).cuda(), done, reward


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
def test_stage_alone(N, M, dtype):
    """All outputs of gemx_episode_step -- the five fields, truncated, ended (and reset_mask, in both of its meanings) -- after each of 7
    calls equal the restatement exactly; one lane, a partial wave, a full wave, wave + 1, several workgroups with a tail."""
    import torch

    import gym_electric_motor_amd as ga
    from episode_restatement import Episodes

    done_d, reward_d, done, reward = _table(STEPS, N, dtype, seed=100 * N + M)
    for in_kernel in (False, True):
        stage = ga.EpisodeStage(M, statistics=True, auto_reset_in_kernel=in_kernel, has_reward=True).create(N, 0, dtype)
        want = Episodes(N, M, in_kernel)
        for k in range(STEPS):
            t, e, m = stage.step(done_d[k], reward_d[k])
            wt, we, wm = want.step(done[k], reward[k])
            torch.cuda.synchronize()
            for name, g, w in (("truncated", t, wt), ("ended", e, we), ("reset_mask", m, wm)):
                _same(g, w, (name, k, in_kernel))
            for name, w in want.fields().items():
                _same(stage.fields()[name], w, (name, k, in_kernel))
        assert int(want.n_finished.sum()) > 0
        stage.close()
    # `done` and `reset_mask` may be the same buffer
    stage = ga.EpisodeStage(M, auto_reset_in_kernel=False, has_reward=True).create(N, 0, dtype)
    want = Episodes(N, M, False)
    buf = done_d[0].clone()
    stage.bind_step(buf, reward_d[0], reset_mask=buf)()
    _same(buf, want.step(done[0], reward[0])[2], "aliased reset_mask")
    # without a reward the return stays 0 and the lengths count
    stage2 = ga.EpisodeStage(M, has_reward=False).create(N, 0, dtype)
    want = Episodes(N, M)
    for k in range(STEPS):
        stage2.step(done_d[k])
        want.step(done[k])
    for name, w in want.fields().items():
        _same(stage2.fields()[name], w, name)
    with pytest.raises(ValueError):
        stage2.bind_step(done_d[0], reward_d[0])
    stage.close(), stage2.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("K,N,M", [(5, 130, 3), (7, 65, 3), (7, 65, 0), (19, 65, 3)])  # (19 rows: two full groups of loads in flight and a tail)
def test_rows_pass_equals_step_calls(K, N, M, dtype):
    """gemx_episode_rows over stored rows == K calls of gemx_episode_step, bit for bit: the handle's state blob, `ended`, and the
    finished_* rows (an episode's totals at the row where it ended, 0 elsewhere); both equal the restatement."""
    import torch

    import gym_electric_motor_amd as ga
    from episode_restatement import Episodes

    done_d, reward_d, done, reward = _table(K, N, dtype, seed=K * N + M)
    make = lambda: ga.EpisodeStage(M or None, statistics=True, has_reward=True).create(N, 0, dtype)  # noqa: E731
    stepped, passed = make(), make()
    ended, fin_ret, fin_len = [], [], []
    for k in range(K):
        _, e, _ = stepped.step(done_d[k], reward_d[k])
        ended.append(e.clone())
        fin_ret.append(torch.where(e != 0, stepped.last_ret, torch.zeros_like(stepped.last_ret)))
        fin_len.append(torch.where(e != 0, stepped.last_length, torch.zeros_like(stepped.last_length)))
    got = passed.rows(done_d, reward_d)
    torch.cuda.synchronize()
    assert torch.equal(passed.get_state(), stepped.get_state())
    want = Episodes(N, M).rows(done, reward)
    for name, g, s in zip(("ended", "finished_return", "finished_length"), got, (ended, fin_ret, fin_len)):
        assert torch.equal(_bits(g), _bits(torch.stack(s))), name
        _same(g, want[name], name)
    # the optional outputs left out: same state; a second pass continues the first
    third = make()
    third.bind_rows(done_d[:2], reward_d[:2], torch.empty((2, N), dtype=torch.uint8, device="cuda"))()
    if K > 2:
        third.bind_rows(done_d[2:], reward_d[2:], torch.empty((K - 2, N), dtype=torch.uint8, device="cuda"))()
    assert torch.equal(third.get_state(), stepped.get_state())
    for s in (stepped, passed, third):
        s.close()


def _actions(env, N, seed):
    """Per-env random actions, held over the steps (a held duty cycle / switching vector drives the currents towards their limits)."""
    import torch

    rng = np.random.default_rng(seed)
    space = env.physical_system.action_space
    if hasattr(space, "n"):
        return torch.as_tensor(rng.integers(0, int(space.n), N).astype(np.uint8)).cuda()
    return torch.as_tensor(rng.uniform(-1, 1, (N, int(space.shape[0])))).cuda().to(env.physical_system._tdtype).contiguous()


def _run(env, a, steps=STEPS, reset=True):
    """`steps` steps -> per step (state, refs | None, reward | None, terminated, truncated) as clones."""
    import torch

    if reset:
        env.reset()
    out = []
    for _ in range(steps):
        obs, w, t, tr, _ = env.step(a)
        s, r = obs if isinstance(obs, tuple) else (obs, None)
        out.append((s.clone(), None if r is None else r.clone(), None if w is None else w.clone(), t.clone(), tr.clone() if torch.is_tensor(tr) else tr))
    torch.cuda.synchronize()
    return out


N_ENV, M_ENV = 65, 3


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("env_id", ["Cont-CC-PMSM-v0", "Finite-CC-PermExDc-v0", "Cont-CC-SCIM-v0"])
def test_env_equals_a_hand_reset_env(env_id, dtype):
    """make(max_episode_steps=3) against a second env without the keyword whose physics the test resets with the expected mask and whose
    generators it restarts on `ended`: states, references, rewards and `terminated` are equal at every step; `truncated` is set exactly at
    steps 3 and 6 for the lanes that did not terminate earlier; the counters equal the restatement.  (Measured: under held random actions
    no PMSM or PermExDc lane terminates within 7 steps, 3 of the 65 SCIM lanes do (6 terminations) -- there the kernel's own restart of a terminated env and
    the masked reset of the truncated ones meet in one run.)"""
    import torch

    import gym_electric_motor_amd as ga
    from episode_restatement import Episodes

    kw = dict(n_envs=N_ENV, dtype=dtype, reference_generator="default", seed=7)
    env = ga.make(env_id, max_episode_steps=M_ENV, episode_statistics=True, **kw)
    twin = ga.make(env_id, **kw)
    assert env.episodes._cfg.auto_reset_in_kernel == 1 and twin.episodes is None
    a = _actions(env, N_ENV, seed=11)
    got = _run(env, a)
    twin.reset()
    ps, gen = twin.physical_system, twin.reference_generator
    want, mask = Episodes(N_ENV, M_ENV, True), np.zeros(N_ENV, np.uint8)
    never, terminations = np.ones(N_ENV, bool), 0
    for k in range(STEPS):
        ps.reset(torch.as_tensor(mask).cuda())  # the truncated envs; the kernel restarts the terminated ones itself
        state = ps.simulate(a, references=gen.references).clone()
        reward, done = ps.reward.clone(), ps.done.clone()
        truncated, ended, mask = want.step(done.cpu().numpy(), reward.cpu().numpy())
        refs = gen.step(torch.as_tensor(ended).cuda()).clone()
        torch.cuda.synchronize()
        s, r, w, t, tr = got[k]
        for name, x, y in (("state", s, state), ("refs", r, refs), ("reward", w, reward), ("terminated", t, done)):
            assert torch.equal(x, y), (name, k, int((x != y).sum()))
        assert tr.dtype == torch.bool and np.array_equal(tr.cpu().numpy(), truncated != 0), k
        never &= done.cpu().numpy() == 0
        terminations += int(done.sum())
        assert np.array_equal(truncated[never] != 0, np.full(int(never.sum()), k in (2, 5))), k
    print(f"{env_id} {dtype}: lanes that never terminated {int(never.sum())} of {N_ENV}, terminations {terminations}")
    assert int(never.sum()) > 0 and (terminations > 0 or "SCIM" not in env_id)
    stats = env.episode_statistics()
    for name, w in want.fields().items():
        _same(stats[name], w, name)
    assert stats["ret"].data_ptr() == env.episodes.ret.data_ptr()  # views: nothing is copied
    env.close(), twin.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("env_id", ["Cont-CC-PMSM-v0", "Cont-CC-SCIM-v0"])
def test_mask_reaches_the_noise_stage(env_id, dtype):
    """StateNoiseProcessor(scale=0) with a time limit == the env without the wrapper with the same limit (whose restart the test above pins):
    behind the noise stage the reset in front of the next step reads the episode stage's `ended` mask."""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(n_envs=N_ENV, dtype=dtype, reference_generator="default", seed=7, max_episode_steps=M_ENV, episode_statistics=True)
    plain = ga.make(env_id, **kw)
    noisy = ga.make(env_id, physical_system_wrappers=(ga.StateNoiseProcessor(["i_sd", "i_sq"], "normal", dict(scale=0)),), **kw)
    assert noisy.episodes._cfg.auto_reset_in_kernel == 0 and noisy.pipeline.launch_order(True) == ["reset", "physics", "noise", "episode", "generators"]
    a = _actions(plain, N_ENV, seed=11)
    want, got = _run(plain, a), _run(noisy, a)
    for k in range(STEPS):
        for name, x, y in zip(("state", "refs", "reward", "terminated", "truncated"), got[k], want[k]):
            assert torch.equal(x, y), (name, k)
    print(f"noise stage {env_id} {dtype}: terminations {sum(int(w[3].sum()) for w in want)}, truncations {sum(int(w[4].sum()) for w in want)}")
    assert sum(int(w[4].sum()) for w in want) > 0
    for name in FIELDS:
        assert torch.equal(_bits(noisy.episode_statistics()[name]), _bits(plain.episode_statistics()[name])), name
    plain.close(), noisy.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_mask_reaches_the_flux_observer(dtype):
    """Cont-CC-SCIM-v0 with a FluxObserver, held actions and a limit of 3: after a truncation the env -- psi_abs and psi_angle included --
    shows what a freshly reset env shows, so for the lanes that never terminate step k + 3 repeats step k bit for bit."""
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-SCIM-v0", n_envs=N_ENV, dtype=dtype, physical_system_wrappers=(ga.FluxObserver(),), max_episode_steps=M_ENV)
    fresh = ga.make("Cont-CC-SCIM-v0", n_envs=N_ENV, dtype=dtype, physical_system_wrappers=(ga.FluxObserver(),))
    a = _actions(env, N_ENV, seed=5)
    got, want = _run(env, a), _run(fresh, a, steps=M_ENV)
    lanes = ~torch.stack([g[3] for g in got]).bool().any(dim=0)
    print(f"flux observer {dtype}: lanes that never terminated {int(lanes.sum())} of {N_ENV}")
    assert int(lanes.sum()) > 0
    psi = env.state_names.index("psi_abs")
    assert (want[0][0][lanes, psi] != want[2][0][lanes, psi]).any()  # (the flux builds up within an episode: a reset shows)
    for k in range(STEPS):
        assert torch.equal(got[k][0][lanes], want[k % M_ENV][0][lanes]), k
        assert torch.equal(got[k][4][lanes], torch.full_like(got[k][4][lanes], k % M_ENV == M_ENV - 1)), k
    env.close(), fresh.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_graph_replay(dtype):
    """`bind_step` captured in a HIP graph and replayed 7 times == 7 eager steps, counters included (no per-call host state, no memsets)."""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(n_envs=N_ENV, dtype=dtype, reference_generator="default", seed=3, max_episode_steps=M_ENV, episode_statistics=True)
    eager, graphed = (ga.make("Cont-CC-PMSM-v0", **kw) for _ in range(2))
    a = _actions(eager, N_ENV, seed=13)
    side = torch.cuda.Stream()
    step, obs, reward, done = graphed.bind_step(a, stream=side)
    step_t, obs_t, reward_t, done_t = eager.bind_step(a)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start; the twin gets the same history
        for _ in range(2):
            step()
        graphed.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(2):
        step_t()
    eager.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    step_t()
    truncations = 0
    for k in range(1, STEPS + 1):  # (the capture itself ran nothing: replay k is step k)
        if k > 1:
            step_t()
        g.replay()
        torch.cuda.synchronize()
        for name, x, y in (("state", obs[0], obs_t[0]), ("refs", obs[1], obs_t[1]), ("reward", reward, reward_t), ("terminated", done, done_t),
                           ("truncated", graphed.truncated, eager.truncated)):
            assert torch.equal(x, y), (name, k)
        for name in FIELDS:
            assert torch.equal(_bits(graphed.episode_statistics()[name]), _bits(eager.episode_statistics()[name])), (name, k)
        truncations += int(graphed.truncated.sum())
    assert truncations > 0 and int(graphed.episode_statistics()["n_finished"].sum()) >= truncations
    eager.close(), graphed.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_checkpoint(dtype):
    """get_checkpoint() after step 4 into a fresh env: steps 5-7 and the counters are those of the uninterrupted run -- with constant
    references, and with the env id's default Wiener references, whose streams the checkpoint carries
    (tests/test_gpu_checkpoint_complete.py: every generator kind)."""
    import gym_electric_motor_amd as ga

    _checkpoint(dtype, lambda: [ga.ConstReferenceGenerator("i_sd", 0.1), ga.ConstReferenceGenerator("i_sq", -0.2)])
    _checkpoint(dtype, lambda: "default")


def _checkpoint(dtype, generator):
    import torch

    import gym_electric_motor_amd as ga

    mk = lambda: ga.make("Cont-CC-PMSM-v0", n_envs=N_ENV, dtype=dtype, max_episode_steps=M_ENV, episode_statistics=True, seed=23,  # noqa: E731
                         reference_generator=generator())
    first, second = mk(), mk()
    a = _actions(first, N_ENV, seed=17)
    _run(first, a, steps=4)
    ck = first.get_checkpoint()
    assert set(ck["episodes"]) == {"state", "reset_mask"} and int(ck["episodes"]["reset_mask"].sum()) == 0  # (step 3 truncated, step 4 did not)
    _run(first, a, steps=1, reset=False)
    _run(first, a, steps=1, reset=False)  # step 6 truncates: this checkpoint carries a pending reset
    ck6 = first.get_checkpoint()
    assert int(ck6["episodes"]["reset_mask"].sum()) > 0
    tail7 = _run(first, a, steps=1, reset=False)
    stats7 = {k: v.clone() for k, v in first.episode_statistics().items()}
    second.reset()
    second.set_checkpoint(ck)
    got = _run(second, a, steps=3, reset=False)
    third = mk()
    third.reset()
    third.set_checkpoint(ck6)
    got7 = _run(third, a, steps=1, reset=False)
    for run, env in ((got[-1], second), (got7[-1], third)):
        for name, x, y in zip(("state", "refs", "reward", "terminated", "truncated"), run, tail7[0]):
            assert torch.equal(x, y), name
        for name in FIELDS:
            assert torch.equal(_bits(env.episode_statistics()[name]), _bits(stats7[name])), name
    assert float(stats7["last_ret"].abs().sum()) > 0
    if generator() == "default":  # the comparison saw references that move: the walk's steps, and the restarts after steps 3 and 6
        assert not torch.equal(got[0][1], got[1][1]) and not torch.equal(got[-1][1], got[-2][1])
    for e in (first, second, third):
        e.close()


def test_each_keyword_alone():
    """`max_episode_steps` alone still truncates (and hands out no statistics); `episode_statistics=True` alone never truncates, and its
    `ret` is the float64 sum of the returned rewards (`last_ret` where an episode terminated); the rollouts run the statistics pass."""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(n_envs=N_ENV, reference_generator="default", seed=9)
    limited = ga.make("Cont-CC-PMSM-v0", max_episode_steps=M_ENV, **kw)
    a = _actions(limited, N_ENV, seed=19)
    got = _run(limited, a)
    alive = ~torch.stack([g[3] for g in got]).bool().any(dim=0)
    assert int(alive.sum()) > 0 and all(bool(got[k][4][alive].all()) == (k in (2, 5)) and bool(got[k][4][alive].any()) == (k in (2, 5)) for k in range(STEPS))
    with pytest.raises(ValueError):
        limited.episode_statistics()
    counted = ga.make("Cont-CC-PMSM-v0", episode_statistics=True, **kw)
    got = _run(counted, a)
    assert all(g[4] is False for g in got)
    rewards, done = torch.stack([g[2] for g in got]).double(), torch.stack([g[3] for g in got]).bool()
    stats = counted.episode_statistics()
    total = torch.zeros(N_ENV, dtype=torch.float64, device="cuda")
    for k in range(STEPS):  # sequential, as the stage adds
        total = torch.where(done[k], torch.zeros_like(total), total + rewards[k])
    assert torch.equal(_bits(stats["ret"]), _bits(total))
    alive = ~done.any(dim=0)
    assert int(alive.sum()) > 0 and bool((stats["length"][alive] == STEPS).all()) and int(stats["n_finished"].sum()) == int(done.sum())
    # the complete rollout: the pass over its reward and done rows continues the counters where the steps left them
    from episode_restatement import Episodes

    K = 5
    want = Episodes(N_ENV)
    want.length, want.ret, want.last_length, want.last_ret, want.n_finished = (stats[n].cpu().numpy().copy() for n in FIELDS)
    actions = a[None].expand(K, *a.shape).contiguous()
    state, refs, reward, done_rows, ep = counted.rollout_complete(actions, episode_statistics=True)
    torch.cuda.synchronize()
    rows = want.rows(done_rows.cpu().numpy(), reward.cpu().numpy())
    assert torch.equal(ep["ended"], done_rows) and set(ep) == {"ended", "finished_return", "finished_length"}
    for name in ("ended", "finished_return", "finished_length"):
        _same(ep[name], rows[name], name)
    for name, w in want.fields().items():
        _same(counted.episode_statistics()[name], w, name)
    assert len(counted.rollout_complete(actions)) == 4
    with pytest.raises(NotImplementedError, match="episode time limit"):
        limited.rollout_complete(actions)
    limited.close(), counted.close()
