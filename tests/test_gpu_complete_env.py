"""GPU tests of the complete batched env (`make(env_id, reference_generator=..., reward_function=...)`) and of the fused generator step
behind it (gemx_refgen_step): bit-equality with the generator's rollout, the shell's semantics against the reference's recorded runs,
the default env end to end, the generator's distribution through `env.step`, and HIP-graph replay."""
import json
import os
import sys
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (sibling test module: fixture helpers)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

from test_gpu_parity import REWARD_CASES, _load, _make_from_meta  # noqa: E402


class _System:
    """What a generator's set_modules reads of a physical system (a PMSM's currents and speed), for generators tested on their own."""

    def __init__(self, ps, n_envs, dtype, env_base):
        import torch

        self.state_positions, self.state_space, self.nominal_state, self.limits = ps.state_positions, ps.state_space, ps.nominal_state, ps.limits
        self.n_envs, self.env_base, self.device = n_envs, env_base, ps.device
        self._tdev, self._tdtype = ps._tdev, dtype


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("states", [("i_sq",), ("i_sd", "i_sq"), ("omega", "i_sd", "i_sq"), ("omega", "torque", "i_sd", "i_sq")])
def test_fused_step_equals_rollout_bit_for_bit(dtype, states):
    """K x step(done[k-1]) == rollout(K, done), row for row; rollout / step / rollout mixed on one handle == one rollout; the generator
    state afterwards is the same.  N is no multiple of the workgroup size, env_base != 0, sub-episodes of 20..60 steps so that every
    stream passes many sub-episode ends, ~1 % terminations."""
    import torch

    import gym_electric_motor_amd as ga

    host = ga.make("Cont-CC-PMSM-v0", n_envs=2)
    n, K = 1000, 640
    ps = _System(host.physical_system, n, getattr(torch, dtype), env_base=12345)

    def gen():
        g = ga.BatchedWienerProcessReferenceGenerator(reference_states=states, seed=9, episode_lengths=(20, 60), sigma_range=(1e-2, 1e-1)).set_modules(ps)
        g.reset()
        return g

    rng = np.random.default_rng(4)
    done = torch.as_tensor((rng.random((K, n)) < 0.01).astype(np.uint8)).cuda()
    assert 0.005 < float(done.float().mean()) < 0.02
    a, b = gen(), gen()
    want = a.rollout(K, done=done)
    got = torch.empty_like(want)
    for k in range(K):
        got[k] = b.step(None if k == 0 else done[k - 1])
    torch.cuda.synchronize()
    assert want.dtype == getattr(torch, dtype) and tuple(want.shape) == (K, n, len(states))
    assert torch.equal(got, want)
    _, _, left = a.state()
    assert int(left.max()) < 60  # (sub-episodes did end: 640 steps of at most 60-step sub-episodes)
    b.reset(mask=done[K - 1])  # the rollout applied the last row's terminations already
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)
    # an `out=` tensor, and the two calls continue each other
    o = torch.empty((n, len(states)), dtype=want.dtype, device="cuda")
    assert b.step(out=o) is o and torch.equal(o, a.rollout(1)[0])
    # an `out=` view that is not aligned to a row (rows of 2 or 4 otherwise go out as one vector store): same values
    buf = torch.empty(n * len(states) + 1, dtype=want.dtype, device="cuda")
    o1 = buf[1:].view(n, len(states))
    assert o1.data_ptr() % (len(states) * o1.element_size()) != 0 or len(states) in (1, 3)
    b.step(out=o1)
    assert torch.equal(o1, a.rollout(1)[0])
    # mixed on one handle, no terminations
    c, d = gen(), gen()
    want = c.rollout(250)
    parts = [d.rollout(100)] + [d.step().clone()[None] for _ in range(50)] + [d.rollout(100)]
    assert torch.equal(torch.cat(parts), want)
    for x, y in zip(c.state(), d.state()):
        assert torch.equal(x, y)
    for g in (a, b, c, d):
        g.close()
    host.close()


@pytest.mark.parametrize("name", REWARD_CASES)
def test_shell_replays_the_reference_runs(name, monkeypatch):
    """The complete env on the reference's recorded runs (actions, references, rewards, terminated of `env.step` there), with the
    recorded references replayed: the observation after reset() shows references[0], after step k references[k+1]; the reward of step
    k is the recorded one (1e-4 x reward scale; the violation reward exactly), i.e. computed against references[k]; and everything
    equals the fused rollout on the same inputs bit for bit, which pins the off-by-one independently of any tolerance."""
    import torch

    import gym_electric_motor_amd as ga

    d, meta = _load(name)
    rw = meta["reward"]
    n_envs = 70
    cols = [i for i, r in enumerate(rw["referenced_states"]) if r]
    ref_states = [meta["state_names"][i] for i in cols]
    refs = d["references"][:, cols]
    K = d["actions"].shape[0]
    reward_kw = dict(reward_weights=np.array(rw["weights"]), reward_power=np.array(rw["powers"]), bias=rw["bias"], violation_reward=rw["violation_reward"])
    # the fixture helper builds its env with `ga.make(env_id, **kw)`; for this one call `make` also gets the two new keywords
    with monkeypatch.context() as mp:
        mp.setattr(ga, "make", partial(ga.make, reference_generator=ga.ReplayReferenceGenerator(refs, reference_states=ref_states), reward_function=reward_kw))
        env = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    assert isinstance(env, ga.CompleteBatchedElectricMotorEnv) and env.reference_names == ref_states
    ps = env.physical_system
    a = torch.as_tensor(np.repeat(d["actions"].reshape(K, 1, -1), n_envs, axis=1))
    if ps._discrete and d["actions"].ndim == 1:
        a = a.reshape(K, n_envs)
    a = a.cuda().to(ps._want_dtype).contiguous()
    refs32 = torch.as_tensor(refs).cuda().float()
    (state, ref), _ = env.reset()
    assert torch.equal(ref, refs32[0].expand(n_envs, -1))
    obs_l, rew_l, done_l, ref_l = [], [], [], []
    for k in range(K - 1):  # (the replay needs row k + 1)
        (state, ref), reward, terminated, truncated, _ = env.step(a[k])
        assert truncated is False
        obs_l.append(state.clone()), rew_l.append(reward.clone()), done_l.append(terminated.clone()), ref_l.append(ref.clone())
    torch.cuda.synchronize()
    obs, rew_t, done_t = torch.stack(obs_l), torch.stack(rew_l), torch.stack(done_l)
    assert torch.equal(torch.stack(ref_l), refs32[1:K, None, :].expand(-1, n_envs, -1))  # after step k: references[k + 1], every k
    rew, done = rew_t.double().cpu().numpy(), done_t.cpu().numpy().astype(bool)
    assert np.array_equal(rew[:, 0], rew[:, n_envs - 1])
    ref_done, ref_rew = d["terminated"][:K - 1], d["rewards"][:K - 1]
    first = int(np.argmax(done[:, 0] != ref_done)) if (done[:, 0] != ref_done).any() else K - 1
    print(f"{name}: first done flip {first} of {K - 1}")
    assert first > 100  # (a done flip at a < 1e-5 constraint margin ends the like-for-like comparison)
    scale = max(1.0, float(np.abs(ref_rew).max()))
    err = float(np.abs(rew[:first, 0] - ref_rew[:first]).max())
    print(f"{name}: max |reward - reference| {err:.3e} (bound {1e-4 * scale:.3e})")
    assert err < 1e-4 * scale
    viol = np.float32(rw["violation_reward"])
    assert (rew[:first, 0][ref_done[:first]] == viol).all()
    # the existing fused path on the same inputs
    env2 = _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)
    env2.physical_system.set_reward(referenced_states=ref_states, **reward_kw)
    o2, d2, r2 = env2.physical_system.rollout(a[:K - 1], references=refs32[:K - 1, None, :].expand(-1, n_envs, -1).contiguous())
    assert torch.equal(o2, obs) and torch.equal(d2, done_t) and torch.equal(r2, rew_t)
    env.close()
    env2.close()


def _policy(state, ref, cols, gain=8.0):
    return (gain * (ref - state[:, cols])).clamp(-1, 1)


def test_default_env_end_to_end():
    """make("Cont-CC-PMSM-v0", reference_generator="default"): the reward recomputed in float64 on the host from the returned (state,
    previous ref, terminated) and the recorded default weights, at every one of the 2000 steps (1e-4 x reward scale, the scale being
    the largest |reward| outside terminations, at least 1; the violation reward exactly); references stay inside the margins; two
    half-size shards show the states and references of the whole env, bit for bit."""
    import torch

    import gym_electric_motor_amd as ga

    want = json.load(open(os.path.join(GOLDEN, "env_defaults.json")))["Cont-CC-PMSM-v0"]
    n, K = 4096, 2000
    dq = (ga.DqToAbcActionProcessor.make("PMSM"),)
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=3, physical_system_wrappers=dq)
    halves = [ga.make("Cont-CC-PMSM-v0", n_envs=n // 2, reference_generator="default", seed=3, physical_system_wrappers=dq, env_base=b) for b in (0, n // 2)]
    ps = env.physical_system
    assert env.reference_names == want["reference_names"] == ["i_sd", "i_sq"]
    cols = [ps.state_positions[s] for s in env.reference_names]
    w = np.array(want["reward"]["_reward_weights"])
    length = ps.state_space.high - ps.state_space.low
    lo, hi = np.array(want["reference_space"]["low"]), np.array(want["reference_space"]["high"])
    (state, ref), _ = env.reset()
    hobs = [h.reset()[0] for h in halves]
    assert torch.equal(torch.cat([o[1] for o in hobs]), ref)
    n_term, worst, scale = 0, 0.0, 1.0
    power, bias, viol = np.array(want["reward"]["_n"]), want["reward"]["_bias"], want["reward"]["_violation_reward"]
    for k in range(K):  # every step: the reward against the reference shown BEFORE the step, margins, shards == whole
        prev = ref.double().cpu().numpy()
        action = _policy(state, ref, cols)
        hact = [_policy(o[0], o[1], cols) for o in hobs]
        (state, ref), reward, terminated, _, _ = env.step(action)
        hobs = [h.step(a_)[0] for h, a_ in zip(halves, hact)]
        s, r, t = state.double().cpu().numpy(), reward.double().cpu().numpy(), terminated.cpu().numpy().astype(bool)
        ref_full = np.zeros_like(s)
        ref_full[:, cols] = prev
        host = -(w * (np.abs(s - ref_full) / length) ** power).sum(axis=1) + bias
        scale = max(scale, float(np.abs(host[~t]).max()) if (~t).any() else 0.0)
        host[t] = viol
        worst = max(worst, float(np.abs(r - host).max()))
        assert (r[t] == np.float32(viol)).all()
        now = ref.double().cpu().numpy()
        assert (now >= lo - 1e-6).all() and (now <= hi + 1e-6).all(), k
        n_term += int(t.sum())
        assert torch.equal(torch.cat([o[1] for o in hobs]), ref), k
        assert torch.equal(torch.cat([o[0] for o in hobs]), state), k
    print(f"default env: max |reward - host float64| {worst:.3e} (bound {1e-4 * scale:.3e}), {n_term} terminations seen")
    assert worst < 1e-4 * scale
    # (what a terminated env shows next is asserted in test_terminated_envs_show_a_fresh_reference: this policy rarely terminates)
    for e in [env] + halves:
        e.close()


def test_terminated_envs_show_a_fresh_reference():
    """Free-running envs under full voltage terminate quickly: the reference an env shows right after its termination is the first value
    of a restarted generator -- uniform over the initial range (= the margin), stepped once --, not the continued walk."""
    import torch
    from scipy import stats

    import gym_electric_motor_amd as ga

    n = 4096
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=11)
    twin = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=11)
    lo, hi = env.reference_space.low, env.reference_space.high
    (state, ref), _ = env.reset()
    twin.reset()
    gen = twin.reference_generator  # the same generators without terminations: the continued walk
    action = torch.ones((n, 3), device="cuda") * torch.tensor([1.0, -1.0, -1.0], device="cuda")
    seen = np.zeros(n, dtype=bool)
    fresh = np.zeros((n, 2))
    for k in range(400):
        (state, ref), reward, terminated, _, _ = env.step(action)
        cont = gen.step()
        t = terminated.cpu().numpy().astype(bool) & ~seen
        if t.any():
            r = ref.double().cpu().numpy()
            if not seen.any():  # up to the first termination both generators are the same streams
                assert torch.equal(ref[~torch.as_tensor(t).cuda()], cont[~torch.as_tensor(t).cuda()])
            fresh[t] = r[t]
            seen |= t
        if seen.all():
            break
    assert seen.mean() > 0.9, seen.mean()
    for j in range(2):
        x = fresh[seen, j]
        assert x.min() >= lo[j] - 1e-6 and x.max() <= hi[j] + 1e-6
        assert stats.kstest(x, stats.uniform(lo[j], hi[j] - lo[j]).cdf).pvalue > 1e-4  # ~ U(margin) + one small clipped step
    env.close()
    twin.close()


def test_default_generator_distribution_through_env_step():
    """The KS comparison of tests/test_gpu_parity.py::test_device_wiener_reference_generator_matches_reference_distribution (same
    fixture, same thresholds), with the sequence collected through `env.step` of the complete env instead of `rollout`."""
    import torch
    from scipy import stats

    import gym_electric_motor_amd as ga

    w = np.load(os.path.join(GOLDEN, "wiener_samples.npz"))
    n, K = 4096, 451
    # (no constraints: no terminations, so every stream stays inside its first sub-episode of >= 500 steps)
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator="default", seed=77, constraints=())
    gen = env.reference_generator
    assert np.allclose([[gen._cfg.margin_lo[j], gen._cfg.margin_hi[j]] for j in range(2)], w["margins"], rtol=1e-14)
    lo, hi = w["margins"][0]
    gen.reset()
    v0, _, _ = gen.state()
    for j in range(2):  # reset(): initial reference ~ U(initial_range = limit margin)
        assert stats.ks_2samp(v0[j].cpu().numpy(), w["initial_values"][:, j]).pvalue > 1e-3
    (state, ref), _ = env.reset()
    _, sg, left = gen.state()
    sg, left = sg.cpu().numpy(), left.cpu().numpy()
    seq = [ref.double().cpu().numpy()]
    action = torch.zeros((n, 3), device="cuda")
    for k in range(K - 1):
        (state, ref), reward, terminated, _, _ = env.step(action)
        seq.append(ref.double().cpu().numpy())
    assert not bool(terminated.any())
    seq = np.stack(seq)  # [451, N, 2]
    assert seq.min() >= lo - 1e-6 and seq.max() <= hi + 1e-6
    for j in range(2):
        assert stats.ks_2samp(np.log10(sg[j]), np.log10(w[f"sub_sigma_{j}"])).pvalue > 1e-3
        assert stats.ks_2samp((left[j] + 1).astype(float), w[f"sub_len_{j}"].astype(float)).pvalue > 1e-3
        assert left[j].min() + 1 >= 500 and left[j].max() + 1 < 2000
        s = seq[:, :, j]
        dz = np.diff(s, axis=0) / sg[j][None, :]
        inside = (s[1:] > lo + 1e-4) & (s[1:] < hi - 1e-4) & (s[:-1] > lo + 1e-4) & (s[:-1] < hi - 1e-4) & (sg[j][None, :] > 3e-3)
        z = dz[inside][:200000]  # (fp32 storage: keep sigmas whose steps are well above the rounding of values ~0.5)
        assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
        assert stats.ks_2samp(z[:20000], w[f"z_{j}"][:20000]).pvalue > 1e-3
    env.close()


def test_bound_step_in_a_hip_graph_equals_eager_steps():
    """One `bind_step` step (policy + physics/reward launch + generator launch) captured with torch.cuda.graph and replayed 200 times
    equals 200 eager steps of a twin env bit for bit -- state, reference, reward, done.  A step index kept on the host would freeze
    the replayed generators at the captured step."""
    import torch

    import gym_electric_motor_amd as ga

    n = 1000
    dq = (ga.DqToAbcActionProcessor.make("PMSM"),)
    kw = dict(n_envs=n, reference_generator="default", seed=5, physical_system_wrappers=dq)

    def loop(env, stream):
        """-> (control_step, state, ref, reward, done) with the stepper bound to `stream`"""
        ps = env.physical_system
        cols = torch.tensor([ps.state_positions[s] for s in env.reference_names], device="cuda")
        gain = torch.tensor(8.0, device="cuda")
        action = torch.zeros((n, 2), device="cuda")
        step, (state, ref), reward, done = env.bind_step(action, stream=stream)

        def control_step():
            torch.clamp(gain * (ref - state.index_select(1, cols)), -1, 1, out=action)  # "policy": proportional dq current controller
            step()

        return control_step, state, ref, reward, done

    env, twin = ga.make("Cont-CC-PMSM-v0", **kw), ga.make("Cont-CC-PMSM-v0", **kw)
    side = torch.cuda.Stream()
    control, state, ref, reward, done = loop(env, side)
    control_t, state_t, ref_t, reward_t, done_t = loop(twin, torch.cuda.current_stream())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start
        for _ in range(3):
            control()
        env.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(3):  # the twin has the same history: reset() restarts the generators, the step index of their draws runs on
        control_t()
    twin.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        control()
    torch.cuda.synchronize()
    assert torch.equal(ref, ref_t)  # (the capture executed nothing)
    ref0 = ref.clone()
    for k in range(200):
        graph.replay()
        control_t()
        if k % 20 == 19 or k < 3:
            torch.cuda.synchronize()
            assert torch.equal(state, state_t) and torch.equal(ref, ref_t) and torch.equal(reward, reward_t) and torch.equal(done, done_t), k
    torch.cuda.synchronize()
    assert not torch.equal(ref, ref0)  # the replays advanced the generators
    assert torch.equal(state, state_t) and torch.equal(ref, ref_t) and torch.equal(reward, reward_t) and torch.equal(done, done_t)
    env.close()
    twin.close()


def test_physics_only_env_is_unchanged_and_kernel_is_covered(tmp_path):
    """make() without the new keywords: step() still returns reward None; the instantiation coverage names the new kernel."""
    import subprocess

    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=64, reference_generator=None, reward_function=None)
    obs, reward, terminated, truncated, info = env.step(torch.zeros((64, 3), device="cuda"))
    assert reward is None and tuple(obs.shape) == (64, 14) and truncated is False
    env.close()
    cov = tmp_path / "cov.txt"
    code = ("import gym_electric_motor_amd as ga, torch\n"
            "for dt in ('float32', 'float64'):\n"
            "    e = ga.make('Cont-CC-PMSM-v0', n_envs=64, reference_generator='default', dtype=dt)\n"
            "    e.reset(); e.step(torch.zeros((64, 3), device='cuda', dtype=getattr(torch, dt))); torch.cuda.synchronize(); e.close()\n")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=repo, env=dict(os.environ, GEMX_COVERAGE_FILE=str(cov)), timeout=300)
    names = set(cov.read_text().split("\n"))
    assert {"refgen_step_kernel<float>", "refgen_step_kernel<double>"} <= names, sorted(x for x in names if "refgen" in x)


def test_replay_generator_columns_follow_the_callers_order_and_refuse_capture(monkeypatch):
    """ReplayReferenceGenerator(refs, reference_states=(...)) names the state of each column in the columns' order; the env shows them in
    the state order of the physical system.  Its row index is host state: stepping under graph capture is refused, not replayed wrong."""
    import torch

    import gym_electric_motor_amd as ga

    n = 64
    prof = np.stack([np.linspace(0.1, 0.5, 6), np.linspace(-0.5, -0.1, 6)], axis=1)  # column 0: i_sq, column 1: i_sd
    env = ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator=ga.ReplayReferenceGenerator(prof, reference_states=("i_sq", "i_sd")))
    assert env.reference_names == ["i_sd", "i_sq"]
    (state, ref), _ = env.reset()
    want = torch.as_tensor(prof[:, ::-1].copy()).float().cuda()
    assert torch.equal(ref, want[0].expand(n, -1))
    action = torch.zeros((n, 3), device="cuda")
    (state, ref), reward, _, _, _ = env.step(action)
    assert torch.equal(ref, want[1].expand(n, -1))
    ps = env.physical_system
    host = -(0.5 * (state[:, ps.state_positions["i_sd"]] - want[0, 0]).abs() / 2 + 0.5 * (state[:, ps.state_positions["i_sq"]] - want[0, 1]).abs() / 2)
    assert torch.allclose(reward, host, atol=2e-6)
    step, _, _, _ = env.bind_step(action)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)  # (no real capture is opened only to be broken off)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        step()
    monkeypatch.undo()
    step()
    assert torch.equal(ref, want[2].expand(n, -1))
    torch.cuda.synchronize()
    env.close()
