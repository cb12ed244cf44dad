"""GPU tests of the complete env's fused K-step rollouts: `rollout_complete` / `rollout_complete_synthetic` / `bind_rollout_complete`
(physics rollout -> generator rollout in the shell's order -> reward pass over the stored trajectory) against K calls of `step()`, the
reward pass (gemx_reward_rows) against the fused reward of gemx_rollout_reward, and the shell-order generator rollout
(gemx_refgen_rollout_shell) against K x gemx_refgen_step.  Every comparison is `torch.equal` on two identically seeded envs (or one env
and the C ABI); the recorded runs of the reference tie the reward pass to the reference's own `env.step()` rewards."""
import ctypes as C
import os
import sys
from functools import partial

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (sibling test modules: cases and fixture helpers)

import reward_path_cases as rp  # noqa: E402
from parity_contract import TOL_FP32  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------------------
# Actions under which some envs terminate again and again and the others never do, fixed once.  Every third env (by GLOBAL index) is
# "hot": a constant duty cycle near full scale -- the armature current of the DC machines passes its limit within a step or two at
# 60 V over 16 mOhm, the PMSM's stator current within a few steps at some 80 A per step --; the others are "calm": duty cycles within
# +-0.005, i.e. a fraction of a volt (the currents stay far below the limits; a PMSM at 100 rad/s feeds some tens of amperes into the
# shorted terminals).  Finite B6 bridge: the hot envs hold one active vector, the calm ones alternate the two zero vectors.
ENVS = {
    "Cont-CC-PMSM-v0": dict(kw={}, states=("i_sd", "i_sq")),
    "Cont-SC-PermExDc-v0": dict(kw={}, states=("omega", "i")),
    "Finite-CC-PMSM-v0": dict(kw=dict(tau=1e-4), states=("i_sd", "i_sq")),
    "Cont-CC-ShuntDc-v0": dict(kw=dict(physical_system_wrappers="default"), states=("i_a", "i_e")),
}
SEED = 11


def _actions(ps, K, n, env_base=0, seed=0):
    import torch

    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    hot = ((torch.arange(n) + env_base) % 3 == 0)
    if ps._discrete:
        calm = torch.where(torch.arange(K)[:, None] % 2 == 0, 0, 7).expand(K, n)
        return torch.where(hot[None, :], torch.ones((K, n), dtype=torch.long), calm).to(torch.uint8).cuda().contiguous()
    A = ps._n_act
    # (drawn for the global env index so that shards see the actions of the whole env)
    noise = torch.rand((K, env_base + n, A), generator=g, dtype=torch.float64)[:, env_base:] * 2 - 1
    sign = torch.tensor([1.0] + [-1.0] * (A - 1), dtype=torch.float64)
    a = torch.where(hot[None, :, None], 0.95 * sign + 0.05 * noise, 0.005 * noise)
    return a.to(ps._tdtype).cuda().contiguous()


def _generator(ga, env_id, kind):
    from gym_electric_motor_amd.envs import default_env_modules

    if kind == "default":  # the env id's Wiener generators (the all-Wiener kernels), with sub-episodes that turn over inside the run
        m = default_env_modules(env_id)
        return ga.BatchedWienerProcessReferenceGenerator(reference_states=m["reference_states"], seed=SEED, **dict(m["generator"], episode_lengths=(3, 9)))
    s0, s1 = ENVS[env_id]["states"]  # a mixed list: refgen_kinds_kernel
    return [ga.SinusoidalReferenceGenerator(reference_state=s0, episode_lengths=(3, 9), frequency_range=(50, 500)),
            ga.StepReferenceGenerator(reference_state=s1, episode_lengths=(3, 9), frequency_range=(100, 800), amplitude_range=(0.05, 0.3))]


def _make(ga, env_id, kind, n, **extra):
    kw = dict(ENVS[env_id]["kw"], **extra)
    return ga.make(env_id, n_envs=n, reference_generator=_generator(ga, env_id, kind), seed=SEED, **kw)


def _steps(torch, env, acts):
    """K x step() -> (state, refs, reward, done) stacked; a flat observation is its own first item, the references come from the generator."""
    rows = ([], [], [], [])
    for k in range(acts.shape[0]):
        obs, reward, terminated, truncated, _ = env.step(acts[k])
        state = obs[0] if isinstance(obs, tuple) else obs
        for lst, t in zip(rows, (state, env.reference_generator.references, reward, terminated)):
            lst.append(t.clone())
    return tuple(torch.stack(r) for r in rows)


def _same(torch, got, want, what):
    for name, g, w in zip(("state", "refs", "reward", "done"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert torch.equal(g, w), (what, name, int((g != w).sum()), "of", g.numel())


# ------------------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind", ["default", "mixed"])
@pytest.mark.parametrize("env_id", sorted(ENVS))
def test_rollout_equals_k_steps(env_id, kind):
    """rollout_complete(actions) == K x step(actions[k]) bit for bit on state, refs, reward and done, for N in {1, 37, 300} and, on
    each pair of envs one after the other, K in {1, 2, 64} (so the later rollouts also start from a used env).  Where both can hold at
    all -- more than one env, and rows strictly inside the run: N > 1, K = 64 -- the run must contain a termination strictly inside
    it and an env that never terminates; with one env, or with one or two rows, the two exclude each other by construction."""
    import torch

    import gym_electric_motor_amd as ga

    for n in (1, 37, 300):
        a, b = _make(ga, env_id, kind, n), _make(ga, env_id, kind, n)
        assert isinstance(a, ga.CompleteBatchedElectricMotorEnv)
        a.reset(), b.reset()
        for j, K in enumerate((1, 2, 64)):
            acts = _actions(a.physical_system, K, n, seed=j)
            got = a.rollout_complete(acts)
            want = _steps(torch, b, acts)
            torch.cuda.synchronize()
            _same(torch, got, want, f"{env_id} {kind} N={n} K={K}")
            assert torch.equal(a.reference_generator.references, got[1][K - 1])  # row K-1 is what the env shows now
            done = got[3].bool()
            print(f"{env_id} {kind} N={n} K={K}: {int(done.sum())} terminations, {int((~done.any(dim=0)).sum())} envs without one")
            if n > 1 and K == 64:
                assert bool(done[1:K - 1].any()), "no termination strictly inside the run: the reset order is untested"
                assert bool((~done.any(dim=0)).any()), "every env terminated"
                assert bool((got[2][done] == a.reward_config.violation_reward).all())
        a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2
def _reward_rows(torch, ps, obs, first, rows, done, K):
    out = torch.full((K, ps.n_envs), float("nan"), dtype=ps._tdtype, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    rc = ps._L.gemx_reward_rows(ps._handle, ptr(obs), ptr(first), ptr(rows), ptr(done), K, ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, ps._L.gemx_last_error().decode()
    return out


def _fused_and_pass(torch, ga, case, dtype, n, K, rng, offset_view=False):
    env = ga.make(case.env_id, n_envs=n, dtype=dtype, auto_reset=True)
    ps = env.physical_system
    ps.set_reward(referenced_states=case.ref_names, **case.set_reward_kwargs)
    tdt = getattr(torch, dtype)
    n_ref = len(case.ref_cols)
    sp = ps.action_space
    if hasattr(sp, "nvec"):
        acts = np.stack([rng.integers(0, int(v), (K, n)) for v in sp.nvec], axis=-1).astype(np.uint8)
    else:
        acts = rng.uniform(np.asarray(sp.low, dtype=np.float64), np.asarray(sp.high, dtype=np.float64), (K, n) + tuple(sp.shape))
    R = torch.as_tensor(rng.uniform(-0.8, 0.8, (K + 1, n, n_ref))).to(device="cuda", dtype=tdt).contiguous()
    obs, done, fused = ps.rollout(acts, references=R[:K] if n_ref else None, reward_out=None if n_ref else torch.empty((K, n), dtype=tdt, device="cuda"))
    if offset_view:  # the same rows in a view one element off: 4-byte aligned fp32 / 8-byte aligned fp64 -> the dword path
        buf = torch.empty(obs.numel() + 1, dtype=tdt, device="cuda")
        view = buf[1:].view(obs.shape)
        view.copy_(obs)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        obs = view
    got = _reward_rows(torch, ps, obs, R[0] if n_ref else None, R[1:] if n_ref else None, done, K)
    torch.cuda.synchronize()
    env.close()
    return fused, got, done


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", sorted(rp.SHAPES))
def test_reward_pass_equals_the_fused_reward(shape, dtype):
    """gemx_reward_rows on the obs / done a fused-reward rollout wrote, with refs_first = R[0] and refs_rows[k] = R[k + 1], returns the
    fused reward bit for bit: every shape of tests/reward_path_cases.py (0, 1 and 4 references, up to 24 terms, powers 1, 2, 0.5 and 3,
    also past term 4, both bias forms), N in {1, 3, 37, 257}, K in {1, 3, 5}."""
    import torch

    import gym_electric_motor_amd as ga

    case = rp.Case(shape)
    rng = np.random.default_rng(sum(map(ord, shape + dtype)))
    for n in (1, 3, 37, 257):
        for K in (1, 3, 5):
            fused, got, done = _fused_and_pass(torch, ga, case, dtype, n, K, rng)
            assert got.dtype == fused.dtype and torch.equal(got, fused), (shape, dtype, n, K, int((got != fused).sum()))
            assert bool((got[done.bool()] == case.violation_reward).all())


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", ["series_nref4_weight0", "shunt_all6_p3_beyond", "eesm_all16_general", "dfim_nref4_all24", "dfim_nref0_4"])
def test_reward_pass_on_an_offset_view_and_around_a_tile(shape, dtype):
    """The element-aligned (dword) path -- `obs` a view offset by one element --, and K * N one row less and one row more than a tile
    (256 fp32 rows, 128 fp64 rows), aligned and offset: the fused reward's bits."""
    import torch

    import gym_electric_motor_amd as ga

    case = rp.Case(shape)
    rng = np.random.default_rng(sum(map(ord, shape + dtype)) + 1)
    tile = 256 if dtype == "float32" else 128
    for n, K, off in ((37, 5, True), (257, 3, True), (tile - 1, 1, False), (tile + 1, 1, False), (tile - 1, 1, True), (tile + 1, 1, True),
                      ((tile + 2) // 3, 3, False), ((tile - 2) // 3, 3, True)):
        fused, got, done = _fused_and_pass(torch, ga, case, dtype, n, K, rng, offset_view=off)
        assert torch.equal(got, fused), (shape, dtype, n, K, off, int((got != fused).sum()))


def test_reward_pass_refuses_what_it_cannot_serve():
    import torch

    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=8)
    ps = env.physical_system
    obs, done = env.rollout(torch.zeros((2, 8, 3), device="cuda"))
    out = torch.empty((2, 8), device="cuda")
    call = lambda p, K=2: p._L.gemx_reward_rows(p._handle, C.c_void_p(obs.data_ptr()), None, None, C.c_void_p(done.data_ptr()), K, C.c_void_p(out.data_ptr()), None)  # noqa: E731
    assert call(ps) != 0 and b"no reward function" in ps._L.gemx_last_error()
    ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=())
    assert call(ps) == 0
    assert call(ps, 0) != 0
    ps.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=("i_sd", "i_sq"))
    assert call(ps) != 0  # a reward with references needs them
    ps.set_reward(reward_weights=False)
    assert call(ps) != 0
    soa = ga.make("Cont-CC-PMSM-v0", n_envs=8, obs_layout="soa")
    soa.physical_system.set_reward(reward_weights=dict(i_sd=0.5, i_sq=0.5), referenced_states=())
    assert call(soa.physical_system) != 0 and b"AOS" in ps._L.gemx_last_error()
    torch.cuda.synchronize()
    env.close(), soa.close()


# ------------------------------------------------------------------------------------------------------------------------------ 3
class _System:
    """What a generator's set_modules reads of a physical system, for generators tested on their own."""

    def __init__(self, ps, n_envs, dtype, env_base):
        self.state_positions, self.state_space, self.nominal_state, self.limits = ps.state_positions, ps.state_space, ps.nominal_state, ps.limits
        self.state_names, self.tau = ps.state_names, ps.tau
        self.n_envs, self.env_base, self.device = n_envs, env_base, ps.device
        self._tdev, self._tdtype = ps._tdev, dtype


def _standalone(ga, torch, kind, dtype, n):
    host = ga.make("Cont-CC-PMSM-v0", n_envs=2)
    ps = _System(host.physical_system, n, getattr(torch, dtype), env_base=777)

    def gen():
        if kind == "wiener":
            g = ga.BatchedWienerProcessReferenceGenerator(reference_states=("omega", "i_sd", "i_sq"), seed=9, episode_lengths=(3, 9), sigma_range=(1e-2, 1e-1))
        else:
            g = ga.BatchedMultipleReferenceGenerator([ga.SinusoidalReferenceGenerator(reference_state="i_sd", episode_lengths=(3, 9), frequency_range=(50, 500)),
                                                      ga.StepReferenceGenerator(reference_state="i_sq", episode_lengths=(4, 11), frequency_range=(100, 800)),
                                                      ga.WienerProcessReferenceGenerator(reference_state="omega", episode_lengths=(3, 9)),
                                                      ga.LaplaceProcessReferenceGenerator(reference_state="torque", episode_lengths=(2, 5))], seed=9)
        g.set_modules(ps)
        g.reset()
        return g

    return host, gen


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind", ["wiener", "mixed"])
def test_shell_order_generator_rollout_equals_k_steps(kind, dtype):
    """rollout_shell(K, done) == K x step(done[k]) row for row, ~5 % ones in the masks, N no multiple of the workgroup size, a global
    env offset; and rollout_shell, step and rollout mixed on one handle == the same sequence made of steps alone."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 300, 64
    host, gen = _standalone(ga, torch, kind, dtype, n)
    rng = np.random.default_rng(4)
    done = torch.as_tensor((rng.random((K, n)) < 0.05).astype(np.uint8)).cuda()
    assert 0.03 < float(done.float().mean()) < 0.07
    a, b = gen(), gen()
    got = a.rollout_shell(K, done)
    want = torch.stack([b.step(done[k]).clone() for k in range(K)])
    torch.cuda.synchronize()
    assert got.dtype == getattr(torch, dtype) and torch.equal(got, want)
    assert not torch.equal(got, gen().rollout(K, done))  # (the other order gives other rows: the masks matter)
    for k_ in (1, 2):
        assert torch.equal(a.rollout_shell(k_, done[:k_]), torch.stack([b.step(done[k]).clone() for k in range(k_)]))
    assert torch.equal(a.rollout_shell(3), torch.stack([b.step().clone() for _ in range(3)]))  # no mask at all
    # mixed on one handle: rollout_shell, step, rollout (which resets AFTER its rows; its last mask row is empty, so that nothing is
    # pending when the next call begins), rollout_shell again, with an `out=` tensor
    c, d = gen(), gen()
    d2 = done[20:30].clone()
    d2[-1] = 0
    out = torch.empty((12, n, got.shape[-1]), dtype=got.dtype, device="cuda")
    parts = [c.rollout_shell(7, done[:7]), c.step(done[7]).clone()[None], c.rollout(10, d2), c.rollout_shell(12, done[40:52], out=out)]
    assert parts[3] is out
    masks = [done[k] for k in range(8)] + [None] + [d2[k] for k in range(9)] + [done[40 + k] for k in range(12)]
    steps = torch.stack([d.step(m).clone() for m in masks])
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts), steps)
    for x, y in zip(c.state(), d.state()) if kind == "wiener" else zip(c.state().values(), d.state().values()):
        assert torch.equal(x, y)
    for g in (a, b, c, d):
        g.close()
    host.close()


# ------------------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("kind", ["default", "mixed"])
def test_chunks(kind):
    """Chunks of 3 + 1 + 5 equal one rollout of 9; rollout_complete(4), two step()s, rollout_complete(3) equal nine steps."""
    import torch

    import gym_electric_motor_amd as ga

    n, env_id = 100, "Cont-CC-PMSM-v0"
    envs = [_make(ga, env_id, kind, n) for _ in range(4)]
    for e in envs:
        e.reset()
    acts = _actions(envs[0].physical_system, 9, n)
    whole = envs[0].rollout_complete(acts)
    parts = [tuple(t.clone() for t in envs[1].rollout_complete(acts[i:j])) for i, j in ((0, 3), (3, 4), (4, 9))]
    _same(torch, tuple(torch.cat(ts) for ts in zip(*parts)), whole, "3 + 1 + 5")
    first = tuple(t.clone() for t in envs[2].rollout_complete(acts[:4]))
    mid = _steps(torch, envs[2], acts[4:6])
    last = envs[2].rollout_complete(acts[6:])
    nine = _steps(torch, envs[3], acts)
    torch.cuda.synchronize()
    _same(torch, tuple(torch.cat(ts) for ts in zip(first, mid, last)), nine, "4 + step + step + 3")
    _same(torch, whole, nine, "9")
    assert bool(whole[3].any()) and bool((~whole[3].bool().any(dim=0)).any())
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("flat", [True, False])
def test_observation_stage(flat):
    """CosSinProcessor with observed_states (and flatten_observation): the processed / flat trajectory of a rollout equals K steps."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 37, 20
    extra = dict(physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True),), observed_states=["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"],
                 flatten_observation=flat)
    a, b = _make(ga, "Cont-CC-PMSM-v0", "default", n, **extra), _make(ga, "Cont-CC-PMSM-v0", "default", n, **extra)
    a.reset(), b.reset()
    acts = _actions(a.physical_system, K, n)
    got = a.rollout_complete(acts)
    want = _steps(torch, b, acts)
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (K, n, 7 if flat else 5)
    _same(torch, got, want, f"observation stage flat={flat}")
    if flat:
        assert torch.equal(got[0][..., 5:], got[1])
    assert bool(got[3].any())
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("kind", ["default", "mixed"])
def test_shards(kind):
    """Two half-size envs with env_base equal one whole env, over the rollout."""
    import torch

    import gym_electric_motor_amd as ga

    n, K, env_id = 74, 30, "Cont-CC-PMSM-v0"
    whole = _make(ga, env_id, kind, n)
    halves = [_make(ga, env_id, kind, n // 2, env_base=b) for b in (0, n // 2)]
    whole.reset()
    acts = _actions(whole.physical_system, K, n)
    want = whole.rollout_complete(acts)
    got = []
    for h, b in zip(halves, (0, n // 2)):
        h.reset()
        got.append(h.rollout_complete(acts[:, b:b + n // 2].contiguous()))
    torch.cuda.synchronize()
    _same(torch, tuple(torch.cat(ts, dim=1) for ts in zip(*got)), want, "shards")
    assert bool(want[3].any())
    for e in [whole] + halves:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("flat", [False, True])
def test_bound_rollout_in_a_hip_graph_equals_eager_launches(flat):
    """bind_rollout_complete captured with torch.cuda.graph and replayed twice equals two eager launches of a twin's bound rollout, and
    those equal 2 K steps: the replays advance the physics and the generators."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 300, 16
    extra = dict(physical_system_wrappers=(ga.CosSinProcessor(),), flatten_observation=True) if flat else {}
    env, twin, stepper = (_make(ga, "Cont-CC-PMSM-v0", "default", n, **extra) for _ in range(3))
    acts = _actions(env.physical_system, K, n)

    def bound(e, stream):
        shapes = e._complete_shapes(K)
        outs = [torch.zeros(s, device="cuda") for s in shapes[:3]] + [torch.zeros(shapes[3], dtype=torch.uint8, device="cuda")]
        return e.bind_rollout_complete(acts, *outs, stream=stream), outs

    side = torch.cuda.Stream()
    launch, outs = bound(env, side)
    launch_t, outs_t = bound(twin, torch.cuda.current_stream())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start
        launch()
        env.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    launch_t()  # (the twins have the same history: reset() restarts the generators, the step index of their draws runs on)
    twin.reset()
    _steps(torch, stepper, acts)
    stepper.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    torch.cuda.synchronize()
    for i in range(2):
        graph.replay()
        assert launch_t() is not None
        want = _steps(torch, stepper, acts)
        torch.cuda.synchronize()
        _same(torch, tuple(outs), tuple(outs_t), f"replay {i}")
        _same(torch, tuple(outs), want, f"replay {i} against steps")
        assert torch.equal(env.reference_generator.references, outs[1][K - 1])
        if i == 0:
            first_refs = outs[1].clone()
    assert not torch.equal(first_refs, outs[1])  # the second replay went on
    for e in (env, twin, stepper):
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------ 8
def test_synthetic_actions():
    """rollout_complete_synthetic(K) == rollout_complete on the actions gemx_synthetic_actions reports for the same seed and step index,
    twice in a row (the default step index is the env's step count)."""
    import torch

    import gym_electric_motor_amd as ga

    n, K = 300, 24
    a, b = _make(ga, "Cont-CC-PMSM-v0", "default", n), _make(ga, "Cont-CC-PMSM-v0", "default", n)
    a.reset(), b.reset()
    for i in range(2):
        acts = b.physical_system.synthetic_actions(K, seed=5)
        got = a.rollout_complete_synthetic(K, seed=5)
        want = b.rollout_complete(acts)
        torch.cuda.synchronize()
        _same(torch, got, want, f"synthetic chunk {i}")
    want2 = _steps(torch, a, acts[:3])  # and step() goes on from there
    got2 = b.rollout_complete(acts[:3])
    _same(torch, got2, want2, "steps after a synthetic rollout")
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------------------------------ 9
from test_gpu_parity import REWARD_CASES, _load, _make_from_meta  # noqa: E402


@pytest.mark.parametrize("name", REWARD_CASES)
def test_rollout_on_the_reference_recorded_runs(name, monkeypatch):
    """The reference's recorded `env.step()` runs (actions, references, rewards, terminated), replayed through a
    ReplayReferenceGenerator and ONE rollout_complete: the references come out as recorded (row k is references[k + 1]); the rewards
    meet the recorded ones within the parity contract (1e-4 x reward scale, the violation reward exactly) up to the first done flip,
    which lies beyond step 100 -- the thresholds tests/test_gpu_complete_env.py applies to `env.step` --; and states, rewards and done
    masks equal those of a twin stepped K times, bit for bit."""
    import torch

    import gym_electric_motor_amd as ga

    d, meta = _load(name)
    rw = meta["reward"]
    n_envs = 70
    cols = [i for i, r in enumerate(rw["referenced_states"]) if r]
    ref_states = [meta["state_names"][i] for i in cols]
    refs = d["references"][:, cols]
    K = d["actions"].shape[0] - 1  # (the replay needs row k + 1)
    reward_kw = dict(reward_weights=np.array(rw["weights"]), reward_power=np.array(rw["powers"]), bias=rw["bias"], violation_reward=rw["violation_reward"])

    def make():
        with monkeypatch.context() as mp:
            mp.setattr(ga, "make", partial(ga.make, reference_generator=ga.ReplayReferenceGenerator(refs, reference_states=ref_states), reward_function=reward_kw))
            return _make_from_meta(meta, n_envs, dtype="float32", auto_reset=True)

    env, twin = make(), make()
    ps = env.physical_system
    a = torch.as_tensor(np.repeat(d["actions"].reshape(K + 1, 1, -1), n_envs, axis=1))
    if ps._discrete and d["actions"].ndim == 1:
        a = a.reshape(K + 1, n_envs)
    a = a.cuda().to(ps._want_dtype).contiguous()[:K]
    refs32 = torch.as_tensor(refs).cuda().float()
    env.reset(), twin.reset()
    state, ref_rows, rew_t, done_t = env.rollout_complete(a)
    want = _steps(torch, twin, a)
    torch.cuda.synchronize()
    _same(torch, (state, ref_rows, rew_t, done_t), want, name)
    assert torch.equal(ref_rows, refs32[1:K + 1, None, :].expand(-1, n_envs, -1))
    with pytest.raises(RuntimeError, match="cannot be captured"):
        env.bind_rollout_complete(a, state, ref_rows, rew_t, done_t)
    rew, done = rew_t.double().cpu().numpy(), done_t.cpu().numpy().astype(bool)
    assert np.array_equal(rew[:, 0], rew[:, n_envs - 1])
    ref_done, ref_rew = d["terminated"][:K], d["rewards"][:K]
    first = int(np.argmax(done[:, 0] != ref_done)) if (done[:, 0] != ref_done).any() else K
    print(f"{name}: first done flip {first} of {K}")
    assert first > 100
    scale = max(1.0, float(np.abs(ref_rew).max()))
    err = float(np.abs(rew[:first, 0] - ref_rew[:first]).max())
    print(f"{name}: max |reward - reference| {err:.3e} (bound {TOL_FP32 * scale:.3e})")
    assert err < TOL_FP32 * scale
    assert (rew[:first, 0][ref_done[:first]] == np.float32(rw["violation_reward"])).all()
    env.close(), twin.close()
