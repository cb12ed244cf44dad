"""Episodic rollouts on the device (csrc/gemx_episodic.hip, gemx_rollout_episodic): K fused steps with the episode time limit inside the
launch equal K calls of `step()` on a second env of the same seed, BIT FOR BIT -- state, references, reward, terminated, truncated, the
`episode_statistics` outputs, all five fields of the episode stage and the ODE state afterwards.  N = 197 (three full waves and a tail of
five lanes), K = 48, per-lane random actions.  What a case must exercise (lanes that truncate without ever terminating, lanes whose
truncation rows differ from lane 0's, a row where done and the limit coincide, no truncation at M = 1000) is asserted from the STEPPED
env's results, so that no comparison can pass empty.

test_every_unit_once runs one env per episodic unit and per (load, solver, table) form; test_against_the_float64_host_shell compares
with tests/env_shell_restatement.py, the reference that shares no code with the kernels (inputs: tests/episodic_rollout_cases.py)."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)  # (sibling modules)

N, K = 197, 48
EDGE_LANES = (0, 63, 64, 65, 196)
FIELDS = ("length", "ret", "last_length", "last_ret", "n_finished")
ENVS = {
    "Cont-CC-PermExDc-v0": dict(bias=0.275),  # (the duty cycle that balances the back-EMF of its constant speed: tests/env_parameters_cases.py)
    "Finite-CC-PMSM-v0": dict(),
    "Cont-SC-SCIM-v0": dict(),
    "dq-PMSM": dict(env_id="Cont-CC-PMSM-v0", control_space="dq"),
}


def _actions(torch, ps, n, k=K, seed=5):
    """Per-lane random actions [k, n, A] / [k, n] on the device, of the dtype the kernels read."""
    rng = np.random.default_rng(seed)
    space = ps.action_space
    if hasattr(space, "n") or hasattr(space, "nvec"):
        count = int(np.prod(space.nvec)) if hasattr(space, "nvec") else int(space.n)
        a = rng.integers(0, count, (k, n)).astype(np.uint8)
    else:
        amp = rng.uniform(0.0, 1.0, (1, n, 1)) ** 2  # per-lane amplitude: gentle lanes never terminate, rough ones every few steps
        a = np.clip(getattr(ps, "_test_bias", 0.0) + amp * rng.uniform(-1.0, 1.0, (k, n, int(space.shape[0]))), -1.0, 1.0).astype(np.float32)
    return torch.as_tensor(a).to(ps._tdev).contiguous()


def _make(ga, case, M, n=N, complete=True, **kw):
    spec = dict(ENVS.get(case, {}))
    env_id = spec.pop("env_id", case)
    bias = spec.pop("bias", 0.0)
    spec.update(kw)
    if complete:
        spec.setdefault("reference_generator", "default")
        spec.setdefault("seed", 3)
    env = ga.make(env_id, n_envs=n, max_episode_steps=M, episode_statistics=True, **spec)
    env.reset()
    env.physical_system._test_bias = bias  # (read by _actions)
    return env


def _state_of(torch, obs):
    return obs if torch.is_tensor(obs) else obs[0]


def _stepped(torch, env, acts):
    """K calls of `step` -> dict of stacked tensors, the `episode_statistics` outputs restated from the stage's fields after every step."""
    out = {k: [] for k in ("state", "refs", "reward", "terminated", "truncated", "ended", "finished_return", "finished_length")}
    complete = hasattr(env, "reference_generator")
    for k in range(acts.shape[0]):
        obs, reward, term, trunc, _ = env.step(acts[k])
        ended = term.bool() | trunc
        f = env.episodes.fields()
        out["state"].append(_state_of(torch, obs).clone())
        out["terminated"].append(term.clone())
        out["truncated"].append(trunc.to(torch.uint8))
        out["ended"].append(ended.to(torch.uint8))
        out["finished_return"].append(torch.where(ended, f["last_ret"], torch.zeros_like(f["last_ret"])))
        out["finished_length"].append(torch.where(ended, f["last_length"], torch.zeros_like(f["last_length"])))
        if complete:
            out["refs"].append(env.reference_generator.references.clone())
            out["reward"].append(reward.clone())
    return {k: torch.stack(v) for k, v in out.items() if v}


def _rolled(torch, env, acts):
    """One episodic rollout -> the same dict (clones: the statistics sit in the pipeline's scratch)."""
    if hasattr(env, "reference_generator"):
        state, refs, reward, term, trunc, stats = env.rollout_complete_episodic(acts, episode_statistics=True)
        out = dict(state=state, refs=refs, reward=reward, terminated=term, truncated=trunc)
    else:
        state, term, trunc, stats = env.rollout_episodic(acts, episode_statistics=True)
        out = dict(state=state, terminated=term, truncated=trunc)
    out.update(stats)
    return {k: v.clone() for k, v in out.items()}


def _cat(torch, parts):
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _same(torch, got, want, what=""):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape, got[k].dtype, want[k].dtype)
        if not torch.equal(got[k], want[k]):
            bad = (got[k] != want[k]).reshape(got[k].shape[0], got[k].shape[1], -1).any(-1).nonzero()
            raise AssertionError(f"{what}: {k} differs at {bad.shape[0]} (row, lane) pairs, first {bad[0].tolist()}")
        for lane in EDGE_LANES:  # block edges and the tail, named
            if lane < got[k].shape[1]:
                assert torch.equal(got[k][:, lane], want[k][:, lane]), (what, k, lane)


def _same_afterwards(torch, rolled_env, stepped_env, what=""):
    """The stage's five fields, what `env.truncated` shows, and the ODE state.  The stepped env still has the reset of the envs its last
    step truncated pending; the rolled env has made it inside the launch and must have nothing pending."""
    a, b = rolled_env.episodes, stepped_env.episodes
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)
    assert torch.equal(rolled_env.truncated, stepped_env.truncated) and torch.equal(a.ended, b.ended), what
    assert int(a.reset_mask.sum()) == 0, what
    stepped_env.pipeline.before_step()  # the pending masked reset, as the next step() would apply it
    assert torch.equal(rolled_env.physical_system.get_state(), stepped_env.physical_system.get_state()), what


def _lanes(want):
    term, trunc = want["terminated"].bool().cpu().numpy(), want["truncated"].bool().cpu().numpy()
    return term, trunc


@pytest.mark.parametrize("M", [1, 5, 7, 1000])
@pytest.mark.parametrize("case", sorted(ENVS))
def test_equals_k_steps_bit_for_bit(case, M):
    import torch

    import gym_electric_motor_amd as ga

    rolled_env, stepped_env = _make(ga, case, M), _make(ga, case, M)
    acts = _actions(torch, rolled_env.physical_system, N)
    want = _stepped(torch, stepped_env, acts)
    got = _rolled(torch, rolled_env, acts)
    torch.cuda.synchronize()
    term, trunc = _lanes(want)
    print(f"{case} M={M}: terminated rows {int(term.sum())}, truncated rows {int(trunc.sum())}, lanes never terminating {int((~term.any(0)).sum())}")
    # ---- what the case must exercise, from the stepped env
    if M in (5, 7):
        only_trunc = ~term.any(0) & trunc.any(0)
        assert only_trunc.any(), "no lane truncates without ever terminating"
        if term.any():
            assert (trunc != trunc[:, :1]).any(0).any(), "no lane's truncation rows differ from lane 0's"
    if case == "Cont-CC-PermExDc-v0":
        assert term.sum() > N, "PermExDc under random actions must terminate every few steps"
        if M != 1000:
            assert (trunc != trunc[:, :1]).any(0).any(), "no lane's truncation rows differ from lane 0's"
        if M == 5:
            length_before = np.zeros(N, dtype=np.int64)
            coincide = 0
            for k in range(K):
                length_before += 1
                coincide += int((term[k] & (length_before >= M)).sum())
                length_before[term[k] | trunc[k]] = 0
            assert coincide >= 1, "no row where done and length >= M coincide"
            assert not (term & trunc).any()
    if M == 1000:
        assert not trunc.any()
    if M == 1:
        assert (term | trunc).all()  # every step ends an episode
    _same(torch, got, want, f"{case} M={M}")
    _same_afterwards(torch, rolled_env, stepped_env, f"{case} M={M}")
    launch = rolled_env.physical_system.last_launch()
    assert "episodic_rollout_kernel" in launch, launch
    for env in (rolled_env, stepped_env):
        env.close()


MOTORS = ("PermExDc", "SeriesDc", "ShuntDc", "ExtExDc", "PMSM", "SCIM", "EESM", "DFIM")
# (env id, make keywords, per-env table): every (system, converter unit) behind the ConstantSpeedLoad of the CC envs (RK4, the one-step map
# wherever the stepping kernel takes it), the two dq units; per system the PolynomialStaticLoad of the SC envs, EulerSolver on both loads,
# and one handle with a parameter table (all rows the env's own values: ep_load / ep_apply with every field read)
UNIT_CASES = ([(f"{conv}-CC-{m}-v0", {}, False) for m in MOTORS for conv in ("Finite", "Cont")] +
              [("Cont-CC-PMSM-v0", dict(control_space="dq"), False), ("Cont-CC-SCIM-v0", dict(control_space="dq"), False)] +
              [(f"Cont-SC-{m}-v0", {}, False) for m in MOTORS] +
              [(f"Finite-CC-{m}-v0", dict(ode_solver="euler"), False) for m in MOTORS] + [(f"Cont-SC-{m}-v0", dict(ode_solver="euler"), False) for m in MOTORS] +
              [(f"Cont-CC-{m}-v0", {}, True) for m in MOTORS] + [(f"Finite-SC-{m}-v0", dict(ode_solver="euler"), True) for m in MOTORS])


@pytest.mark.parametrize("env_id, kw, table", UNIT_CASES, ids=[f"{e}-{'-'.join(map(str, k.values())) or 'rk4'}{'-table' if t else ''}" for e, k, t in UNIT_CASES])
def test_every_unit_once(env_id, kw, table):
    """Every episodic unit, and per system every (load, solver, table) form of the kernel, at M = 5 against the stepped env."""
    import torch

    import gym_electric_motor_amd as ga

    kw = dict(kw)
    if kw.get("ode_solver") == "euler":
        kw["ode_solver"] = ga.EulerSolver()
    envs = []
    for _ in range(2):
        if table:
            kw["env_parameters"] = ga.EnvParameters()
        envs.append(_make(ga, env_id, 5, **kw))
    rolled_env, stepped_env = envs
    acts = _actions(torch, rolled_env.physical_system, N, 24)
    want = _stepped(torch, stepped_env, acts)
    assert want["ended"].any() and not want["ended"].all()
    _same(torch, _rolled(torch, rolled_env, acts), want, env_id)
    _same_afterwards(torch, rolled_env, stepped_env, env_id)
    launch = rolled_env.physical_system.last_launch()
    assert f"tab={int(table)}" in launch and f"solver={0 if 'ode_solver' in kw else 1}" in launch and f"load={int('-SC-' in env_id)}" in launch, launch
    for env in envs:
        env.close()


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("case", ["Cont-CC-PermExDc-v0", "Finite-CC-PMSM-v0"])
def test_physics_only_env(case, layout):
    import torch

    import gym_electric_motor_amd as ga

    M = 5
    rolled_env, stepped_env = (_make(ga, case, M, complete=False, obs_layout=layout) for _ in range(2))
    acts = _actions(torch, rolled_env.physical_system, N)
    want = _stepped(torch, stepped_env, acts)
    got = _rolled(torch, rolled_env, acts)
    assert got["state"].shape == ((K, N, got["state"].shape[2]) if layout == "aos" else (K, got["state"].shape[1], N))
    if layout == "soa":  # compare lane by lane in one orientation
        got["state"], want["state"] = got["state"].transpose(1, 2).contiguous(), want["state"].transpose(1, 2).contiguous()
    assert want["truncated"].any() and (case != "Cont-CC-PermExDc-v0" or want["terminated"].any())
    _same(torch, got, want, f"{case} {layout}")
    _same_afterwards(torch, rolled_env, stepped_env, f"{case} {layout}")
    for env in (rolled_env, stepped_env):
        env.close()


@pytest.mark.parametrize("case", ["Cont-CC-PermExDc-v0"])  # (terminations shift the lanes' counters: both traps occur; an env that never terminates truncates at steps 4, 8, ... only)
def test_interleaving_steps_and_rollouts(case):
    """3 steps, a rollout, 2 steps, a rollout == 2K + 5 steps with M = 4: the third step truncates every lane that has not terminated, so
    a reset is pending when the first rollout starts; and rows K-1 of the rollouts truncate lanes that a `step()` follows."""
    import torch

    import gym_electric_motor_amd as ga

    M = 4
    mixed, stepped_env = _make(ga, case, M), _make(ga, case, M)
    acts = _actions(torch, mixed.physical_system, N, 2 * K + 5)
    want = _stepped(torch, stepped_env, acts)
    parts = [_stepped(torch, mixed, acts[:3])]
    pending = int(mixed.episodes.reset_mask.sum())
    parts.append(_rolled(torch, mixed, acts[3:3 + K]))
    assert parts[-1]["truncated"][K - 1].any(), "the rollout's last row truncates no lane"
    assert torch.equal(mixed.truncated, parts[-1]["truncated"][K - 1].bool()) and int(mixed.episodes.reset_mask.sum()) == 0
    parts.append(_stepped(torch, mixed, acts[3 + K:5 + K]))
    pending += int(mixed.episodes.reset_mask.sum())
    assert pending > 0, "no step() left a reset pending in front of a rollout"
    parts.append(_rolled(torch, mixed, acts[5 + K:]))
    _same(torch, _cat(torch, parts), want, case)
    _same_afterwards(torch, mixed, stepped_env, case)
    for env in (mixed, stepped_env):
        env.close()


@pytest.mark.parametrize("n", [3, 256])
def test_block_edges_other_batch_sizes(n):
    import torch

    import gym_electric_motor_amd as ga

    case, M = "Cont-CC-PermExDc-v0", 5
    rolled_env, stepped_env = _make(ga, case, M, n=n), _make(ga, case, M, n=n)
    acts = _actions(torch, rolled_env.physical_system, n)
    want = _stepped(torch, stepped_env, acts)
    assert want["truncated"].any() and want["terminated"].any()
    _same(torch, _rolled(torch, rolled_env, acts), want, f"n={n}")
    _same_afterwards(torch, rolled_env, stepped_env, f"n={n}")
    for env in (rolled_env, stepped_env):
        env.close()


def test_auto_reset_false():
    import torch

    import gym_electric_motor_amd as ga

    case, M = "Cont-CC-PermExDc-v0", 5
    rolled_env, stepped_env = (_make(ga, case, M, auto_reset=False) for _ in range(2))
    assert rolled_env.episodes._cfg.auto_reset_in_kernel == 0
    acts = _actions(torch, rolled_env.physical_system, N)
    want = _stepped(torch, stepped_env, acts)
    assert want["truncated"].any() and want["terminated"].any()
    _same(torch, _rolled(torch, rolled_env, acts), want, "auto_reset=False")
    _same_afterwards(torch, rolled_env, stepped_env, "auto_reset=False")
    for env in (rolled_env, stepped_env):
        env.close()


def test_per_env_parameters():
    """Four parameter sets per wave, M = 5: equals the stepped per-env env; lane 65 equals, rows and ODE state, a uniform episodic handle built with its machine."""
    import torch

    import env_parameters_cases as epc
    import gym_electric_motor_amd as ga

    case, M = "Cont-SC-SCIM-v0", 5
    kw = dict(reference_generator="default", seed=3, max_episode_steps=M, episode_statistics=True)
    rolled_env, stepped_env = (ga.make(epc.env_id_of(case), n_envs=N, env_parameters=epc.env_parameters(case), **epc.make_kwargs(case), **kw) for _ in range(2))
    acts = torch.as_tensor(epc.actions(case)).to(rolled_env.physical_system._tdev).contiguous()
    for env in (rolled_env, stepped_env):
        env.reset()
    want = _stepped(torch, stepped_env, acts)
    got = _rolled(torch, rolled_env, acts)
    assert want["truncated"].any()
    _same(torch, got, want, "per-env")
    _same_afterwards(torch, rolled_env, stepped_env, "per-env")
    launch = rolled_env.physical_system.last_launch()
    assert "episodic_rollout_kernel" in launch and "tab=1" in launch and "per-env parameters" in launch, launch
    lane = 65
    # a uniform handle built with lane 65's machine, given the COMMON limits (a table changes parameters, not the normalisation:
    # tests/test_gpu_env_parameters.py); the physics-only env: its rows are the complete env's state rows
    uni = ga.make(epc.env_id_of(case), n_envs=4, max_episode_steps=M, **epc.uniform_kwargs(case, int(epc.set_of_env("factors")[lane])))
    ups = uni.physical_system
    ups.close()
    for i, v in enumerate(epc.base_env(case).physical_system.limits):
        ups._cfg.limits[i] = float(v)
    ups._create()
    uni.reset()
    rows, term, trunc = uni.rollout_episodic(acts[:, lane:lane + 1].expand(K, 4, acts.shape[2]).contiguous())
    assert "tab=0" in ups.last_launch()
    assert torch.equal(rows[:, 0], got["state"][:, lane]), int((rows[:, 0] != got["state"][:, lane]).any(-1).sum())
    assert torch.equal(term[:, 0], got["terminated"][:, lane]) and torch.equal(trunc[:, 0], got["truncated"][:, lane])
    assert torch.equal(ups.get_state()[:, 0], rolled_env.physical_system.get_state()[:, lane])
    assert not torch.equal(got["state"][:, lane], got["state"][:, lane - 1])  # (the neighbour's machine is another one)
    for env in (rolled_env, stepped_env, uni):
        env.close()


def _stage_cases(ga):
    return {
        "flux-observer": ("Cont-SC-SCIM-v0", dict(physical_system_wrappers=(ga.FluxObserver(),))),
        "flat-cossin": ("dq-PMSM", dict(flatten_observation=True, physical_system_wrappers=(ga.CosSinProcessor(),))),
        "step-generator": ("Cont-CC-PermExDc-v0", None),
        "profile-generator": ("Cont-CC-PermExDc-v0", None),
    }


@pytest.mark.parametrize("stage", ["flux-observer", "flat-cossin", "step-generator", "profile-generator"])
def test_stages_follow_the_ended_rows(stage):
    import torch

    import gym_electric_motor_amd as ga

    case, kw = _stage_cases(ga)[stage]
    M = 5
    envs = []
    for _ in range(2):
        if stage == "step-generator":
            kw = dict(reference_generator=ga.StepReferenceGenerator(reference_state="i", episode_lengths=(3, 9), frequency_range=(100, 800)))
        if stage == "profile-generator":
            profile = 0.5 * np.sin(2 * np.pi * np.linspace(0.0, 1.0, 64))[:, None]  # [T, n_ref]
            kw = dict(reference_generator=ga.ProfileReferenceGenerator(profile, end="wrap", start="random", seed=7))
        envs.append(_make(ga, case, M, **kw))
    rolled_env, stepped_env = envs
    acts = _actions(torch, rolled_env.physical_system, N)
    want = _stepped(torch, stepped_env, acts)
    got = _rolled(torch, rolled_env, acts)
    assert want["truncated"].any()
    _same(torch, got, want, stage)
    _same_afterwards(torch, rolled_env, stepped_env, stage)
    if stage == "flux-observer":
        assert torch.equal(rolled_env.flux.get_state(), stepped_env.flux.get_state())
    for env in envs:
        env.close()


def test_graph_replays_carry_the_counters():
    import torch

    import gym_electric_motor_amd as ga

    case, M = "Cont-CC-PermExDc-v0", 7
    bound_env, stepped_env = _make(ga, case, M), _make(ga, case, M)
    ps = bound_env.physical_system
    acts = _actions(torch, ps, N, 2 * K)
    want = _stepped(torch, stepped_env, acts)
    S, R = len(bound_env.state_names), len(bound_env.reference_names)
    new = lambda *shape, dtype=ps._tdtype: torch.zeros(shape, dtype=dtype, device=ps._tdev)  # noqa: E731
    buf = torch.zeros_like(acts[:K])
    outs = (new(K, N, S), new(K, N, R), new(K, N), new(K, N, dtype=torch.uint8), new(K, N, dtype=torch.uint8))
    stats = dict(ended=new(K, N, dtype=torch.uint8), finished_return=new(K, N, dtype=torch.float64), finished_length=new(K, N, dtype=torch.int32))
    side = torch.cuda.Stream()
    launch = bound_env.bind_rollout_complete_episodic(buf, *outs, stream=side, episode_statistics=stats)
    side.wait_stream(torch.cuda.current_stream())
    start = bound_env.get_checkpoint()
    with torch.cuda.stream(side):  # an eager launch first: the handle's one-step map is built outside a capture
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    torch.cuda.synchronize()
    bound_env.set_checkpoint(start)  # back to where the stepped env started: physics, generators, episode stage
    torch.cuda.synchronize()
    parts = []
    for r in range(2):
        buf.copy_(acts[r * K:(r + 1) * K])
        g.replay()
        torch.cuda.synchronize()
        part = dict(zip(("state", "refs", "reward", "terminated", "truncated"), outs))
        part.update(stats)
        parts.append({k: v.clone() for k, v in part.items()})
    _same(torch, _cat(torch, parts), want, "graph")
    _same_afterwards(torch, bound_env, stepped_env, "graph")
    for env in (bound_env, stepped_env):
        env.close()


@pytest.mark.parametrize("M", [7, 10])
def test_against_the_float64_host_shell(M):
    """`rollout_complete_episodic` of the PMSM, lane by lane, against the float64 HOST shell (tests/env_shell_restatement.py: the fp64 C
    oracle per env, numpy restatements of reward, generators, episode rule and observation -- no code shared with the kernels), under the
    parity module's constants as tests/test_gpu_env_shell.py applies them: values within TOL_FP32 relative to max(max|column|, REL_FLOOR),
    terminated, truncated and the finished lengths exact, a lane compared up to its first close call (constraint margin in the shell below
    DONE_MARGIN), at most 2 % of the lane-steps left out.  Inputs: tests/episodic_rollout_cases.py, whose conditions
    tests/test_episodic_rollout_cpu.py asserts from the shell alone.  The generators' waveform parameters are device streams no host code
    restates: they are read off a stepped twin of the same seed and handed to the shell, which decides when and for whom each set applies."""
    import torch

    import env_shell_cases as cases
    import env_shell_restatement as esr
    import episodic_rollout_cases as erc
    import gym_electric_motor_amd as ga
    import test_gpu_env_shell as shelltest
    from parity_contract import DONE_MARGIN, TOL_FP32

    spec = erc.spec(M)
    acts = cases.actions(spec)
    kw = cases.make_kwargs(ga, spec, "float32")
    twin = ga.make(spec["env_id"], **kw)
    a = torch.as_tensor(acts).to(device="cuda", dtype=twin.physical_system._want_dtype).contiguous()
    seen = [[None] * erc.N for _ in spec["generators"]]
    sets = [[[] for _ in range(erc.N)] for _ in spec["generators"]]
    twin.reset()
    shelltest._collect_params(twin.reference_generator, seen, sets)
    for k in range(erc.K):
        twin.step(a[k])
        shelltest._collect_params(twin.reference_generator, seen, sets)
    twin.close()

    env = ga.make(spec["env_id"], **kw)
    env.reset()
    obs, refs, reward, term, trunc, stats = env.rollout_complete_episodic(a, episode_statistics=True)
    torch.cuda.synchronize()
    assert "episodic_rollout_kernel" in env.physical_system.last_launch()
    host = lambda t: t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()  # noqa: E731
    got = dict(obs=host(obs), rows=host(env.pipeline.raw_scratch), refs=host(refs), reward=host(reward), terminated=host(term), truncated=host(trunc),
               finished_length=host(stats["finished_length"]), finished_return=host(stats["finished_return"]))
    env.close()

    shell = cases.build_shell(ga, spec, sets)
    _, out = shell.run(acts)
    s_term, s_trunc = out["terminated"], out["truncated"]
    assert s_trunc.any() and (M == 7 or (s_term.any() and (s_term.any(axis=0) & s_trunc.any(axis=0)).any()))
    keep = np.arange(erc.K)[:, None] < esr.first_close_call(out["margin"], DONE_MARGIN)[None, :]
    share = 1.0 - float(keep.mean())
    ended = out["ended"]
    want_len = np.where(ended, out["statistics"]["last_length"], 0)
    want_ret = np.where(ended, out["statistics"]["last_ret"], 0.0)
    circle = [c for c, n in enumerate(shell.wrapped) if n == "epsilon"]
    errs = dict(state=shelltest._errors(got["rows"], out["state"], "float32", keep.astype(np.float64), circle),
                observation=shelltest._errors(got["obs"], out["obs"], "float32", keep.astype(np.float64)),
                references=shelltest._errors(got["refs"], out["refs"], "float32", keep),
                reward=shelltest._errors(got["reward"], out["reward"], "float32", keep),
                finished_return=shelltest._errors(got["finished_return"], want_ret, "float32", keep))
    exact = dict(terminated=int(((got["terminated"] != 0) != s_term)[keep].sum()), truncated=int(((got["truncated"] != 0) != s_trunc)[keep].sum()),
                 finished_length=int((got["finished_length"].astype(np.int64) != want_len.astype(np.int64))[keep].sum()))
    print(f"M={M}: errors {({k: f'{v:.1e}' for k, v in errs.items()})}, mismatches {exact}, left out {share:.4f}, terminated rows {int(s_term.sum())}, "
          f"truncated rows {int(s_trunc.sum())}")
    assert share <= 0.02
    assert not any(exact.values()), exact
    assert max(errs.values()) <= TOL_FP32, errs


def test_launch_record_names_the_kind_and_the_unit():
    import torch

    import gym_electric_motor_amd as ga

    env = _make(ga, "Cont-SC-SCIM-v0", 5, n=64)
    ps = env.physical_system
    env.step(_actions(torch, ps, 64, 1)[0])
    assert "episodic" not in ps.last_launch()
    env.rollout_complete_episodic(_actions(torch, ps, 64, 6))
    launch = ps.last_launch()
    s = ps._cfg.system_kind
    unit = re.search(r"conv=(\d+)", launch).group(1)  # (the converter UNIT, dq kinds included: what the stepping kernel's record names too)
    assert "gemx::episodic_rollout_kernel<" in launch and "K=6" in launch and "max_steps=5" in launch and "tab=0" in launch, launch
    assert f"unit libgemx_tl{s}_{unit}.so" in launch and f"sys={s}," in launch, launch
    env.step(_actions(torch, ps, 64, 1)[0])
    stepped = ps.last_launch()
    assert "episodic" not in stepped and f"sys={s},conv={unit}," in stepped, (stepped, launch)  # the same unit as the stepping kernel's
    env.close()
