"""Every eager K-step rollout and its bound counterpart launched once agree bit for bit on every returned tensor, the episode
statistics dict included, and leave the episode stage in the same state.  Both forms are built from one plan (envs.py: `_plan`); this
holds the pairs together on the device: `rollout` / `bind_rollout` (with an observation stage and `episode_statistics`),
`rollout_episodic` / `bind_rollout_episodic`, `rollout_policy_episodic` / `bind_rollout_policy_episodic`, `rollout_complete` /
`bind_rollout_complete` and `rollout_complete_episodic` / `bind_rollout_complete_episodic`.  Two envs built and reset identically, the
eager form on one, the bound form on the other, into zeroed tensors of its own.

The shapes are those of tests/test_gpu_pipeline_forms.py, whose docstring establishes the terminations on the fp64 CPU oracle: N = 70 (one
full wave and a partial one), float32, auto-reset on, every third env at full voltage (1, -1, -1):

* Cont-CC-PMSM, K = 8, a column program: the hot envs pass the current limit in the eighth step, row 7;
* Cont-CC-SCIM, K = 3, a FluxObserver: the hot envs pass it in the third step, row 2.

The episodic families run the SCIM with `max_episode_steps=3` over K = 8 rows: two whole episodes and the start of a third.  A hot env
terminates in its third step -- rows 2 and 5, from the reset state both times, and a step that terminates and reaches the limit at once
counts as terminated --, every other env is truncated there, and rows 3 and 6 are the first of restarted episodes.  (The PMSM cannot
terminate under that limit: it needs eight steps.)  The policy reads the raw row, so its env has no stage; its hot lanes are driven
through the `noise` input, which the squash saturates to the same full voltage.

Cells other tests already assert are left to them: `rollout_complete` against `bind_rollout_complete` without episode statistics
(both against K steps: tests/test_gpu_pipeline_forms.py, the observer shapes; tests/test_gpu_complete_rollout.py:
test_bound_rollout_in_a_hip_graph_equals_eager_launches, no stage), and `bind_rollout_complete_episodic` without a stage against steps
(tests/test_gpu_episodic_rollout.py: test_graph_replays_carry_the_counters).  Here those two families carry `episode_statistics` and a
stage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SEED, M = 70, 5, 3
HOT = (1.0, -1.0, -1.0)
PROGRAM = ["omega", "i_sd", "i_sq", "cos(epsilon)", "sin(epsilon)"]
OBSERVED = ["omega", "i_sd", "i_sq", "psi_abs", "psi_angle"]
# family -> (motor, K, complete, episodic)
CASES = {
    "rollout-program": ("PMSM", 8, False, False),
    "rollout-observer": ("SCIM", 3, False, False),
    "episodic-observer": ("SCIM", 8, False, True),
    "policy": ("SCIM", 8, False, True),
    "complete-program": ("PMSM", 8, True, False),
    "complete-observer": ("SCIM", 3, True, False),
    "complete_episodic-observer": ("SCIM", 8, True, True),
}


def _make(ga, family):
    motor, _, complete, episodic = CASES[family]
    kw = dict(episode_statistics=True)
    if family.endswith("program"):
        kw.update(physical_system_wrappers=(ga.CosSinProcessor(remove_angle=True),), observed_states=PROGRAM, flatten_observation=complete)
    if family.endswith("observer"):
        kw.update(physical_system_wrappers=(ga.FluxObserver(),), observed_states=OBSERVED)
    if complete:
        kw.update(reference_generator="default")
    if episodic:
        kw.update(max_episode_steps=M)
    env = ga.make(f"Cont-CC-{motor}-v0", n_envs=N, dtype="float32", auto_reset=True, seed=SEED, **kw)
    env.reset()
    return env


def _zeros_like(torch, result):
    """Zeroed tensors of the caller's own in the shapes and dtypes of an eager result: the outputs, and the statistics dict."""
    return [torch.zeros_like(t) for t in result[:-1]], {k: torch.zeros_like(v) for k, v in result[-1].items()}


@pytest.mark.parametrize("family", sorted(CASES))
def test_the_eager_form_equals_its_bound_form_launched_once(family):
    import torch

    import gym_electric_motor_amd as ga

    _, K, complete, episodic = CASES[family]
    hot = torch.arange(N) % 3 == 0
    small = 0.005 * (torch.rand((K, N, 3), generator=torch.Generator().manual_seed(SEED), dtype=torch.float64) * 2 - 1)
    acts = torch.where(hot[None, :, None], torch.tensor(HOT, dtype=torch.float64), small).float().cuda().contiguous()
    eager_env, bound_env = _make(ga, family), _make(ga, family)
    if family == "policy":
        n_state = len(eager_env.physical_system.state_names)
        rng = np.random.default_rng(SEED)
        policy = ga.MLPPolicy([(0.01 * rng.standard_normal((16, n_state)), np.zeros(16)), (0.01 * rng.standard_normal((3, 16)), np.zeros(3))])
        noise = torch.where(hot[None, :, None], 20.0 * torch.tensor(HOT, dtype=torch.float64), small).float().cuda().contiguous()  # (tanh(+-20) is +-1 in fp32)
        want = eager_env.rollout_policy_episodic(policy, K, noise=noise, episode_statistics=True)
        outs, stats = _zeros_like(torch, want)
        got = bound_env.bind_rollout_policy_episodic(policy, K, *outs, noise=noise, episode_statistics=stats)()
    else:
        name = ("rollout_complete" if complete else "rollout") + ("_episodic" if episodic else "")
        want = getattr(eager_env, name)(acts, episode_statistics=True)
        outs, stats = _zeros_like(torch, want)
        got = getattr(bound_env, "bind_" + name)(acts, *outs, episode_statistics=stats)()
    torch.cuda.synchronize()
    assert len(got) == len(want) == (2 + 2 * complete + episodic + (family == "policy") + 1)
    assert all(g is o for g, o in zip(got, outs)) and all(got[-1][key] is t for key, t in stats.items())  # (the caller's own tensors)
    for i, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (family, i, int((g != w).sum()), "of", g.numel())
    assert sorted(got[-1]) == sorted(want[-1]) == ["ended", "finished_length", "finished_return"]
    for key, w in want[-1].items():
        g = got[-1][key]
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (family, key, int((g != w).sum()), "of", g.numel())
    # masks that are all zero prove nothing: the hot envs terminate where the oracle's do, the others are truncated at the limit
    hot = hot.cuda()
    if episodic:
        terminated, truncated, ended = want[-3].bool(), want[-2].bool(), want[-1]["ended"].bool()
        print(f"{family}: K={K}, {int(terminated.sum())} terminations, {int(truncated.sum())} truncations")
        assert terminated.any() and truncated.any()
        for row in (2, 5):
            assert terminated[row, hot].all() and truncated[row, ~hot].all() and not truncated[row, hot].any()
        assert not terminated[:2, hot].any() and not truncated[:2].any() and torch.equal(ended, terminated | truncated)
        assert int(want[-1]["finished_length"][5].min()) == M  # (the second episode started inside the rows, and was counted from its restart)
    else:
        done = want[-2].bool()
        print(f"{family}: K={K}, {int(done.sum())} terminations, first in row {int(done.any(dim=1).nonzero()[0])}")
        assert done[K - 1, hot].all() and not done[:K - 1, hot].any()
    # ... and both envs go on from the same episode counters
    for key, w in eager_env.episode_statistics().items():
        assert torch.equal(bound_env.episode_statistics()[key], w), (family, key)
    if episodic:
        assert torch.equal(bound_env.truncated, eager_env.truncated)
    eager_env.close(), bound_env.close()
