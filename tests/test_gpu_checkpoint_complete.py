"""The complete env's checkpoint: `get_checkpoint()` of a running env, restored into a DIRTY env of the same configuration, continues
the run bit for bit -- reference generators, references shown, reward, masks, statistics -- for every generator kind, with every device
stage on, with a restart pending, into `rollout_complete` and into a HIP graph captured before the restore, and per shard.

Every test follows one pattern (`_resume`):
    1. env A runs K1 steps;  2. ck = A.get_checkpoint();  3. A runs K2 more steps: the uninterrupted run IS the expected output;
    4. env B, same configuration, is made dirty: reset(), then 3 steps on other actions -- no array of B still holds its create-time
       zero, so a restore that skips an array cannot pass by luck;
    5. B.set_checkpoint(ck), then B runs the same K2 steps.
state, references, reward, terminated and truncated are compared with torch.equal on the BITS at each of the K2 steps; at the end the
generator's state(), episode_statistics() and the two envs' get_checkpoint(), leaf by leaf.  No tolerance anywhere in this file.

Sizes: N = 70 (one whole wave and a partial one: the per-lane arrays and the partial workgroup both matter), K1 = 5, K2 = 7.

What makes each case a test is asserted on the UNINTERRUPTED run A, read from the done masks and the generator's `state()` (never from
the checkpoint code under test).  In the K2 window:
    * at least one env terminates;
    * with a time limit, at least one env truncates;
    * every random generator column starts at least one new sub-episode in at least a quarter of the envs;
    * the switched column starts a new super-episode in at least one env.
The generators' sub-episodes last 2 or 3 steps and the super-episodes 3 or 4 (`episode_lengths=(2, 4)`, `super_episode_length=(3, 5)`,
upper bounds excluded) wherever the case chooses them; `"default"` keeps the env id's 500..2000 steps, and its sub-episodes start with
the restarts of the lanes that terminate.  Every second lane holds the action that drives its machine over the current limit
(tests/env_shell_cases.py: the PMSM under abc (1, -1, -1) in its eighth step, the PermExDc under switch state 2 in its sixth, the SCIM
in its third), the others stay near zero.

And the comparison must be able to fail: for every generator case the same K2 steps on B WITHOUT a restore, and on B restored the way
the env restored before its checkpoint carried the generators (everything but `reference_generator`), differ from A in the references
or the rewards.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import env_shell_cases as shell_cases  # noqa: E402

N, K1, K2 = 70, 5, 7
SEED = 29
SHORT = dict(episode_lengths=(2, 4))
WAVE = dict(frequency_range=(500, 2000), amplitude_range=(0.1, 0.4), offset_range=(-0.2, 0.2), **SHORT)
WALK = dict(sigma_range=(1e-2, 1e-1), **SHORT)
SUPER = (3, 5)
KEYS = ("state", "references", "reward", "terminated", "truncated")


def _bits(t):
    """A tensor's bits: floats compared as integers (bit-equal, not merely equal)."""
    import torch

    t = t.detach().contiguous()
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _equal(x, y):
    import torch

    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def _leaves(tree, path=""):
    """(path, leaf) of a checkpoint, a generator's state() or episode_statistics(): nested dicts / tuples of tensors and numbers."""
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], f"{path}/{k}")
    elif isinstance(tree, (tuple, list)):
        for i, v in enumerate(tree):
            yield from _leaves(v, f"{path}/{i}")
    else:
        yield path, tree


def _assert_same_tree(got, want, what):
    import torch

    got, want = list(_leaves(got)), list(_leaves(want))
    assert [p for p, _ in got] == [p for p, _ in want], (what, [p for p, _ in got], [p for p, _ in want])
    for (p, x), (_, y) in zip(got, want):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and _equal(x, y), (what, p, int((_bits(x) != _bits(y)).sum()) if x.shape == y.shape else (x.shape, y.shape))
        else:
            assert type(x) is type(y) and x == y, (what, p, x, y)


def _snapshot(tree):
    import torch

    if isinstance(tree, dict):
        return {k: _snapshot(v) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return tuple(_snapshot(v) for v in tree)
    return tree.clone() if torch.is_tensor(tree) else tree


def _actions(env, steps, seed, lanes=None):
    """[steps, N, A] (continuous) | [steps, N] uint8 (discrete) device tensor: every second lane holds the action that drives its machine
    over the current limit, the others stay near zero (continuous) or alternate between the two zero-voltage states (discrete)."""
    import torch

    ps = env.physical_system
    n = ps.n_envs
    lane = np.arange(n) if lanes is None else np.asarray(lanes)
    rng = np.random.default_rng(seed)
    hot = (lane % 2 == 0)[None, :]
    space = env.action_space
    if hasattr(space, "n"):
        cold = rng.choice([0, 3], (steps, int(lane.max()) + 1))[:, lane]
        return torch.as_tensor(np.where(hot, 2, cold).astype(np.uint8)).cuda().contiguous()
    A = int(space.shape[0])
    pattern = np.array([1.0] + [-1.0] * (A - 1)) if A != 2 else np.array([1.0, 1.0])  # abc (1, -1, -1); dq (1, 1); one duty cycle: 1
    cold = 0.005 * rng.uniform(-1.0, 1.0, (steps, int(lane.max()) + 1, A))[:, lane]
    return torch.as_tensor(np.where(hot[..., None], pattern, cold)).to(device="cuda", dtype=ps._tdtype).contiguous()


def _new_subepisodes(gen, before):
    """-> (bool [n_ref, N]: the lanes whose generator started a sub-episode in the step just made, the state to compare the next step with).
    A kinds / switched handle tracks the index inside the sub-episode: 1 directly after a start (the lengths are >= 2).  An all-Wiener
    handle does not: there `left` falls by one per step, and is the new length - 1 after a start."""
    s = gen.state()
    if isinstance(s, dict):
        if bool((s["index"] >= 0).any()):
            return (s["index"] == 1).cpu(), None
        left = s["left"]
    else:
        left = s[2]
    left = left.cpu()
    return (left != before - 1) if before is not None else None, left


class _Run:
    """K steps of an env on given actions -> per step the five tensors (clones), and what the generators did meanwhile."""

    def __init__(self, env, acts, track=False):
        import torch

        gen = env.reference_generator
        self.rows = []
        device_gen = hasattr(gen, "state")
        n_ref = len(env.reference_names)
        self.new_sub = torch.zeros((n_ref, env.n_envs), dtype=torch.bool)
        self.n_super = None
        before = _new_subepisodes(gen, None)[1] if track and device_gen else None
        first_super = gen.state().get("n_super") if track and device_gen and isinstance(gen.state(), dict) else None
        for a in acts:
            obs, reward, term, trunc, _ = env.step(a)
            state = obs[0] if isinstance(obs, tuple) else obs
            trunc = trunc.clone() if torch.is_tensor(trunc) else torch.zeros(env.n_envs, dtype=torch.bool, device=state.device)
            self.rows.append(dict(state=state.clone(), references=gen.references.clone(), reward=reward.clone(), terminated=term.clone(), truncated=trunc))
            if track and device_gen:
                new, before = _new_subepisodes(gen, before)
                self.new_sub |= new
        torch.cuda.synchronize()
        if first_super is not None:
            self.n_super = (gen.state()["n_super"] - first_super).cpu()

    def stacked(self, key):
        import torch

        return torch.stack([r[key] for r in self.rows])


def _assert_rows_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got.rows, want.rows)):
        for key in KEYS:
            assert _equal(g[key], w[key]), (what, key, k, int((_bits(g[key]) != _bits(w[key])).sum()))


def _differs(got, want):
    """references or rewards differ somewhere in the window"""
    return any(not _equal(g[key], w[key]) for g, w in zip(got.rows, want.rows) for key in ("references", "reward"))


def _assert_is_a_test(run, random_columns, time_limit, switched_columns=(), what=""):
    """The conditions of the module docstring, on the uninterrupted run's K2 window."""
    term, trunc = run.stacked("terminated"), run.stacked("truncated")
    assert bool(term.any()), (what, "no env terminates in the window")
    assert not time_limit or bool(trunc.any()), (what, "no env truncates in the window")
    for c in random_columns:
        share = float(run.new_sub[c].float().mean())
        assert share >= 0.25, (what, f"column {c} starts a sub-episode in {share:.2f} of the envs only")
    for c in switched_columns:
        assert run.n_super is not None and int((run.n_super[c] > 0).sum()) >= 1, (what, f"column {c} starts no super-episode")


def _dirty(env, seed):
    """reset(), then 3 steps on other actions: nothing of the env holds its create-time zero any more."""
    env.reset()
    for a in _actions(env, 3, seed):
        env.step(a)


def _legacy_restore(env, ck):
    """What `set_checkpoint` restored before the checkpoint carried the generators: everything but `reference_generator`."""
    import gym_electric_motor_amd as ga

    ga.envs.BatchedElectricMotorEnv.set_checkpoint(env, {k: v for k, v in ck.items() if k != "reference_generator"})


def _resume(make, k1=K1, random_columns=(), switched_columns=(), time_limit=False, must_differ=True, conditions=True, what=""):
    """The pattern of the module docstring -> (A, B, ck, actions, A's window) for further checks; both envs are left open."""
    import torch

    A, B = make(), make()
    acts = _actions(A, k1 + K2, SEED)
    A.reset()
    _Run(A, acts[:k1])
    ck = _snapshot(A.get_checkpoint())
    want = _Run(A, acts[k1:], track=True)
    if conditions:
        _assert_is_a_test(want, random_columns, time_limit, switched_columns, what)
    _dirty(B, SEED + 1)
    if must_differ:
        assert _differs(_Run(B, acts[k1:]), want), (what, "the run without a restore equals the uninterrupted one: the comparison proves nothing")
        _legacy_restore(B, ck)
        assert _differs(_Run(B, acts[k1:]), want), (what, "a restore without the generators equals the uninterrupted run: the comparison proves nothing")
    B.set_checkpoint(ck)
    got = _Run(B, acts[k1:])
    _assert_rows_equal(got, want, what)
    ga_, gb = A.reference_generator, B.reference_generator
    if hasattr(ga_, "state"):
        _assert_same_tree(gb.state(), ga_.state(), (what, "generator state"))
    if A.episodes is not None and A.episodes.statistics:
        _assert_same_tree(B.episode_statistics(), A.episode_statistics(), (what, "episode statistics"))
    _assert_same_tree(B.get_checkpoint(), A.get_checkpoint(), (what, "checkpoint after the window"))
    torch.cuda.synchronize()
    return A, B, ck, acts, want


# ---- generator kinds, each without other stages -----------------------------------------------------------------------------------
def _mixed(ga):
    """Cont-SC-PMSM-v0, columns in state order: omega, torque, i_sd, i_sq"""
    return [ga.StepReferenceGenerator(reference_state="omega", **WAVE), ga.SinusoidalReferenceGenerator(reference_state="torque", **WAVE),
            ga.LaplaceProcessReferenceGenerator(reference_state="i_sd", **WALK), ga.ConstReferenceGenerator(reference_state="i_sq", reference_value=-0.125)]


def _switched(ga):
    """Cont-CC-PMSM-v0 (tests/test_gpu_refgen_switched.py, the two-column case): i_sd switched between a Wiener walk and a step, i_sq
    between a constant, a sine and a sawtooth"""
    return [ga.SwitchedReferenceGenerator([ga.WienerProcessReferenceGenerator(reference_state="i_sd", **WALK), ga.StepReferenceGenerator(reference_state="i_sd", **WAVE)],
                                          p=[0.6, 0.4], super_episode_length=SUPER),
            ga.SwitchedReferenceGenerator([ga.ConstReferenceGenerator(reference_state="i_sq", reference_value=-0.125), ga.SinusoidalReferenceGenerator(reference_state="i_sq", **WAVE),
                                           ga.SawtoothReferenceGenerator(reference_state="i_sq", **WAVE)], super_episode_length=SUPER)]


def _replay(ga):
    rng = np.random.default_rng(5)
    return ga.ReplayReferenceGenerator(rng.uniform(-0.5, 0.5, (3 + 3 * K2 + K1 + 2, N, 2)))


# name -> (env id, generator, make keywords, random columns, switched columns)
GENERATOR_CASES = {
    "default-2": ("Cont-CC-PMSM-v0", lambda ga: "default", dict(), (0, 1), ()),
    "default-1": ("Finite-CC-PermExDc-v0", lambda ga: "default", dict(), (0,), ()),
    "mixed": ("Cont-SC-PMSM-v0", _mixed, dict(reward_function=dict(reward_weights=dict(omega=0.25, torque=0.25, i_sd=0.25, i_sq=0.25))), (0, 1, 2), ()),
    "switched": ("Cont-CC-PMSM-v0", _switched, dict(), (0, 1), (0, 1)),
    "replay": ("Cont-CC-PMSM-v0", _replay, dict(), (), ()),
}


def _make_case(case, dtype, n_envs=N, **extra):
    import gym_electric_motor_amd as ga

    env_id, generator, kw, _, _ = GENERATOR_CASES[case]
    return ga.make(env_id, n_envs=n_envs, dtype=dtype, seed=SEED, reference_generator=generator(ga), **dict(kw, **extra))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(GENERATOR_CASES))
def test_generator_kinds(case, dtype):
    _, _, _, random_columns, switched_columns = GENERATOR_CASES[case]
    A, B, ck, _, _ = _resume(lambda: _make_case(case, dtype), random_columns=random_columns, switched_columns=switched_columns, what=(case, dtype))
    assert "reference_generator" in ck and ("row" if case == "replay" else "blob") in ck["reference_generator"]
    if case != "replay":  # the blob's size is the table's sum (tests/test_checkpoint_complete_cpu.py pins the formula to the table)
        from gym_electric_motor_amd import _lib

        n_ref, handle = len(A.reference_names), dict(kinds=case in ("mixed", "switched"), switched=case == "switched")
        assert ck["reference_generator"]["blob"].numel() == A.reference_generator.state_bytes() == _lib.refgen_state_bytes(N, n_ref, **handle)
    A.close(), B.close()


# ---- all stages at once: the cases of tests/env_shell_cases.py, as tests/test_gpu_env_shell.py builds them ---------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", sorted(shell_cases.CASES))
def test_all_stages(case, dtype):
    """State noise, the time limit and the statistics, the flux observer with flux-oriented dq actions, the observation program.  The
    cases' own time limits (5, 8, 10) put a truncation into the window [5, 12); their sub-episodes last 6..11 steps, and every lane's
    generators restart with its episode inside the window."""
    import gym_electric_motor_amd as ga

    spec = shell_cases.CASES[case]
    kw = shell_cases.make_kwargs(ga, dict(spec, N=N), dtype)
    n_ref = len(spec["generators"])
    A, B, ck, _, _ = _resume(lambda: ga.make(spec["env_id"], **shell_cases.make_kwargs(ga, dict(spec, N=N), dtype)), random_columns=range(n_ref), time_limit=True,
                             what=(case, dtype))
    assert kw["max_episode_steps"] == spec["M"] and "episodes" in ck and ("state_noise" in ck) == bool(spec.get("noise")) and ("flux_observer" in ck) == bool(spec.get("observer"))
    A.close(), B.close()


# ---- a checkpoint with a pending restart -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("pending", ["truncated", "terminated"])
def test_pending_restart(pending, dtype):
    """The checkpoint is taken directly after a step in which envs truncated (time limit 5, K1 = 5: every lane) or terminated (K1 = 8:
    the PMSM's hot lanes pass the limit in their eighth step, behind a StateNoiseProcessor of scale 0, which moves the restart in front
    of the next step): the masked reset happens after the restore."""
    import gym_electric_motor_amd as ga

    if pending == "truncated":
        mk = lambda: _make_case("switched", dtype, max_episode_steps=5, episode_statistics=True)  # noqa: E731
        k1 = 5
    else:
        mk = lambda: _make_case("switched", dtype, physical_system_wrappers=(ga.StateNoiseProcessor(["i_sd", "i_sq"], "normal", dict(scale=0)),))  # noqa: E731
        k1 = 8
    A, B, ck, _, _ = _resume(mk, k1=k1, conditions=False, what=(pending, dtype))
    mask = ck["episodes"]["reset_mask"] if pending == "truncated" else ck["state_noise"]["done"]
    assert int(mask.sum()) > 0, "no restart is pending in the checkpoint"
    A.close(), B.close()


# ---- resume into the other entry points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", ["mixed", "switched"])
def test_resume_into_rollout_complete(case, dtype):
    """After set_checkpoint, rollout_complete(actions[K1:]) equals the K2 uninterrupted step()s, stacked."""
    import torch

    _, _, _, random_columns, switched_columns = GENERATOR_CASES[case]
    A, B, ck, acts, want = _resume(lambda: _make_case(case, dtype), random_columns=random_columns, switched_columns=switched_columns, must_differ=False, what=(case, dtype))
    _dirty(B, SEED + 2)
    B.set_checkpoint(ck)
    state, refs, reward, done = B.rollout_complete(acts[K1:])
    torch.cuda.synchronize()
    for key, got in (("state", state), ("references", refs), ("reward", reward), ("terminated", done)):
        assert _equal(got, want.stacked(key)), (key, int((_bits(got) != _bits(want.stacked(key))).sum()))
    _assert_same_tree(B.reference_generator.state(), A.reference_generator.state(), "generator state")
    assert _equal(B.reference_generator.references, A.reference_generator.references)
    A.close(), B.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_resume_into_a_captured_graph(dtype):
    """A bind_step captured in a HIP graph BEFORE set_checkpoint and replayed after it continues the run: the restore replaces nothing
    the binding points at.  (Switched generators, a time limit and the statistics.)"""
    import torch

    # (time limit 9: the hot lanes terminate in their eighth step, the others truncate in the ninth, both inside the window [5, 12))
    mk = lambda: _make_case("switched", dtype, max_episode_steps=9, episode_statistics=True)  # noqa: E731
    A, B, ck, acts, want = _resume(mk, random_columns=(0, 1), switched_columns=(0, 1), time_limit=True, must_differ=False, what=("graph", dtype))
    buf = torch.zeros_like(acts[0])
    side = torch.cuda.Stream()
    step, obs, reward, done = B.bind_step(buf, stream=side)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # dirty again, on the capture stream
        B.reset()
        for a in _actions(B, 3, SEED + 3):
            buf.copy_(a)
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    B.set_checkpoint(ck)
    torch.cuda.synchronize()
    for k in range(K2):
        buf.copy_(acts[K1 + k])
        g.replay()
        torch.cuda.synchronize()
        w = want.rows[k]
        for key, got in (("state", obs[0]), ("references", obs[1]), ("reward", reward), ("terminated", done), ("truncated", B.truncated)):
            assert _equal(got, w[key]), (key, k, int((_bits(got) != _bits(w[key])).sum()))
    _assert_same_tree(B.episode_statistics(), A.episode_statistics(), "episode statistics")
    # all but the two HOST counters, which a replayed graph cannot move: `k` (it only seeds the default step0 of rollout_synthetic) and the
    # informational count of launched steps in the aux blob's header (bytes 40..47: AuxHeader.steps_total, csrc/gemx_capi.hip)
    def device_part(c):
        c = {k: v for k, v in c.items() if k != "k"}
        c["aux"] = c["aux"].clone()
        c["aux"][40:48] = 0
        return c

    _assert_same_tree(device_part(B.get_checkpoint()), device_part(A.get_checkpoint()), "checkpoint after the replays")
    A.close(), B.close()


# ---- shards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shards(dtype):
    """N = 70 as 35 + 35 (`make_sharded`: env_base 0 and 35).  Shard 1's checkpoint is refused by shard 0 and nothing of shard 0 moves;
    each shard's own checkpoint continues what the whole env does on its lanes."""
    import torch

    import gym_electric_motor_amd as ga

    env_id, generator, kw, random_columns, _ = GENERATOR_CASES["mixed"]
    whole = _make_case("mixed", dtype)
    from gym_electric_motor_amd.distributed import make_sharded

    mk = lambda rank: make_sharded(env_id, N, rank, 2, 0, dtype=dtype, seed=SEED, reference_generator=generator(ga), **kw)  # noqa: E731
    shards, fresh = [mk(0), mk(1)], [mk(0), mk(1)]
    assert [s.shard for s in shards] == [(0, 35), (35, 70)]
    acts = _actions(whole, K1 + K2, SEED)
    whole.reset()
    _Run(whole, acts[:K1])
    want = _Run(whole, acts[K1:], track=True)
    _assert_is_a_test(want, random_columns, False, what="shards")
    cks = []
    for s in shards:
        s.reset()
        _Run(s, acts[:K1, s.shard[0]:s.shard[1]].contiguous())
        cks.append(_snapshot(s.get_checkpoint()))
    for rank, s in enumerate(fresh):
        lo, hi = s.shard
        _dirty(s, SEED + 4)
        if rank == 0:
            before = _snapshot(s.get_checkpoint())
            with pytest.raises(ValueError, match="env_base"):
                s.set_checkpoint(cks[1])
            _assert_same_tree(s.get_checkpoint(), before, "shard 0 after the refused restore")
        s.set_checkpoint(cks[rank])
        got = _Run(s, acts[K1:, lo:hi].contiguous())
        for k in range(K2):
            for key in KEYS:
                assert _equal(got.rows[k][key], want.rows[k][key][lo:hi]), (rank, key, k)
    torch.cuda.synchronize()
    for e in [whole] + shards + fresh:
        e.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Each mismatch raises a ValueError that names it, nothing of the env moves (its own checkpoint before and after is the same, leaf by
    leaf), and the env still takes the right checkpoint afterwards and continues the run."""
    import torch

    import gym_electric_motor_amd as ga

    dtype = "float32"
    A, B, ck, acts, want = _resume(lambda: _make_case("mixed", dtype), random_columns=(0, 1, 2), must_differ=False, what="refusals")
    _dirty(B, SEED + 5)
    before = _snapshot(B.get_checkpoint())

    def refused(bad, match):
        with pytest.raises(ValueError, match=match):
            B.set_checkpoint(bad)
        torch.cuda.synchronize()
        _assert_same_tree(B.get_checkpoint(), before, ("after the refusal", match))

    gen_state = ck["reference_generator"]
    # a checkpoint of another n_envs
    half = _make_case("mixed", dtype, n_envs=35)
    half.reset()
    refused(half.get_checkpoint(), "bytes")
    # ... whose blob happens to have this env's size (35 envs x 4 columns = 70 envs x 2): the blob's header names n_envs
    two = ga.BatchedMultipleReferenceGenerator(_mixed(ga)[:2], seed=SEED).set_modules(A.physical_system)
    assert two.state_bytes() == half.reference_generator.state_bytes()
    with pytest.raises(ValueError, match="n_envs"):
        two.set_state(dict(blob=half.reference_generator.get_state()["blob"], references=two.references.clone()))
    # another column count (size), another generator kind (size: an all-Wiener handle owns fewer arrays), another kind in a column (header)
    refused(dict(ck, reference_generator=two.get_state()), "bytes")
    wiener = ga.BatchedWienerProcessReferenceGenerator(reference_states=("omega", "torque", "i_sd", "i_sq"), seed=SEED).set_modules(A.physical_system)
    refused(dict(ck, reference_generator=wiener.get_state()), "bytes")
    swapped = ga.BatchedMultipleReferenceGenerator([ga.SinusoidalReferenceGenerator(reference_state="omega", **WAVE), ga.StepReferenceGenerator(reference_state="torque", **WAVE)]
                                                   + _mixed(ga)[2:], seed=SEED).set_modules(A.physical_system)  # (the kinds on omega and torque swap places)
    assert swapped.state_bytes() == B.reference_generator.state_bytes()
    refused(dict(ck, reference_generator=swapped.get_state()), "another generator kind")
    refused(dict(ck, reference_generator=_replay(ga).set_modules(A.physical_system, default_states=("i_sd", "i_sq")).get_state()), "blob")
    # a truncated blob; a checkpoint without the generators' entry
    refused(dict(ck, reference_generator=dict(gen_state, blob=gen_state["blob"][:-8].clone())), "truncated")
    refused({k: v for k, v in ck.items() if k != "reference_generator"}, "reference_generator")
    refused(A.physical_system.get_checkpoint(), "reference_generator")
    # still usable: the right checkpoint continues the run
    B.set_checkpoint(ck)
    _assert_rows_equal(_Run(B, acts[K1:]), want, "after the refusals")
    for g in (two, wiener, swapped):
        g.close()
    A.close(), B.close(), half.close()
