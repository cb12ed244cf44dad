"""GPU tests of the device-side profile references (`ga.ProfileReferenceGenerator`, csrc/gemx_refprofile.hip) against the float64 host
restatement (tests/refprofile_restatement.py): exact table reads, linear interpolation, the step / rollout / shell-rollout contract, the
complete env against a ReplayReferenceGenerator run, restarts on termination and truncation, HIP-graph replay, random start rows by
property, shards by env_base, and the checkpoint.

Shapes: N = 70 (a full wave and a partial one, unaligned) and N = 1, T = 5 rows, K = 7 steps (the end is crossed), n_ref in {1, 2, MAX_REF},
fp32 and fp64; done masks with restarts at row 0, at the last row and on lanes 63 / 64 / 69."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (sibling module: the restatement)

from refprofile_restatement import Profiles  # noqa: E402

T, K = 5, 7
STATES = {1: ("i_sq",), 2: ("i_sd", "i_sq"), 4: ("omega", "torque", "i_sd", "i_sq")}  # (in the state order of the PMSM system)
# interpolated values: |x| <= 1, w exact in double, one fma in the working dtype (ProfileReferenceGenerator's definition) -- fp32: the
# roundings of w (2^-24 relative, times |b - a| <= 2), of b - a and of the result stay below 2^-22; fp64: below 1e-15
TOL = {"float32": 2.0 ** -22, "float64": 1e-15}


class _System:
    """What the generator's set_modules reads of a physical system (a PMSM's), for generators tested on their own."""

    def __init__(self, ps, n_envs, dtype, env_base=0):
        self.state_positions, self.state_space, self.state_names, self.tau = ps.state_positions, ps.state_space, ps.state_names, ps.tau
        self.n_envs, self.env_base, self.device = n_envs, env_base, ps.device
        self._tdev, self._tdtype = ps._tdev, dtype


@pytest.fixture(scope="module")
def host():
    import gym_electric_motor_amd as ga

    env = ga.make("Cont-CC-PMSM-v0", n_envs=2)
    yield env.physical_system
    env.close()


def _table(n, n_ref, per_env, dtype, rows=T, seed=1):
    """normalised values of the working dtype, as float64 (what the device table holds)"""
    shape = (rows, n, n_ref) if per_env else (rows, n_ref)
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dtype).astype(np.float64)


def _done(n, seed=0):
    """[K, N] uint8: restarts at row 0, at the last row and on lanes 63 / 64 / 69 (N = 1: on lane 0), and a few more"""
    d = (np.random.default_rng(seed).random((K, n)) < 0.1).astype(np.uint8)
    for row, lane in ((0, 0), (0, 64), (K - 1, 63), (K - 1, 0), (2, 63), (3, 64), (4, 69), (K - 1, 69)):
        d[row, min(lane, n - 1)] = 1
    return d


def _gen(host, n, dtype, table, n_ref, env_base=0, **kw):
    import torch

    import gym_electric_motor_amd as ga

    holder = ga.ProfileReferenceGenerator(table, reference_states=STATES[n_ref], **kw)
    return ga.ProfileReferences(holder).set_modules(_System(host, n, getattr(torch, dtype), env_base))


def _state_equals(gen, want):
    got = gen.state()
    return all(np.array_equal(got[f].cpu().numpy().astype(np.int64), want.state()[f]) for f in ("k", "s", "e"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_ref", [1, 2, 4])
@pytest.mark.parametrize("n", [70, 1])
def test_exact_table_reads(host, dtype, n_ref, n):
    """Rows sampled at tau, or zero-order hold of rows at 2.5 tau: every value shown is the table entry itself, bit for bit; shared and
    per-env tables, both end rules; k, s, e are the restatement's."""
    import torch

    done = _done(n)
    d_dev = torch.as_tensor(done).cuda()
    for per_env in (False, True):
        table = _table(n, n_ref, per_env, dtype)
        for end in ("hold", "wrap"):
            for kw in (dict(), dict(profile_tau=2.5 * host.tau, interpolation="hold")):
                g = _gen(host, n, dtype, table, n_ref, end=end, **kw)
                ref = Profiles(table, n, ratio=g.ratio, interpolation="hold", end=end)
                assert g.ratio == (1.0 if not kw else host.tau / (2.5 * host.tau))
                g.reset()
                ref.reset()
                got = g.rollout_shell(K, d_dev)
                assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == (K, n, n_ref)
                assert np.array_equal(got.double().cpu().numpy(), ref.rollout_shell(K, done)), (per_env, end, kw)
                assert _state_equals(g, ref)
                got = g.rollout(K, d_dev)  # (goes on from there, restarts after the row)
                assert np.array_equal(got.double().cpu().numpy(), ref.rollout(K, done)), (per_env, end, kw)
                assert _state_equals(g, ref)
                g.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_ref", [1, 2, 4])
@pytest.mark.parametrize("n", [70, 1])
def test_linear_interpolation(host, dtype, n_ref, n):
    """Rows at 2.5 tau, interpolated: within one fma's rounding of the exact value (TOL); positions that fall on a row show the entry."""
    import torch

    done = _done(n, seed=3)
    d_dev = torch.as_tensor(done).cuda()
    for per_env in (False, True):
        table = _table(n, n_ref, per_env, dtype, seed=2)
        for end in ("hold", "wrap"):
            g = _gen(host, n, dtype, table, n_ref, end=end, profile_tau=2.5 * host.tau)
            ref = Profiles(table, n, ratio=g.ratio, end=end)
            g.reset(), ref.reset()
            for call in ("rollout_shell", "rollout", "rollout_shell"):  # (21 steps: positions up to 8.4 rows, the end is crossed)
                got = getattr(g, call)(K, d_dev).double().cpu().numpy()
                want = getattr(ref, call)(K, done)
                err = float(np.abs(got - want).max())
                print(f"{dtype} n_ref={n_ref} N={n} per_env={per_env} end={end} {call}: max |device - float64| = {err:.3e} (bound {TOL[dtype]:.3e})")
                assert err <= TOL[dtype]
            assert _state_equals(g, ref)
            g.close()
    # no done: the wave stays on one row (the uniform table path)
    table = _table(n, n_ref, False, dtype, seed=4)
    g = _gen(host, n, dtype, table, n_ref, profile_tau=2.5 * host.tau)
    ref = Profiles(table, n, ratio=g.ratio)
    got = g.rollout_shell(K).double().cpu().numpy()
    assert float(np.abs(got - ref.rollout_shell(K)).max()) <= TOL[dtype]
    assert np.array_equal(got[0], np.broadcast_to(table[0], (n, n_ref)))  # (position 0: the entry itself)
    g.close()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_ref", [1, 2, 4])
def test_step_rollout_and_shell_rollout(host, dtype, n_ref):
    """rollout_shell(done, K) == K x step(done[k]) bit for bit (interpolating, per-env table, wrap); rollout(done, K) restarts after the
    row; step, rollout, reset and rollout_shell mixed on one handle follow the restatement; `out=` views off the row alignment."""
    import torch

    n = 70
    done = _done(n, seed=5)
    d_dev = torch.as_tensor(done).cuda()
    table = _table(n, n_ref, True, dtype, seed=6)
    kw = dict(end="wrap", profile_tau=2.5 * host.tau)
    a, b = _gen(host, n, dtype, table, n_ref, **kw), _gen(host, n, dtype, table, n_ref, **kw)
    a.reset(), b.reset()
    want = a.rollout_shell(K, d_dev)
    buf = torch.empty(n * n_ref + 1, dtype=want.dtype, device="cuda")
    odd = buf[1:].view(n, n_ref)  # (not aligned to a row of 2 or 4: the scalar stores)
    for k in range(K):
        got = b.step(d_dev[k], out=odd if k % 2 else None)
        assert torch.equal(got, want[k]), k
    for x, y in zip(a.state().values(), b.state().values()):
        assert torch.equal(x, y)
    a.close(), b.close()
    # exact reads, so that the host restatement is bit for bit: a mixed sequence on one handle
    for per_env in (False, True):
        table = _table(n, n_ref, per_env, dtype, seed=7)
        g, ref = _gen(host, n, dtype, table, n_ref, end="wrap"), Profiles(table, n, end="wrap")
        g.reset(), ref.reset()
        same = lambda x, y: np.array_equal(x.double().cpu().numpy(), y)  # noqa: E731
        assert same(g.step(), ref.step())
        assert same(g.rollout(K, d_dev), ref.rollout(K, done))
        assert same(g.step(d_dev[1]), ref.step(done[1]))
        g.reset(d_dev[4]), ref.reset(done[4])
        assert same(g.rollout_shell(K, d_dev), ref.rollout_shell(K, done))
        assert same(g.rollout(3), ref.rollout(3))
        assert same(g.step(d_dev[0]), ref.step(done[0]))
        assert _state_equals(g, ref)
        assert torch.equal(g.references, g.step(out=g.references))  # (the buffer the generator owns is what step() writes)
        g.close()


def _env(ga, gen, n=70, **kw):
    return ga.make("Cont-CC-PMSM-v0", n_envs=n, reference_generator=gen, seed=5, **kw)


def _cycle(rows):
    """a two-column cycle [rows, 2], column 0: i_sd, column 1: i_sq, every row different"""
    t = np.arange(rows)
    return np.stack([-0.3 + 0.01 * t, 0.4 - 0.01 * t], axis=1).astype(np.float32).astype(np.float64)


def test_complete_env_equals_a_replayed_run():
    """start zero, rows at tau, a shared table longer than the run, no termination: step() x K and rollout_complete with the profile
    generator equal the same run with a ReplayReferenceGenerator bit for bit -- state, refs, reward, done."""
    import torch

    import gym_electric_motor_amd as ga

    n = 70
    prof = _cycle(2 * K + 2)
    acts = torch.as_tensor(np.random.default_rng(8).uniform(-0.2, 0.2, (K, n, 3)).astype(np.float32)).cuda()

    def run(gen):
        env = _env(ga, gen, n)
        (state, ref), _ = env.reset()
        rows = [(state.clone(), ref.clone(), None, None)]
        for k in range(K):
            (state, ref), reward, terminated, truncated, _ = env.step(acts[k])
            rows.append((state.clone(), ref.clone(), reward.clone(), terminated.clone()))
        fused = [t.clone() for t in env.rollout_complete(acts)]  # (goes on: rows K + 1 .. 2 K of the profile)
        torch.cuda.synchronize()
        env.close()
        return rows, fused

    rows_r, fused_r = run(ga.ReplayReferenceGenerator(prof))
    assert not any(bool(r[3].any()) for r in rows_r[1:]) and not bool(fused_r[3].any())  # the replayed run has no done
    rows_p, fused_p = run(ga.ProfileReferenceGenerator(prof))
    for k, (r, p) in enumerate(zip(rows_r, rows_p)):
        for x, y in zip(r, p):
            assert (x is None and y is None) or torch.equal(x, y), k
    want = torch.as_tensor(prof).float().cuda()
    assert torch.equal(torch.stack([p[1] for p in rows_p]), want[:K + 1, None, :].expand(-1, n, -1))
    for x, y in zip(fused_r, fused_p):
        assert torch.equal(x, y)
    assert torch.equal(fused_p[1], want[K + 1:2 * K + 1, None, :].expand(-1, n, -1))


def test_a_terminated_env_restarts_its_profile():
    """Envs under full voltage terminate: with the profile generator the reference a terminated env shows next is its start row again;
    with a ReplayReferenceGenerator it is the next row of the walk."""
    import torch

    import gym_electric_motor_amd as ga

    n, steps = 70, 400
    prof = _cycle(steps + 2)
    want = torch.as_tensor(prof).float().cuda()
    action = torch.ones((n, 3), device="cuda") * torch.tensor([1.0, -1.0, -1.0], device="cuda")
    seen = {}
    for name, gen in (("profile", ga.ProfileReferenceGenerator(prof)), ("replay", ga.ReplayReferenceGenerator(prof))):
        env = _env(ga, gen, n)
        env.reset()
        for k in range(steps):
            (state, ref), reward, terminated, _, _ = env.step(action)
            if bool(terminated.any()):
                t = terminated.bool()
                seen[name] = (k, ref[t].clone(), ref[~t].clone())
                if name == "profile":  # and it walks on from there
                    (state, ref2), _, term2, _, _ = env.step(action)
                    assert torch.equal(ref2[t & ~term2.bool()], want[1].expand(int((t & ~term2.bool()).sum()), -1))
                    s = env.reference_generator.state()
                    assert bool((s["e"][t] >= 2).all()) and bool((s["e"][~t & ~term2.bool()] == 1).all())
                break
        torch.cuda.synchronize()
        env.close()
    assert set(seen) == {"profile", "replay"}, "no env terminated"
    k, restarted, others = seen["profile"]
    assert k >= 1 and torch.equal(restarted, want[0].expand(restarted.shape[0], -1))  # the start row again
    assert torch.equal(others, want[k + 1].expand(others.shape[0], -1))
    k_r, restarted_r, others_r = seen["replay"]
    assert k_r == k and torch.equal(restarted_r, want[k + 1].expand(restarted_r.shape[0], -1))  # `done` is ignored there


def test_a_truncated_env_restarts_its_profile():
    """max_episode_steps = 3: every env is truncated at its third step and shows its start row again."""
    import torch

    import gym_electric_motor_amd as ga

    n = 70
    prof = _cycle(12)
    want = torch.as_tensor(prof).float().cuda()
    env = _env(ga, ga.ProfileReferenceGenerator(prof), n, max_episode_steps=3, constraints=())
    (state, ref), _ = env.reset()
    assert torch.equal(ref, want[0].expand(n, -1))
    action = torch.zeros((n, 3), device="cuda")
    shown = []
    for k in range(7):
        (state, ref), reward, terminated, truncated, _ = env.step(action)
        assert not bool(terminated.any()) and bool(truncated.all()) == (k % 3 == 2)
        shown.append(int(torch.nonzero((want == ref[0]).all(dim=1))[0]))
        assert torch.equal(ref, ref[0].expand(n, -1))
    assert shown == [1, 2, 0, 1, 2, 0, 1]
    torch.cuda.synchronize()
    env.close()


def test_bound_step_in_a_hip_graph_equals_eager_steps():
    """One `bind_step` captured with torch.cuda.graph and replayed 6 times (T = 5, end 'wrap': the end is crossed) equals 6 eager steps
    of a twin env bit for bit: the position lives on the device, so the replays advance it."""
    import torch

    import gym_electric_motor_amd as ga

    n = 70
    prof = _cycle(T)
    kw = dict(end="wrap")

    def loop(env, stream):
        action = torch.full((n, 3), 0.05, device="cuda")
        step, (state, ref), reward, done = env.bind_step(action, stream=stream)
        return step, state, ref, reward, done

    env, twin = _env(ga, ga.ProfileReferenceGenerator(prof, **kw), n), _env(ga, ga.ProfileReferenceGenerator(prof, **kw), n)
    side = torch.cuda.Stream()
    step, state, ref, reward, done = loop(env, side)
    step_t, state_t, ref_t, reward_t, done_t = loop(twin, torch.cuda.current_stream())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start
        for _ in range(3):
            step()
        env.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _ in range(3):
        step_t()
    twin.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    assert torch.equal(ref, ref_t)  # (the capture executed nothing)
    shown = []
    for k in range(6):
        graph.replay()
        step_t()
        torch.cuda.synchronize()
        assert torch.equal(state, state_t) and torch.equal(ref, ref_t) and torch.equal(reward, reward_t) and torch.equal(done, done_t), k
        shown.append(ref[0].clone())
    assert all(not torch.equal(shown[i], shown[i + 1]) for i in range(5))  # the replays advanced the profile
    assert int(env.reference_generator.state()["k"][0]) == 7
    env.close()
    twin.close()


def test_bound_rollout_in_a_hip_graph_goes_on_from_the_first_replay():
    """bind_rollout_complete captured and replayed twice equals two eager rollout_complete calls of a twin: the second replay goes on
    from where the first one ended."""
    import torch

    import gym_electric_motor_amd as ga

    n = 70
    prof = _cycle(T)
    env, twin = (_env(ga, ga.ProfileReferenceGenerator(prof, end="wrap"), n) for _ in range(2))
    acts = torch.as_tensor(np.random.default_rng(9).uniform(-0.2, 0.2, (K, n, 3)).astype(np.float32)).cuda()
    shapes = env._complete_shapes(K)
    outs = [torch.zeros(s, device="cuda") for s in shapes[:3]] + [torch.zeros(shapes[3], dtype=torch.uint8, device="cuda")]
    side = torch.cuda.Stream()
    launch = env.bind_rollout_complete(acts, *outs, stream=side)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream, then a fresh start
        launch()
        env.reset()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    twin.rollout_complete(acts)
    twin.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    torch.cuda.synchronize()
    want_rows = torch.as_tensor(prof).float().cuda()
    for i in range(2):
        graph.replay()
        want = twin.rollout_complete(acts)
        torch.cuda.synchronize()
        for x, y in zip(outs, want):
            assert torch.equal(x, y), i
        assert not bool(outs[3].any())
        idx = (1 + i * K + torch.arange(K, device="cuda")) % T  # rows 1 + i K, ... of the cycle, modulo T
        assert torch.equal(outs[1], want_rows[idx][:, None, :].expand(-1, n, -1))
    assert int(env.reference_generator.state()["k"][0]) == 1 + 2 * K
    env.close()
    twin.close()


def test_random_start_rows(host):
    """start='random', by property: s in [0, T - 1] and the rows shown are the table's from s on; the same seed reproduces them; envs and
    episodes differ; two half-size shards with env_base 0 and 35 show what one handle of 70 shows."""
    import torch

    n, rows = 70, 4096
    table = _table(n, 2, False, "float32", rows=rows, seed=10)
    kw = dict(start="random", seed=12, end="wrap")
    g, twin = _gen(host, n, "float32", table, 2, **kw), _gen(host, n, "float32", table, 2, **kw)
    other = _gen(host, n, "float32", table, 2, **dict(kw, seed=13))
    for x in (g, twin, other):
        x.reset()
    s1 = g.state()["s"].cpu().numpy()
    assert s1.min() >= 0 and s1.max() <= rows - 1 and len(set(s1.tolist())) >= 2  # two envs differ
    assert np.array_equal(twin.state()["s"].cpu().numpy(), s1) and not np.array_equal(other.state()["s"].cpu().numpy(), s1)
    got = g.rollout_shell(3).double().cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], table[(s1 + k) % rows])
    assert torch.equal(twin.rollout_shell(3), torch.as_tensor(got).float().cuda())
    mask = np.zeros(n, np.uint8)
    mask[[0, 5, 63, 64, 69]] = 1
    g.reset(torch.as_tensor(mask).cuda())
    st = g.state()
    s2 = st["s"].cpu().numpy()
    assert np.array_equal(s2[mask == 0], s1[mask == 0]) and not np.array_equal(s2[mask == 1], s1[mask == 1])  # two episodes of one env differ
    assert s2.min() >= 0 and s2.max() <= rows - 1
    assert np.array_equal(st["e"].cpu().numpy(), 1 + mask) and np.array_equal(st["k"].cpu().numpy(), np.where(mask, 0, 3))
    assert np.array_equal(g.step().double().cpu().numpy(), table[(s2 + np.where(mask, 0, 3)) % rows])
    # end 'hold' with T = 5: s reaches both ends over 70 envs x 3 episodes, and never leaves [0, T - 1]
    small = _gen(host, n, "float32", _table(n, 2, False, "float32"), 2, start="random", seed=1)
    seen = set()
    for _ in range(3):
        small.reset()
        seen |= set(small.state()["s"].cpu().numpy().tolist())
    assert seen == set(range(T))
    for x in (g, twin, other, small):
        x.close()
    # shards: per-env table, two masked resets (one through step's done byte)
    table = _table(n, 2, True, "float32", rows=rows, seed=11)
    whole = _gen(host, n, "float32", table, 2, **kw)
    halves = [_gen(host, 35, "float32", table[:, lo:lo + 35], 2, env_base=lo, **kw) for lo in (0, 35)]
    m1, m2 = ((np.random.default_rng(s).random(n) < 0.5).astype(np.uint8) for s in (20, 21))
    outs = []
    for x, sl in ((whole, slice(0, n)), (halves[0], slice(0, 35)), (halves[1], slice(35, 70))):
        x.reset()
        a = x.step().clone()
        x.reset(torch.as_tensor(m1[sl]).cuda())
        b = x.step().clone()
        c = x.step(torch.as_tensor(m2[sl]).cuda()).clone()
        outs.append((a, b, c, torch.stack(list(x.state().values()))))
    for j in range(3):
        assert torch.equal(outs[0][j], torch.cat([outs[1][j], outs[2][j]])), j
    assert torch.equal(outs[0][3], torch.cat([outs[1][3], outs[2][3]], dim=1))
    for x in [whole] + halves:
        x.close()


def test_checkpoint_continues_the_run():
    """get_checkpoint() in mid-run, set_checkpoint() into a fresh env and into the same env behind a captured bind_step: the run continues
    bit for bit; a blob of another N, n_ref, T or shard raises ValueError before anything is restored."""
    import torch

    import gym_electric_motor_amd as ga

    n = 70
    prof = _cycle(T)
    kw = dict(end="wrap", start="random", seed=4)
    action = torch.full((n, 3), 0.05, device="cuda")
    env = _env(ga, ga.ProfileReferenceGenerator(prof, **kw), n)
    side = torch.cuda.Stream()
    step, (state, ref), reward, done = env.bind_step(action, stream=side)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.reset()
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    ck = env.get_checkpoint()
    assert ck["reference_generator"]["blob"].numel() == 64 + 12 * n
    want = []
    for _ in range(4):
        graph.replay()
        torch.cuda.synchronize()
        want.append((state.clone(), ref.clone(), reward.clone(), done.clone()))
    # a fresh env continues with eager steps
    fresh = _env(ga, ga.ProfileReferenceGenerator(prof, **kw), n)
    fresh.reset()
    fresh.set_checkpoint(ck)
    for k in range(4):
        (s, r), rew, term, _, _ = fresh.step(action)
        torch.cuda.synchronize()
        assert torch.equal(s, want[k][0]) and torch.equal(r, want[k][1]) and torch.equal(rew, want[k][2]) and torch.equal(term, want[k][3]), k
    # the same env, behind its captured step
    env.set_checkpoint(ck)
    torch.cuda.synchronize()
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(state, want[k][0]) and torch.equal(ref, want[k][1]) and torch.equal(reward, want[k][2]) and torch.equal(done, want[k][3]), k
    # blobs of another configuration: refused, and the generator is where it was
    before = {f: v.clone() for f, v in fresh.reference_generator.state().items()}
    others = dict(N=_env(ga, ga.ProfileReferenceGenerator(prof, **kw), 35),
                  n_ref=_env(ga, ga.ProfileReferenceGenerator(prof[:, :1], reference_states="i_sq", **kw), n),
                  T=_env(ga, ga.ProfileReferenceGenerator(_cycle(T + 1), **kw), n),
                  shard=_env(ga, ga.ProfileReferenceGenerator(prof, **kw), n, env_base=35))
    for what, other in others.items():
        other.reset()
        bad = other.reference_generator.get_state()
        with pytest.raises(ValueError):
            fresh.reference_generator.set_state(bad)
        if what in ("T", "shard"):  # (the same sizes: the blob's header tells them apart)
            with pytest.raises(ValueError, match="T = 6 rows" if what == "T" else "env_base = 35"):
                fresh.reference_generator.set_state(bad)
        other.close()
    torch.cuda.synchronize()
    for f, v in fresh.reference_generator.state().items():
        assert torch.equal(v, before[f]), f
    env.close()
    fresh.close()
