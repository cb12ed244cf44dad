"""Per-env motor, load and supply parameters on the device (env_parameters=, gemx_set_env_params): lane e of a system with a parameter
table equals, bit for bit, lane e of a uniform system built with lane e's parameter set.

Shape, sets and actions: tests/env_parameters_cases.py (N = 197, K = 48, set = env % 4; the oracle asserts that one set violates its
constraint and one never does).  The uniform systems are built through make() with the set's motor / load / supply and then given the
COMMON limits (those of the env without a table: a table changes parameters, not the normalisation).  For the constant-speed envs a
uniform system may take the one-step linear map, which the per-env kernels never do: there the table env is compared with the fp64 oracle
run per set at the parity contract's tolerance (done masks exact) -- and, bit for bit, with uniform systems created under GEMX_LINMAP=0.
Induction machines against the oracle: the field-oriented columns through their rotation-invariant magnitudes (the frame is undefined at
zero flux, where every episode starts); the bit-for-bit comparisons cover the frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_parameters_cases as cases  # noqa: E402
from parity_contract import REL_FLOOR, TOL_FP32  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import gym_electric_motor_amd as ga  # noqa: E402

N, K = cases.N, cases.K
ALL = list(cases.CASES)
POLY = [c for c in ALL if cases.CASES[c]["poly"]]
CONST = [c for c in ALL if not cases.CASES[c]["poly"]]


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint8 if x.dtype == np.uint8 or x.dtype == bool else np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def table_env(case, **extra):
    return ga.make(cases.env_id_of(case), n_envs=N, env_parameters=cases.env_parameters(case), **cases.make_kwargs(case), **extra)


def with_common_limits(env, case):
    """Re-create the env's handle with the limits of the env without a table."""
    ps = env.physical_system
    ps.close()
    for i, v in enumerate(cases.base_env(case).physical_system.limits):
        ps._cfg.limits[i] = float(v)
    ps._create()
    return env


def uniform_env(case, s, linmap=True):
    old = os.environ.get("GEMX_LINMAP")
    if not linmap:
        os.environ["GEMX_LINMAP"] = "0"
    try:
        return with_common_limits(ga.make(cases.env_id_of(case), n_envs=N, **cases.uniform_kwargs(case, s)), case)
    finally:
        if not linmap:
            os.environ.pop("GEMX_LINMAP") if old is None else os.environ.__setitem__("GEMX_LINMAP", old)


def run_rollout(ps, a):
    ps.reset()
    obs, done = ps.rollout(torch.as_tensor(a, device=f"cuda:{ps.device}"))
    launch = ps.last_launch()
    return obs.cpu().numpy(), done.cpu().numpy(), ps.get_state().cpu().numpy(), launch


def run_steps(ps, a):
    ps.reset()
    at = torch.as_tensor(a, device=f"cuda:{ps.device}")
    obs, done = [], []
    for k in range(len(a)):
        obs.append(ps.simulate(at[k]).clone())
        done.append(ps.done.clone())
    launch = ps.last_launch()
    return torch.stack(obs).cpu().numpy(), torch.stack(done).cpu().numpy(), ps.get_state().cpu().numpy(), launch


_cache = {}


def table_runs(case):
    """The table env's rollout and step x K results, computed once per case and shared."""
    if case not in _cache:
        env = table_env(case)
        a = cases.actions(case)
        _cache[case] = dict(rollout=run_rollout(env.physical_system, a), steps=run_steps(env.physical_system, a))
        env.close()
    return _cache[case]


def assert_exercised(case):
    """The oracle's verdict on the chosen sets: one set violates (and auto-resets) within the K steps, one never does."""
    _, done = cases.oracle_runs(case)
    per_set = [bool(done[:, s::cases.NSETS].any()) for s in range(cases.NSETS)]
    assert any(per_set) and not all(per_set), (case, per_set)


def compare_with_uniform(case, linmap):
    a = cases.actions(case)
    tab = table_runs(case)
    assert "envparams_rollout_kernel" in tab["rollout"][3] and "envparams_step_kernel" in tab["steps"][3], tab
    assert same_bits(tab["rollout"][0], tab["steps"][0]) and same_bits(tab["rollout"][1], tab["steps"][1]) and same_bits(tab["rollout"][2], tab["steps"][2])
    assert tab["rollout"][1].any(), "no lane of the table env terminated: the done path went unexercised"
    for s in range(cases.NSETS):
        env = uniform_env(case, s, linmap=linmap)
        lanes = np.arange(s, N, cases.NSETS)
        for how, run in (("rollout", run_rollout), ("steps", run_steps)):
            obs, done, state, launch = run(env.physical_system, a)
            assert "envparams" not in launch and "kernel" in launch, launch
            t_obs, t_done, t_state, _ = tab[how]
            assert same_bits(t_done[:, lanes], done[:, lanes]), (case, s, how)
            assert same_bits(t_obs[:, lanes], obs[:, lanes]), (case, s, how, float(np.abs(t_obs[:, lanes] - obs[:, lanes]).max()))
            assert same_bits(t_state[:, lanes], state[:, lanes]), (case, s, how)
        env.close()


@pytest.mark.parametrize("case", POLY)
def test_lane_equals_its_uniform_handle(case):
    """Check 1: rows, done bytes and final state of every lane, through step x K and through rollout."""
    assert_exercised(case)
    compare_with_uniform(case, linmap=True)


@pytest.mark.parametrize("case", CONST)
def test_constant_speed_lane_equals_its_uniform_handle_without_the_linear_map(case):
    assert_exercised(case)
    compare_with_uniform(case, linmap=False)


def oracle_error(case, got, got_done):
    ref, ref_done = cases.oracle_runs(case)
    names = list(cases.base_env(case).physical_system.state_names)
    assert np.array_equal(got_done.astype(bool), ref_done), (case, int((got_done.astype(bool) != ref_done).sum()))
    got = got.astype(np.float64)
    cols = {n: i for i, n in enumerate(names)}
    induction = "i_sa" in cols
    worst = 0.0
    skip = set()
    if induction:  # rotation-invariant magnitudes of the field-oriented pairs
        for p, q in (("i_sd", "i_sq"), ("u_sd", "u_sq"), ("i_rd", "i_rq"), ("u_rd", "u_rq")):
            if p in cols:
                skip |= {cols[p], cols[q]}
                mg, mr = np.hypot(got[..., cols[p]], got[..., cols[q]]), np.hypot(ref[..., cols[p]], ref[..., cols[q]])
                worst = max(worst, float(np.abs(mg - mr).max() / max(float(mr.max()), REL_FLOOR)))
    for j, n in enumerate(names):
        if j in skip:
            continue
        d = np.abs(got[..., j] - ref[..., j])
        if n == "epsilon":
            d = np.minimum(d, 2.0 - d)  # normalised angle wraps at +-1
        worst = max(worst, float(d.max() / max(float(np.abs(ref[..., j]).max()), REL_FLOOR)))
    return worst


@pytest.mark.parametrize("case", CONST)
def test_constant_speed_lanes_match_the_fp64_oracle(case):
    """Check 2: every lane against the fp64 oracle run once per set; done masks exact."""
    assert_exercised(case)
    obs, done, _, launch = table_runs(case)["rollout"]
    assert "envparams_rollout_kernel" in launch
    worst = oracle_error(case, obs, done)
    print(f"{case}: worst relative error against the fp64 oracle {worst:.3e}")
    assert worst < TOL_FP32, (case, worst)


@pytest.mark.parametrize("case", ALL)
def test_all_rows_equal_reproduces_the_env_without_a_table(case):
    """Check 3: a table whose rows all equal the env's own parameters.  PolynomialStaticLoad: bit for bit against the env without a table;
    constant speed: bit for bit against it without the linear map, and within the contract's tolerance of it as make() builds it."""
    a = cases.actions(case)
    env = ga.make(cases.env_id_of(case), n_envs=N, env_parameters=ga.EnvParameters(), **cases.make_kwargs(case))
    got = run_rollout(env.physical_system, a)
    assert "envparams_rollout_kernel" in got[3]
    # check 7: clearing the table returns the handle to its previous kernel and results
    env.physical_system.clear_env_parameters()
    plain = run_rollout(env.physical_system, a)
    assert "envparams" not in plain[3]
    env.close()
    old = os.environ.get("GEMX_LINMAP")
    os.environ["GEMX_LINMAP"] = "0"
    try:
        ref_env = ga.make(cases.env_id_of(case), n_envs=N, **cases.make_kwargs(case))
    finally:
        os.environ.pop("GEMX_LINMAP") if old is None else os.environ.__setitem__("GEMX_LINMAP", old)
    ref = run_rollout(ref_env.physical_system, a)
    ref_env.close()
    for i in range(3):
        assert same_bits(got[i], ref[i]), (case, i)
    if cases.CASES[case]["poly"]:
        for i in range(3):
            assert same_bits(got[i], plain[i]), (case, i)
    else:
        assert np.array_equal(got[1], plain[1])
        g, p = got[0].astype(np.float64), plain[0].astype(np.float64)
        names = list(cases.base_env(case).physical_system.state_names)
        d = np.abs(g - p)
        if "epsilon" in names:
            j = names.index("epsilon")
            d[..., j] = np.minimum(d[..., j], 2.0 - d[..., j])
        err = (d.reshape(-1, d.shape[-1]).max(0) / np.maximum(np.abs(p).reshape(-1, d.shape[-1]).max(0), REL_FLOOR)).max()
        assert err < TOL_FP32, (case, err)


def test_clear_returns_the_handle_to_its_previous_kernel():
    """Check 7 on the closed-loop path: step kernel before, per-env kernel with the table, the same step kernel and bits after."""
    case = "Cont-SC-SCIM-v0"
    a = cases.actions(case)
    env = ga.make(cases.env_id_of(case), n_envs=N, **cases.make_kwargs(case))
    ps = env.physical_system
    before = run_steps(ps, a[:8])
    ps.set_env_parameters(cases.env_parameters(case))
    with_table = run_steps(ps, a[:8])
    tab = ps.get_env_parameter_table()
    assert tab.shape[1] == N and torch.isfinite(tab).all()
    ps.clear_env_parameters()
    after = run_steps(ps, a[:8])
    env.close()
    assert "step_kernel" in before[3] and "envparams" not in before[3] and "envparams_step_kernel" in with_table[3] and after[3] == before[3]
    assert all(same_bits(after[i], before[i]) for i in range(3))
    assert not same_bits(with_table[0], before[0])


def test_two_half_size_shards_equal_one_whole():
    """Check 4, bit for bit."""
    from gym_electric_motor_amd.distributed import make_sharded, shard_range

    case = "Cont-SC-SCIM-v0"
    a = cases.actions(case)
    whole = table_runs(case)["rollout"]
    for rank in range(2):
        lo, hi = shard_range(N, rank, 2)
        env = make_sharded(cases.env_id_of(case), N, rank, 2, 0, env_parameters=cases.env_parameters(case), **cases.make_kwargs(case))
        got = run_rollout(env.physical_system, a[:, lo:hi])
        env.close()
        assert "envparams_rollout_kernel" in got[3]
        assert same_bits(got[0], whole[0][:, lo:hi]) and same_bits(got[1], whole[1][:, lo:hi]) and same_bits(got[2], whole[2][:, lo:hi])


COMPLETE = dict(reference_generator="default", max_episode_steps=20, episode_statistics=True, seed=5)


def complete_steps(env, a, k0=0, k1=None):
    at = torch.as_tensor(a, device="cuda:0")
    out = []
    for k in range(k0, len(a) if k1 is None else k1):
        (state, ref), reward, term, trunc, _ = env.step(at[k])
        trunc = trunc if torch.is_tensor(trunc) else torch.zeros_like(term, dtype=torch.bool)  # (no time limit: False)
        out.append((state.clone(), ref.clone(), reward.clone(), term.clone(), trunc.clone()))
    return [torch.stack([o[i] for o in out]).cpu().numpy() for i in range(5)]


def started(env, at):
    """reset, two warm-up steps, reset: every env of the test below gets this history (the graphed one needs the warm-up before its capture)."""
    env.reset()
    for k in range(2):
        env.step(at[k])
    env.reset()
    return env


def test_complete_env_steps_rollout_graph_and_checkpoint():
    """Checks 5 and 6 on Cont-SC-SCIM-v0.  Every run starts from a FRESH env of the same seed (a second reset() of one env draws the
    generators' next episodes).  The fused K-step rollouts refuse a time limit, so `rollout_complete` is compared on the env without one."""
    case = "Cont-SC-SCIM-v0"
    a = cases.actions(case)
    at = torch.as_tensor(a, device="cuda:0")
    nolimit = dict(reference_generator="default", episode_statistics=True, seed=5)
    # K calls of step == rollout_complete stacked; the state rows are check 1's
    env = started(table_env(case, **nolimit), at)
    free = complete_steps(env, a)
    assert "envparams_rollout_kernel" in env.physical_system.last_launch()  # (K = 1 with the fused reward)
    env.close()
    assert same_bits(free[0], table_runs(case)["steps"][0])
    env = started(table_env(case, **nolimit), at)
    state, refs, reward, done = env.rollout_complete(at)[:4]
    assert "envparams_rollout_kernel" in env.physical_system.last_launch()
    env.close()
    assert same_bits(state, free[0]) and same_bits(refs, free[1]) and same_bits(reward, free[2]) and same_bits(done.to(torch.uint8), free[3].astype(np.uint8))
    assert free[3].any()
    # with the time limit: 48 eager steps, a checkpoint on the way at step 24
    env = started(table_env(case, **COMPLETE), at)
    first = complete_steps(env, a, 0, 24)
    ck = env.get_checkpoint()
    second = complete_steps(env, a, 24, K)
    env.close()
    eager = [np.concatenate([x, y]) for x, y in zip(first, second)]
    assert eager[4].any(), "no env was truncated: the time limit went unexercised"
    assert "env_parameters" in ck and tuple(ck["env_parameters"].shape) == (26, N)
    fresh = table_env(case, **COMPLETE)
    fresh.reset()
    fresh.set_checkpoint(ck)
    resumed = complete_steps(fresh, a, 24, K)
    fresh.close()
    for i in range(5):
        assert same_bits(resumed[i], eager[i][24:]), i
    plain = ga.make(cases.env_id_of(case), n_envs=N, **cases.make_kwargs(case), **COMPLETE)
    with pytest.raises(ValueError, match="per-env parameters"):
        plain.set_checkpoint(ck)
    plain.close()
    # HIP graph: 16 bound steps captured once, replayed three times == the 48 eager steps
    env = table_env(case, **COMPLETE)
    buf = torch.zeros_like(at[0])
    chunk = torch.zeros_like(at[:16])
    rows = torch.zeros((16,) + tuple(eager[0].shape[1:]), device="cuda:0")
    stream = torch.cuda.Stream()
    step, (state, _), _, _ = env.bind_step(buf, stream=stream)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # the history of `started`, on the capture stream
        env.reset()
        for k in range(2):
            buf.copy_(at[k])
            step()
        env.reset()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            for k in range(16):
                buf.copy_(chunk[k])
                step()
                rows[k].copy_(state)
    got = []
    for r in range(3):
        chunk.copy_(at[16 * r:16 * r + 16])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got.append(rows.clone())
    env.close()
    assert same_bits(torch.cat(got), eager[0])
    # a fresh env of OTHER per-env parameters (the sets shifted by one env): same shape, other values -- refused before anything is restored
    other = ga.make(cases.env_id_of(case), n_envs=N, env_parameters=cases.env_parameters(case, sets=(np.arange(N) + 1) % cases.NSETS),
                    **cases.make_kwargs(case), **COMPLETE)
    other.reset()
    before = other.physical_system.get_state().clone()
    with pytest.raises(ValueError, match="per-env parameter table differs in value"):
        other.set_checkpoint(ck)
    assert same_bits(other.physical_system.get_state(), before)
    other.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The fused reward of the per-env rollout kernel against independent producers of the same numbers: the existing kernels of uniform
# handles (lane by lane), and the complete env without a table.
# ---------------------------------------------------------------------------------------------------------------------------------------
def reward_kwargs(names, which):
    """set_reward keywords over the first states of an env.
    hot:     two referenced states, powers 1 and 2 -- the terms the kernel holds by value (GEMX_REWARD_HOT = 4)
    slow:    five or six weighted states, three of them referenced -- the terms beyond the hot ones go through the description in memory
    general: powers other than 1 and 2 -- EVERY term goes through the description in memory and pow()"""
    if which == "hot":
        return dict(reward_weights={names[0]: 0.4, names[2]: 0.6}, reward_power={names[0]: 1, names[2]: 2}, referenced_states=(names[0], names[2]))
    if which == "slow":
        m = min(6, len(names))
        return dict(reward_weights={names[i]: 0.1 + 0.05 * i for i in range(m)}, reward_power={names[i]: 1 + i % 2 for i in range(m)},
                    referenced_states=(names[0], names[1], names[3]), bias="positive", violation_reward=-7.5)
    m = min(5, len(names))
    return dict(reward_weights={names[i]: 0.2 for i in range(m)}, reward_power={names[i]: (0.5, 3, 1, 2, 1.5)[i] for i in range(m)},
                referenced_states=(names[1],), gamma=0.8)


REWARD_KINDS = ("hot", "slow", "general")


def run_rewarded(ps, a, refs, steps=False):
    """-> obs [K, N, S], done [K, N], reward [K, N], launch: one fused K-step launch, or K launches of one step."""
    at, rt = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(refs, device="cuda:0")
    ps.reset()
    if not steps:
        obs, done, reward = ps.rollout(at, references=rt)
    else:
        out = []
        for k in range(len(a)):
            o = ps.simulate(at[k], references=rt[k])
            out.append((o.clone(), ps.done.clone(), ps.reward.clone()))
        obs, done, reward = (torch.stack([x[i] for x in out]) for i in range(3))
    return obs.cpu().numpy(), done.cpu().numpy(), reward.cpu().numpy(), ps.last_launch()


@pytest.mark.parametrize("case", ALL)
def test_fused_reward_of_every_lane_equals_its_uniform_handles(case):
    """Rows, done bytes and the reward computed in the launch (`rollout(actions, references=)`, `simulate(action, references=)`), lane by lane
    and bit for bit against uniform systems, whose launches are the existing kernels: three reward descriptions, seeded references."""
    a = cases.actions(case)
    names = list(cases.base_env(case).physical_system.state_names)
    rng = np.random.default_rng(23)
    kws = {w: reward_kwargs(names, w) for w in REWARD_KINDS}
    refs = {w: rng.uniform(-0.8, 0.8, (K, N, len(kws[w]["referenced_states"]))).astype(np.float32) for w in REWARD_KINDS}
    env = table_env(case)
    ps = env.physical_system
    tab = {}
    for w in REWARD_KINDS:
        ps.set_reward(**kws[w])
        tab[w] = run_rewarded(ps, a, refs[w])
        stepped = run_rewarded(ps, a, refs[w], steps=True)
        assert "envparams_rollout_kernel" in tab[w][3] and "K=48" in tab[w][3] and "envparams_rollout_kernel" in stepped[3] and "K=1," in stepped[3]
        for i in range(3):
            assert same_bits(tab[w][i], stepped[i]), (case, w, i)
        done = tab[w][1].astype(bool)
        assert done.any() and not done.all()
        assert np.isfinite(tab[w][2]).all() and len(np.unique(tab[w][2][~done])) > N  # (rewards that follow the rows, not one constant)
    env.close()
    for s in range(cases.NSETS):
        env = uniform_env(case, s, linmap=cases.CASES[case]["poly"])
        ps = env.physical_system
        lanes = np.arange(s, N, cases.NSETS)
        for w in REWARD_KINDS:
            ps.set_reward(**kws[w])  # (on the handle re-created with the common limits)
            obs, done, reward, launch = run_rewarded(ps, a, refs[w])
            assert "envparams" not in launch and "kernel" in launch, launch
            assert same_bits(tab[w][0][:, lanes], obs[:, lanes]) and same_bits(tab[w][1][:, lanes], done[:, lanes]), (case, s, w)
            assert same_bits(tab[w][2][:, lanes], reward[:, lanes]), (case, s, w, float(np.abs(tab[w][2][:, lanes] - reward[:, lanes]).max()))
        env.close()


@pytest.mark.parametrize("case", POLY)
def test_complete_env_with_all_rows_equal_reproduces_the_complete_env_without_a_table(case):
    """State, references, reward and terminated of a complete env whose table rows all equal its own parameters against the same env
    without a table (the existing kernels compute its reward): K calls of `step` and `rollout_complete`, bit for bit."""
    a = cases.actions(case)
    at = torch.as_tensor(a, device="cuda:0")
    got = []
    for kw in (dict(env_parameters=ga.EnvParameters()), dict()):
        def fresh():
            return started(ga.make(cases.env_id_of(case), n_envs=N, reference_generator="default", seed=5, **cases.make_kwargs(case), **kw), at)
        env = fresh()
        steps = complete_steps(env, a)[:4]
        step_launch = env.physical_system.last_launch()
        env.close()
        env = fresh()
        state, refs, reward, done = env.rollout_complete(at)[:4]
        roll_launch = env.physical_system.last_launch()
        env.close()
        got.append((steps, [x.cpu().numpy() for x in (state, refs, reward, done.to(torch.uint8))], step_launch, roll_launch))
    table, plain = got
    assert "envparams_rollout_kernel" in table[2] and "envparams_rollout_kernel" in table[3]
    assert "envparams" not in plain[2] and "envparams" not in plain[3] and "kernel" in plain[2] and "kernel" in plain[3]
    # (every env is the default machine here, which in some cases never violates within K steps: the violation reward of terminated lanes is
    # asserted in test_fused_reward_of_every_lane_equals_its_uniform_handles, whose sets do terminate)
    assert np.isfinite(plain[0][2]).all() and len(np.unique(plain[0][2])) > N
    for i in range(4):
        assert same_bits(table[0][i], plain[0][i]), (case, "step", i)
        assert same_bits(table[1][i], plain[1][i]), (case, "rollout_complete", i)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The library's own checks (gemx_set_env_params, the launch forms), which Python's refusals otherwise keep out of reach
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_library_checks_the_arrays_itself_and_changes_nothing_on_a_failure():
    from gym_electric_motor_amd import _lib, env_parameters as epm

    C = _lib.C
    env = ga.make("Cont-SC-PMSM-v0", n_envs=8)
    ps = env.physical_system
    L = ps._L
    good = ga.EnvParameters(motor={"r_s": np.linspace(15.0, 20.0, 8)}).resolve(ps)
    cols = _lib.MODEL_COLS

    def call(arrays, n_envs=8, struct_size=None):
        p = epm.GemxEnvParams()
        p.struct_size = C.sizeof(epm.GemxEnvParams) if struct_size is None else struct_size
        p.n_envs = n_envs
        keep = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items() if v is not None}
        for k, v in keep.items():
            setattr(p, k, v.ctypes.data)
        rc = L.gemx_set_env_params(ps._handle, C.byref(p))
        return rc, L.gemx_last_error().decode()

    def changed(key, index, value):
        arr = {k: v.copy() for k, v in good.items()}
        arr[key][index] = value
        return arr

    outside = (_lib.MODEL_ROWS - 1) * cols + cols - 1  # the matrix's last entry: in no synchronous machine's pattern
    bad = [
        (call(good, struct_size=8), "size mismatch"),
        (call(good, n_envs=7), "the arrays hold 7 envs, the handle 8"),
        (call(changed("j_total", 3, np.nan)), "j_total[3] is not finite"),
        (call(changed("u_nominal", 7, np.inf)), "u_nominal[7] is not finite"),
        (call(changed("model", (2, 0), -np.inf)), "model[" + str(2 * good["model"].shape[1]) + "] is not finite"),
        (call(changed("torque_coef", (1, 1), np.nan)), "torque_coef[5] is not finite"),
        (call(changed("load_b", 0, np.nan)), "load_b[0] is not finite"),
        (call(changed("j_total", 5, 0.0)), "j_total[5] = 0 must be positive"),
        (call(changed("j_total", 6, -1e-3)), "j_total[6]"),
        (call(changed("model", (4, outside), 1.0)), "env 4: model[%d][%d] = 1 is outside the sparsity pattern" % (_lib.MODEL_ROWS - 1, cols - 1)),
        (call(changed("model", (5, 2 * cols), good["model"][5, 2 * cols] + 1.0)), "env 5 has pole pair entry"),
    ]
    for (rc, msg), what in bad:
        assert rc == -1 and what in msg and ("per-env parameters" in msg or "gemx_env_params" in msg), (rc, msg, what)
    # nothing changed: the handle has no table, and steps with the kernel it always launched
    out = torch.empty((epm.table_fields(_lib.SYS_SYNC), 8), device="cuda:0")
    assert L.gemx_get_env_params(ps._handle, C.c_void_p(out.data_ptr()), None) == -1 and "no parameter table" in L.gemx_last_error().decode()
    ps.reset()
    ps.simulate(torch.zeros((8, 3), device="cuda:0"))
    assert "envparams" not in ps.last_launch()
    # a good call (NULL arrays: the handle's own values), then a bad one: the table stays what the good call made it
    assert call(dict(good, load_a=None, load_b=None, load_c=None, torque_coef=None))[0] == 0
    assert L.gemx_get_env_params(ps._handle, C.c_void_p(out.data_ptr()), None) == 0
    kept = out.clone()
    assert call(changed("j_total", 2, np.nan))[0] == -1
    first = torch.empty_like(out)
    assert L.gemx_get_env_params(ps._handle, C.c_void_p(first.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, kept) and any(len(torch.unique(kept[f])) == 8 for f in range(kept.shape[0]))  # (r_s differs per env)
    # the launch forms the per-env kernels do not serve, asked of the library directly
    a = torch.zeros((4, 8, 3), device="cuda:0")
    for launch, what in ((lambda: ps.rollout_synthetic(4), "gemx_rollout_synthetic"), (lambda: ps.rollout(a.half()), "gemx_rollout_half"),
                         (lambda: ps.rollout(a, last_only=True), "last-step-only")):
        with pytest.raises(ValueError, match="per-env parameters.*" + what):
            launch()
    assert L.gemx_clear_env_params(ps._handle) == 0
    ps.rollout(a, last_only=True)
    assert "envparams" not in ps.last_launch()
    env.close()


@pytest.mark.parametrize("kw, what", [
    (dict(dtype="float64"), "fp32 handles only"),
    (dict(ode_solver=ga.ScipyOdeSolver()), "error-controlled Dormand-Prince"),
    (dict(ode_solver=ga.DormandPrince5Solver()), "solver kind"),
    (dict(converter=dict(interlocking_time=1e-6)), "interlocking time"),
    (dict(physical_system_wrappers=(ga.DeadTimeProcessor(steps=1),)), "DeadTimeProcessor"),
    (dict(supply=ga.RCVoltageSupply(u_nominal=400.0)), "RCVoltageSupply"),
    (dict(motor=dict(motor_initializer=dict(random_init="uniform"))), "random initial states"),
])
def test_the_library_refuses_what_the_per_env_kernels_do_not_serve(kw, what):
    """The refusals of tests/test_env_parameters_cpu.py, asked of gemx_set_env_params on a real handle (Python's own check bypassed)."""
    from gym_electric_motor_amd import env_parameters as epm

    env = ga.make("Cont-SC-PMSM-v0", n_envs=8, **kw)
    ps = env.physical_system
    arrays = ga.EnvParameters().resolve(ps)
    with pytest.raises(ValueError, match="per-env parameters") as err:
        epm.install(ps, arrays)
    assert what in str(err.value)
    ps.reset()
    ps.simulate(torch.zeros((8, 3), dtype=ps._tdtype, device="cuda:0"))
    assert "envparams" not in ps.last_launch()
    env.close()
